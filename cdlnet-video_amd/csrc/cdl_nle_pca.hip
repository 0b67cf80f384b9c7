// Blind noise-level estimation by weak-texture PCA (reference model/nle.py:29-89, nle_pca): the device half.
// One call = one pass of one channel: for every p x p patch of channel c over the whole batch, its texture
// strength
//     Xtr = sum over the p x (p-2) window of ((x[i][j] - x[i][j+2]) / 2)^2 + the same over (p-2) x p along rows,
// the predicate  keep = Xtr < tau  (tau = +inf keeps every patch), and the p^2 x p^2 second moment of the kept
// patches,  G = sum_kept x x^T  (non-centred, as the reference's X X^T), plus an integer count of them.  The host
// (nle.py) divides by count - 1 and takes the smallest eigenvalue.
//
// Layout of the work.  A persistent grid of workgroups walks 32 x 32 tiles of patch origins (a tile never spans two
// samples).  Per tile: the image tile plus its (p-1) halo goes to LDS, then the squared half-differences, then Xtr and
// the keep flag of each patch (a 0/1 weight w), then the Gram on v_mfma_f32_32x32x2_f32 with K = patches:
// the patch vector is padded to PP = 64 (p^2 < 64) or 128 (p^2 < 128) and only the lower 32 x 32 tiles are formed
// (3 of 4, or 10 of 16).  PP = 64: every wave forms all 3 tiles over a quarter of the patches; PP = 128: wave w forms
// tiles w, w+4, w+8 over all of them.
//
// Precision.  The smallest eigenvalue is ~sigma^2, orders of magnitude below the Gram's largest (~p^2 mean^2), so
// an fp32 Gram of raw pixels would not hold it.  Three things keep it:
//   - each workgroup subtracts a shift m (one pixel of its first tile, rounded to 8 mantissa bits) and accumulates
//     D = sum w d d^T of d = x - m, whose entries scale with the local variance rather than with mean^2;
//   - row p^2 of the padded vector carries the constant 1, so D's row p^2 holds s = sum w d and D[p^2][p^2] the
//     number of kept patches; then  G = D + m (s 1^T + 1 s^T) + n m^2 1 1^T  is rebuilt in fp64;
//   - the fp32 MFMA chain runs over one tile (<= 1024 patches); each tile's result is added to fp64 registers.
// The per-workgroup fp64 partials are reduced in a fixed order (two stages), so repeated calls are bit-identical.
// The count is integer throughout (patch counts above 2^24 stay exact); all offsets into y are 64-bit.
//
// Domains.  The patches that pool into one Gram form a domain.  cdl_nle_pca_gram has one: every
// patch of the batch.  cdl_nle_pca_gram_cells has one per sample and cell of a regular grid of window x window pixel
// cells (`step` apart, the last of an axis flush with the border): only patches wholly inside the cell, its own tau.
// Both run the same three launches.  Domain d owns the gpd consecutive workgroups d * gpd .. of the Gram kernel, which
// walk the domain's own 32 x 32 tiles of origins (tile g, g + gpd, ...), so a partial belongs to exactly one domain;
// the domain of a workgroup and the cell's first pixel follow from the block index and the grid descriptor.  The two
// reduction kernels take the domain as grid dimension z.  One domain (gpd = the whole grid) is the whole-image call.
// The length of the fp32 MFMA chains is launch-uniform too: a tile's whole slice for the whole-image domain (its bits
// are those of the one-chain-per-tile form), CELL_CHAIN patches for a cell, each chain added into the fp64 registers.
#include "cdl_common.h"

namespace {

constexpr int P_MIN = 3, P_MAX = 11;
constexpr int TR = 32, TC = 32, TP = TR * TC;             // patch origins per tile
constexpr int LH = TR + P_MAX - 1, LWP = TC + P_MAX;       // LDS image rows, row pitch (one spare column)
constexpr int LIMG = LH * LWP;
constexpr int NTHREADS = 256;
constexpr int RED_CHUNK = 16;                              // partials per stage-1 reduction block
constexpr int GRID_PP64 = 512, GRID_PP128 = 512;           // persistent grid: 2 workgroups per CU (register-bound)
constexpr int LDS_FLOATS = 3 * LIMG + TP;                  // image, squared h / v differences, patch weights
static_assert(LDS_FLOATS >= 3 * 1024 * 2, "the PP = 64 wave reduction reuses the tile buffers (3 tiles, fp64)");

typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int tiles_of(int nb) { return nb * (nb + 1) / 2; }
// lower 32 x 32 tile (I >= J) -> index I (I + 1) / 2 + J
__device__ __forceinline__ int tile_index(int I, int J) { return I * (I + 1) / 2 + J; }

struct Shape {
    int N, C, H, W, c, p, P2;
    int Hp, Wp;                // patch origins per sample of a domain
    int tr, tc;                // tiles per sample of a domain
    long long ntiles;          // tiles of a domain
    // the domains: ny x nx cells of wh x ww pixels per group of dn pooled samples (the whole image: 1 x 1 cells of
    // H x W, dn = N)
    int wh, ww, step, ny, nx, dn;
    int gpd;                   // workgroups per domain
    int chain;                 // patches per fp32 MFMA chain; 0: a tile's whole slice
    long long nd;              // domains
};

// first pixel of cell i along an axis of L pixels with cells of w: min(i * step, L - w)
__device__ __forceinline__ int cell_start(int i, int step, int L, int w) { return min(i * step, L - w); }

// partial layout: part[g][tile][row][col] (fp64, 32 x 32 per tile of the shifted D), shift[g], count[g]
template <int NB>
__global__ __launch_bounds__(NTHREADS) void k_pca_gram(const float *__restrict__ y, Shape s,
                                                       const float *__restrict__ taus, float tau1,
                                                       double *__restrict__ part, double *__restrict__ shift,
                                                       long long *__restrict__ count)
{
    constexpr int NT = tiles_of(NB);
    constexpr int MAXT = 3;                    // tiles per wave
    constexpr int SLICE = NB == 2 ? TP / 4 : TP;
    __shared__ float lds[LDS_FLOATS];
    __shared__ unsigned long long s_count;
    float *img = lds, *gh = lds + LIMG, *gv = lds + 2 * LIMG, *wk = lds + 3 * LIMG;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = s.p, P2 = s.P2;
    const int LH_used = TR + p - 1, LW_used = TC + p - 1;
    // this workgroup's domain d, its place g among the domain's workgroups, the domain's first sample and pixel
    const long long d = blockIdx.x / s.gpd;
    const int g = (int)(blockIdx.x % s.gpd);
    const int cell = (int)(d % ((long long)s.ny * s.nx));
    const long long n0 = d / ((long long)s.ny * s.nx) * s.dn;
    const int R0 = cell_start(cell / s.nx, s.step, s.H, s.wh), C0 = cell_start(cell % s.nx, s.step, s.W, s.ww);
    const int R1 = R0 + s.wh, C1 = C0 + s.ww;                // one past the domain's last pixel
    const float tau = taus ? taus[d] : tau1;
    const bool keep_all = __builtin_isinf(tau) && tau > 0.0f;
    const int kbase = NB == 2 ? wave * SLICE : 0;

    // this wave's tiles and, per tile, the lane's A (row block I) and B (column block J) element:
    // value = sc * img[base + off] + ad, times the patch weight (pixel: sc 1, ad -m; row P2: 0, 1; padding: 0, 0)
    int tI[MAXT], tJ[MAXT];
    bool tv[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int ti = NB == 2 ? t : wave + 4 * t;
        tv[t] = ti < NT;
        int I = 0;
        while (tiles_of(I + 1) <= ti) ++I;
        tI[t] = I;
        tJ[t] = ti - tiles_of(I);
    }

    if (tid == 0) s_count = 0;
    unsigned long long my_count = 0;

    // shift: the pixel at the middle of this workgroup's first tile, rounded to bf16 precision
    float m = 0.0f;
    {
        const long long t0 = g;
        const long long n = n0 + t0 / ((long long)s.tr * s.tc);
        const int rem = (int)(t0 % ((long long)s.tr * s.tc));
        const int r = min(R0 + (rem / s.tc) * TR + TR / 2, R1 - 1), c = min(C0 + (rem % s.tc) * TC + TC / 2, C1 - 1);
        const float v = y[(((size_t)n * s.C + s.c) * s.H + r) * s.W + c];
        m = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & 0xffff0000u);
    }

    int offA[MAXT], offB[MAXT];
    float scA[MAXT], adA[MAXT], scB[MAXT], adB[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int a = tI[t] * 32 + (lane & 31), b = tJ[t] * 32 + (lane & 31);
        offA[t] = a < P2 ? (a / p) * LWP + a % p : 0;
        scA[t] = a < P2 ? 1.0f : 0.0f;
        adA[t] = a < P2 ? -m : (a == P2 ? 1.0f : 0.0f);
        offB[t] = b < P2 ? (b / p) * LWP + b % p : 0;
        scB[t] = b < P2 ? 1.0f : 0.0f;
        adB[t] = b < P2 ? -m : (b == P2 ? 1.0f : 0.0f);
    }

    double acc64[MAXT][16];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc64[t][r] = 0.0;

    const long long per_n = (long long)s.tr * s.tc;
    for (long long tile = g; tile < s.ntiles; tile += s.gpd) {
        const long long n = n0 + tile / per_n;
        const int rem = (int)(tile % per_n);
        const int r0 = R0 + (rem / s.tc) * TR, c0 = C0 + (rem % s.tc) * TC;
        const float *src = y + ((size_t)n * s.C + s.c) * s.H * (size_t)s.W;

        __syncthreads();                                   // the previous tile's readers are done
        for (int e = tid; e < LH_used * LW_used; e += NTHREADS) {
            const int i = e / LW_used, j = e % LW_used;
            const int gi = r0 + i, gj = c0 + j;
            img[i * LWP + j] = (gi < R1 && gj < C1) ? src[(size_t)gi * s.W + gj] : 0.0f;
        }
        __syncthreads();
        // squared half-differences: the reference's conv2d with [1/2, 0, -1/2], then **2
        for (int e = tid; e < LH_used * LW_used; e += NTHREADS) {
            const int i = e / LW_used, j = e % LW_used;
            float h = 0.0f, v = 0.0f;
            if (j + 2 < LW_used) {
                const float d = 0.5f * img[i * LWP + j] - 0.5f * img[i * LWP + j + 2];
                h = d * d;
            }
            if (i + 2 < LH_used) {
                const float d = 0.5f * img[i * LWP + j] - 0.5f * img[(i + 2) * LWP + j];
                v = d * d;
            }
            gh[i * LWP + j] = h;
            gv[i * LWP + j] = v;
        }
        __syncthreads();
        // texture strength and keep flag per patch origin
        for (int k = tid; k < TP; k += NTHREADS) {
            const int pr = k / TC, pc = k % TC;
            float w = 0.0f;
            if (r0 - R0 + pr < s.Hp && c0 - C0 + pc < s.Wp) {      // the patch lies wholly inside the domain
                float xh = 0.0f, xv = 0.0f;
                for (int u = 0; u < p; ++u)
                    for (int v = 0; v < p - 2; ++v) xh += gh[(pr + u) * LWP + pc + v];
                for (int u = 0; u < p - 2; ++u)
                    for (int v = 0; v < p; ++v) xv += gv[(pr + u) * LWP + pc + v];
                const float xtr = xh + xv;
                if (keep_all || xtr < tau) {
                    w = 1.0f;
                    ++my_count;
                }
            }
            wk[k] = w;
        }
        __syncthreads();

        // Gram of this tile's kept patches: one fp32 MFMA chain per output tile, K = patches (2 per instruction)
        // in chains of `chain` patches (launch-uniform; the whole slice for the whole-image domain), each added to fp64
        const int chain = s.chain > 0 ? s.chain : SLICE;
        for (int k0 = 0; k0 < SLICE; k0 += chain) {
            f32x16 acc[MAXT];
#pragma unroll
            for (int t = 0; t < MAXT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            for (int k2 = k0; k2 < k0 + chain; k2 += 2) {
                const int k = kbase + k2 + (lane >> 5);
                const int base = (k / TC) * LWP + k % TC;
                const float w = wk[k];
#pragma unroll
                for (int t = 0; t < MAXT; ++t) {
                    if (!tv[t]) continue;                  // wave-uniform
                    const float A = fmaf(scA[t], img[base + offA[t]], adA[t]) * w;
                    const float B = fmaf(scB[t], img[base + offB[t]], adB[t]) * w;
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A, B, acc[t], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < MAXT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc64[t][r] += (double)acc[t][r];
        }
    }

    atomicAdd(&s_count, my_count);                         // integer: order-free
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = lane & 31;
    double *out = part + (size_t)blockIdx.x * NT * 1024;
    __syncthreads();                                       // tile buffers are free from here
    if (NB == 2) {
        // four waves hold the same three tiles over different patches: sum them in LDS in wave order
        double *red = reinterpret_cast<double *>(lds);
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
#pragma unroll
                for (int t = 0; t < MAXT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                        double &d = red[t * 1024 + row * 32 + col];
                        d = w == 0 ? acc64[t][r] : d + acc64[t][r];
                    }
            }
            __syncthreads();
        }
        for (int e = tid; e < NT * 1024; e += NTHREADS) out[e] = red[e];
    } else {
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            if (!tv[t]) continue;
            const int ti = tile_index(tI[t], tJ[t]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                out[ti * 1024 + row * 32 + col] = acc64[t][r];
            }
        }
    }
    if (tid == 0) {
        shift[blockIdx.x] = (double)m;
        count[blockIdx.x] = (long long)s_count;
    }
}

// element (a, b), a >= b, of partial g's shifted D
__device__ __forceinline__ double d_at(const double *part, int NT, int g, int a, int b)
{
    return part[((size_t)g * NT + tile_index(a >> 5, b >> 5)) * 1024 + (a & 31) * 32 + (b & 31)];
}

// stage 1: block (x, chunk, domain) rebuilds G_g = D + m (s_a + s_b) + n m^2 for lower entries e of its range and
// partials g of its chunk of the domain's G, summed in g order; grid z strides over the nd domains
__global__ __launch_bounds__(256) void k_pca_reduce1(const double *__restrict__ part, const double *__restrict__ shift,
                                                     double *__restrict__ stage, int NT, int P2, int E, int G,
                                                     long long nd)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    const int b = e - a * (a + 1) / 2;
    const int g0 = blockIdx.y * RED_CHUNK, g1 = min(g0 + RED_CHUNK, G);
    for (long long d = blockIdx.z; d < nd; d += gridDim.z) {
        const double *dpart = part + (size_t)d * G * NT * 1024;
        const double *dshift = shift + (size_t)d * G;
        double acc = 0.0;
        for (int g = g0; g < g1; ++g) {
            const double m = dshift[g];
            const double n = d_at(dpart, NT, g, P2, P2);
            const double sa = d_at(dpart, NT, g, P2, a), sb = d_at(dpart, NT, g, P2, b);
            acc += d_at(dpart, NT, g, a, b) + m * (sa + sb) + n * m * m;
        }
        stage[((size_t)d * gridDim.y + blockIdx.y) * E + e] = acc;
    }
}

// stage 2: per domain (grid z strides over them) sum the chunks in order, write both triangles of gram[d]; one
// thread adds the domain's counts in order
__global__ __launch_bounds__(256) void k_pca_reduce2(const double *__restrict__ stage,
                                                     const long long *__restrict__ count, double *__restrict__ gram,
                                                     long long *__restrict__ total, int P2, int E, int G, int nchunks,
                                                     long long nd)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    const int b = e - a * (a + 1) / 2;
    for (long long d = blockIdx.z; d < nd; d += gridDim.z) {
        if (e == 0) {
            long long c = 0;
            for (int g = 0; g < G; ++g) c += count[(size_t)d * G + g];
            total[d] = c;
        }
        if (e >= E) continue;
        double acc = 0.0;
        for (int k = 0; k < nchunks; ++k) acc += stage[((size_t)d * nchunks + k) * E + e];
        double *out = gram + (size_t)d * P2 * P2;
        out[a * P2 + b] = acc;
        out[b * P2 + a] = acc;
    }
}

// Patches per fp32 chain in a cell (divides both slices).  A cell has one or two thousand patches, not an image's tens
// of thousands, and its smallest eigenvalue (~sigma^2 per patch) sits 100 x below the Gram's entries: with one chain
// per tile the rounding of the fp32 accumulation (~eps sqrt(steps) of the running sum) moved it by 1e-4 relative;
// chains of 8 patches (4 MFMA steps) hold it to 2e-6 for 27 % more time in this kernel.
constexpr int CELL_CHAIN = 8;
constexpr int GRID_Z_MAX = 65535;                         // grid dimension z of the reduction kernels

// The whole image as one domain (window <= 0) or a grid of window x window cells, `step` apart, per sample.
bool make_shape(int N, int C, int H, int W, int channel, int patchsize, int window, int step, Shape &s)
{
    if (N <= 0 || C <= 0 || channel < 0 || channel >= C) return false;
    if (patchsize < P_MIN || patchsize > P_MAX || H < patchsize || W < patchsize) return false;
    s.N = N; s.C = C; s.H = H; s.W = W; s.c = channel; s.p = patchsize; s.P2 = patchsize * patchsize;
    if (window <= 0) {
        s.wh = H; s.ww = W; s.step = 1; s.ny = s.nx = 1; s.dn = N; s.nd = 1; s.chain = 0;
    } else {
        if (window < patchsize || step < 1) return false;
        s.wh = H < window ? H : window;
        s.ww = W < window ? W : window;
        s.step = step;
        s.ny = H <= window ? 1 : (H - window + step - 1) / step + 1;
        s.nx = W <= window ? 1 : (W - window + step - 1) / step + 1;
        s.dn = 1;
        s.chain = CELL_CHAIN;
        s.nd = (long long)N * s.ny * s.nx;
    }
    s.Hp = s.wh - patchsize + 1;
    s.Wp = s.ww - patchsize + 1;
    s.tr = (s.Hp + TR - 1) / TR;
    s.tc = (s.Wp + TC - 1) / TC;
    s.ntiles = (long long)s.dn * s.tr * s.tc;
    s.gpd = 0;                                             // plan_of sets it
    return true;
}

struct Plan {
    int NB, NT, G, nchunks, E;                     // G: workgroups (partials) per domain
    size_t part_d, shift_d, stage_d, count_d;      // sizes in doubles / int64
};

// Workgroups per domain: the persistent grid shared among the domains, at least one each and no more than a
// domain has tiles.  One domain: min(tiles, grid), the whole-image launch.
bool plan_of(Shape &s, Plan &q)
{
    q.NB = s.P2 < 64 ? 2 : 4;                      // row P2 carries the constant 1, so P2 < PP
    q.NT = tiles_of(q.NB);
    const long long gmax = q.NB == 2 ? GRID_PP64 : GRID_PP128;
    long long gpd = (gmax + s.nd - 1) / s.nd;
    if (gpd > s.ntiles) gpd = s.ntiles;
    if (s.nd * gpd > 0x7fffffffLL) return false;   // grid dimension x
    q.G = s.gpd = (int)gpd;
    q.nchunks = (q.G + RED_CHUNK - 1) / RED_CHUNK;
    q.E = s.P2 * (s.P2 + 1) / 2;
    q.part_d = (size_t)s.nd * q.G * q.NT * 1024;
    q.shift_d = (size_t)s.nd * q.G;
    q.stage_d = (size_t)s.nd * q.nchunks * q.E;
    q.count_d = (size_t)s.nd * q.G;
    return true;
}

size_t plan_floats(const Plan &q) { return 2 * (q.part_d + q.shift_d + q.stage_d + q.count_d) + 64; }

// The one launcher of both entry points: per domain d, gram[d] and count[d] from taus[d] (or tau1 where taus is null).
int launch_gram(const float *y, const Shape &s, const Plan &q, const float *taus, float tau1, double *gram,
                long long *count, float *scratch, void *stream)
{
    // 8-byte aligned carve-up of the float scratch
    double *part = reinterpret_cast<double *>(((uintptr_t)scratch + 255) & ~(uintptr_t)255);
    double *shift = part + q.part_d;
    double *stage = shift + q.shift_d;
    long long *cnt = reinterpret_cast<long long *>(stage + q.stage_d);
    const unsigned grid = (unsigned)(s.nd * q.G);
    const unsigned gz = (unsigned)(s.nd < GRID_Z_MAX ? s.nd : GRID_Z_MAX);
    CDL_TRACE_NOTE("k_pca_gram<%d>", q.NB == 2 ? 2 : 4);
    if (q.NB == 2)
        k_pca_gram<2><<<grid, NTHREADS, 0, S(stream)>>>(y, s, taus, tau1, part, shift, cnt);
    else
        k_pca_gram<4><<<grid, NTHREADS, 0, S(stream)>>>(y, s, taus, tau1, part, shift, cnt);
    CDL_LAUNCH_CHECK();
    k_pca_reduce1<<<dim3((q.E + 255) / 256, q.nchunks, gz), 256, 0, S(stream)>>>(part, shift, stage, q.NT, s.P2, q.E, q.G, s.nd);
    CDL_LAUNCH_CHECK();
    k_pca_reduce2<<<dim3((q.E + 255) / 256, 1, gz), 256, 0, S(stream)>>>(stage, cnt, gram, count, s.P2, q.E, q.G, q.nchunks, s.nd);
    CDL_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t cdl_nle_pca_scratch_floats(int N, int C, int H, int W, int patchsize)
{
    Shape s;
    Plan q;
    if (!make_shape(N, C, H, W, 0, patchsize, 0, 0, s) || !plan_of(s, q)) return 0;
    return plan_floats(q);
}

int cdl_nle_pca_gram(const float *y, int N, int C, int H, int W, int channel, int patchsize, float tau,
                     double *gram, long long *count, float *scratch, size_t scratch_floats, void *stream)
{
    Shape s;
    Plan q;
    if (!y || !gram || !count || !scratch) return CDL_EINVAL;
    if (!make_shape(N, C, H, W, channel, patchsize, 0, 0, s) || !plan_of(s, q)) return CDL_EINVAL;
    if (scratch_floats < plan_floats(q)) return CDL_EINVAL;
    return launch_gram(y, s, q, nullptr, tau, gram, count, scratch, stream);
}

size_t cdl_nle_pca_gram_cells_scratch_floats(int N, int C, int H, int W, int patchsize, int window, int step)
{
    Shape s;
    Plan q;
    if (window < patchsize || !make_shape(N, C, H, W, 0, patchsize, window, step, s) || !plan_of(s, q)) return 0;
    return plan_floats(q);
}

int cdl_nle_pca_gram_cells(const float *y, int N, int C, int H, int W, int channel, int patchsize, int window,
                           int step, const float *tau, double *gram, long long *count, float *scratch,
                           size_t scratch_floats, void *stream)
{
    Shape s;
    Plan q;
    if (!y || !tau || !gram || !count || !scratch) return CDL_EINVAL;
    if (patchsize < P_MIN || patchsize > P_MAX || window < patchsize || step < 1) return CDL_EINVAL;
    if (!make_shape(N, C, H, W, channel, patchsize, window, step, s) || !plan_of(s, q)) return CDL_EINVAL;
    if (scratch_floats < plan_floats(q)) return CDL_EINVAL;
    return launch_gram(y, s, q, tau, 0.0f, gram, count, scratch, stream);
}

}  // extern "C"
