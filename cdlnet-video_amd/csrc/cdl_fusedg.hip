// Fused ISTA iteration on the matrix cores for the shapes the 2-D flagship kernel (cdl_fused2d.hip) does not take:
// any number of image channels C, 2-D or 3-D (depth taps Pd), unit stride, square filter planes P in {3, 5, 7},
// M <= 64 -- BASELINE configs[2] (CDLNetVideo K=20 M=48 P=5x5x5) and configs[3] (JDD: C=3, M=64, P=7, Bayer mask).
// Reference: the loop bodies model/net.py:87 and :205,  z = ST(z - A_k(mask * B_k z - yp), tau_k).
//
// Same fusion boundary as cdl_fused2d.hip: the launch is cut where the tensor is THIN (C channels), never where it
// is fat (M channels):
//
//     launch k :  r_k (thin) , z_k (fat)  ->  z_{k+1} (fat) , partial B_{k+1} z_{k+1} (thin patches)
//
// so every fat tensor crosses HBM exactly once in and once out per iteration, with no halo; the (P-1)-wide halo in
// y, x and depth lives on the thin residual.  Per 32-pixel row block of a wave:
//
//   analysis   acc[ch][px]   = sum_k W_A[ch][k] * im2col(r)[k][px]     k = (c, kd, ki, kj): C*Pd*P*P taps, padded to 16;
//                                                                      im2col gathered from bf16 hi/lo planes in LDS
//                                                                      through a tap -> offset table
//   epilogue   z'            = ST(z -/+ acc, tau) -> global            (reverse mode: du = [z' != 0] (du' + acc), dtau)
//   synthesis  col_g[tap][px] = sum_ch W_B^T[g][tap][ch] * z'[ch][px]  per group g = (c, kd); z' fed straight from the
//                                                                      accumulator registers (no LDS)
//   col2im     column direction by a Horner chain of DPP wave shifts (taps of a filter row are packed so that they sit
//              in known registers / lane halves), row direction in a P-row register ring per group
//
// A wave writes its (RB + P - 1) x (32 + P - 1) partial patch per group into its PRIVATE LDS patch (no cross-wave
// hazard inside the row loop); at the end of a tile the 8 wave patches are summed in a fixed order into the tile's
// patch, which goes to global memory; k_assemble_g sums the overlapping tile patches and depth taps in a fixed order and
// applies alpha, mask and -yp.  Everything is order-fixed: results are bit-reproducible, no atomics.
//
// fp32-grade accuracy on the bf16 matrix cores by the hi/lo split of cdl_fused2d.hip (3 MFMAs per product).
// Arithmetic intensity: 93 (cfg3) / 132 (cfg4) MFMA instructions per 32 voxels against 12-16 KB of fat traffic: this
// kernel needs ~50 % matrix-core utilisation to be HBM-bound (the 2-D flagship kernel: 16 %).
#include <atomic>
#include <type_traits>
#include <vector>

#include "cdl_common.h"
#include "cdl_fused_sweep.h"
#include "cdl_strip.h"

namespace {

#include "cdl_wave_dev.h"

constexpr int WX = 2, WY = 4, NW = WX * WY, NT = 64 * NW;   // 8 waves: 2 (x) x 4 (y)
constexpr int RB = 4;                                      // image rows per wave
constexpr int TW = 32 * WX, TH = RB * WY;                  // 64 x 16 pixel tile of one (n, depth) plane
// groups g = (c, kd) are a template parameter (their col2im rings live in registers): G = C * Pd in {1, 3, 5, 7}

struct GParams {
    const float *r;          // (N,C,D,H,W) thin input of the analysis-like half
    const float *zin;        // (N,M,D,H,W) or nullptr
    unsigned *map;           // (N,4,D,H,W) support / sign bit planes (forward: written when given; reverse: read)
    float *zout;             // (N,M,D,H,W)
    const float *tau;        // forward: (N,M); (N*D,M), a row per (sample, depth) plane, with tau_planes
    float *dtau;             // reverse: (tiles, M) partial sums of -sign(z') * du
    const uint4 *frags;      // prepared weights (k_prep_g)
    float *patches;          // (tiles, G, PY, PX)
    float sgn;
    int do_synth;
    int N, C, M, D, H, W, Pd, tilesX, tilesY, KS, rev;
    int tau_planes;          // CDL_TAU_PER_PLANE: the tile's thresholds are row n * D + zd of tau, not row n
    unsigned long long *tl;  // profiling hook (cdl_fusedg_set_timeline): s_memtime stamps of workgroup 0, [wave][256]
    CDL_DBG_FIELD(int dbg;)  // probe build only (CDL_FUSED_DEBUG; results are wrong): 1 no thin staging after the
                             // first tile, 2 no analysis GEMM, 4 no synthesis / col2im, 8 no fat loads, 16 no fat stores,
                             // 32 no patch combine
};

// ---- weight preparation ------------------------------------------------------------------------------------------
// fragment list of one (analysis bank wA, synthesis bank wB) pair, 16-byte lane entries:
//   [A hi | A lo] : (R, ks)            lane (row ch = 32R + (lane&31), h): taps k = 16ks + 8h + e of wA[ch] in its own
//                                       memory order k = ((c*Pd + kd)*P + ki)*P + kj (zero beyond M or K)
//   [B hi | B lo] : (g, Rt, q = 2R + s) lane (row t = 32Rt + (lane&31), h), element e: channel
//                                       32R + 16s + 8(e>>2) + 4h + (e&3) of wB[.][c][kd][tap of slot t] -- the k order
//                                       in which an accumulator tile presents itself as the next MFMA's B operand
template <int P>
__device__ __forceinline__ void prep_one(const float *__restrict__ wA, const float *__restrict__ wB,
                                         uint4 *__restrict__ out, int M, int C, int Pd, int MT, int KS, int KQ, int t)
{
    constexpr int RT = TapTiles<P>::RT;
    const int G = C * Pd, K = G * P * P;
    const int FA = MT * KS, FB = G * RT * KQ;
    if (t >= (FA + FB) * 64) return;
    const int lane = t & 63, f = t >> 6;
    const int row = lane & 31, h = lane >> 5;
    float v[8];
    if (f < FA) {
        const int R = f / KS, ks = f % KS;
        const int ch = 32 * R + row;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 16 * ks + 8 * h + e;
            v[e] = (ch < M && k < K) ? wA[(size_t)ch * K + k] : 0.0f;
        }
    } else {
        int q = f - FA;
        const int kq = q % KQ; q /= KQ;
        const int Rt = q % RT, g = q / RT;
        const int slot = 32 * Rt + row;
        int tap = -1;                                       // (i, j) whose slot this is
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j)
                if (tap_slot<P>(i, j) == slot) tap = i * P + j;
        const int R = kq >> 1, s = kq & 1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ch = 32 * R + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3);
            v[e] = (tap >= 0 && ch < M) ? wB[((size_t)ch * G + g) * (P * P) + tap] : 0.0f;
        }
    }
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 hh = (__bf16)v[e];
        hi[e] = hh;
        lo[e] = (__bf16)(v[e] - (float)hh);
    }
    uint4 *hd, *ld;
    if (f < FA) { hd = out + (size_t)f * 64; ld = out + (size_t)(FA + f) * 64; }
    else { hd = out + (size_t)(2 * FA + (f - FA)) * 64; ld = out + (size_t)(2 * FA + FB + (f - FA)) * 64; }
    hd[lane] = __builtin_bit_cast(uint4, hi);
    ld[lane] = __builtin_bit_cast(uint4, lo);
}

constexpr int PREP_BATCH = 32;
struct PrepBatch {
    const float *wA[PREP_BATCH];
    const float *wB[PREP_BATCH];
};
template <int P>
__global__ void k_prep_g(PrepBatch b, uint4 *__restrict__ out, int frag_uint4, int M, int C, int Pd, int MT, int KS, int KQ)
{
    prep_one<P>(b.wA[blockIdx.y], b.wB[blockIdx.y], out + (size_t)blockIdx.y * frag_uint4, M, C, Pd, MT, KS, KQ,
                blockIdx.x * blockDim.x + threadIdx.x);
}

// ---- the stage kernel --------------------------------------------------------------------------------------------
// LDS carve (bytes), see lds_bytes(): [A frags][B frags][koff][thin hi][thin lo][wave patches][tau][tacc]
struct Carve {
    int wa, wb, koff, xh, xl, wp, tau, tacc, total;
};
template <int P>
__host__ __device__ inline Carve carve(int MT, int KS, int KQ, int G, int prec)
{
    constexpr int RT = TapTiles<P>::RT;
    constexpr int XH = TH + P - 1, XW = TW + P - 1, PS = ((XH * XW + 7) / 8) * 8;
    constexpr int WPE = (RB + P - 1) * (32 + P - 1);
    Carve c;
    const int hl = prec == 0 ? 2 : 1;
    c.wa = 0;
    c.wb = c.wa + MT * KS * hl * 1024;
    c.koff = c.wb + G * RT * KQ * hl * 1024;
    c.xh = c.koff + KS * 16 * 4;
    c.xl = c.xh + G * PS * 2;
    c.wp = c.xl + (prec == 0 ? G * PS * 2 : 0);
    c.wp = (c.wp + 15) & ~15;
    c.tau = c.wp + NW * G * WPE * 4;
    c.tacc = c.tau + 64 * 4;
    c.total = c.tacc + NW * 64 * 4;
    return c;
}

// FOUR: split-bf16 x4 -- the lo * lo products as well (exact fp32 products); precision 2 of the entry points.
template <int P, int G, int MT, int MODE, bool FOUR = false>
__global__ __launch_bounds__(NT) void k_stage_g(GParams p)
{
    constexpr int PREC = 0;                                  // split-bf16 x3 (a plain-bf16 variant is not built)
    constexpr int RT = TapTiles<P>::RT;
    constexpr int HALO = P / 2;
    constexpr int XH = TH + P - 1, XW = TW + P - 1, PS = ((XH * XW + 7) / 8) * 8;
    constexpr int WPW = 32 + P - 1, WPH = RB + P - 1, WPE = WPH * WPW;      // wave patch
    constexpr int PY = TH + P - 1, PX = TW + P - 1;                          // tile patch
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int KS = (G * P * P + 15) / 16;               // 16-tap k-steps of the analysis-like GEMM (== p.KS)
    const int M = p.M;
    const int KQ = (M + 15) / 16;                            // 16-channel k-steps of the synthesis-like GEMM
    const Carve cv = carve<P>(MT, KS, KQ, G, PREC);
    const uint4 *wa = reinterpret_cast<const uint4 *>(smem + cv.wa);
    const uint4 *wb = reinterpret_cast<const uint4 *>(smem + cv.wb);
    int *koff = reinterpret_cast<int *>(smem + cv.koff);
    __bf16 *xh = reinterpret_cast<__bf16 *>(smem + cv.xh);
    __bf16 *xl = reinterpret_cast<__bf16 *>(smem + cv.xl);
    float *wp_all = reinterpret_cast<float *>(smem + cv.wp);
    float *tau_s = reinterpret_cast<float *>(smem + cv.tau);
    float *tacc_s = reinterpret_cast<float *>(smem + cv.tacc);

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wxi = wid % WX, wyi = wid / WX;
    const int c = lane & 31, h = lane >> 5;
    const size_t HW = (size_t)p.H * p.W, DHW = (size_t)p.D * HW;
    const int K = G * P * P;
    int tli = 0;
    const bool tl_on = p.tl != nullptr && blockIdx.x == 0;      // uniform
#define CDL_TL() do { if (tl_on) { if (lane == 0 && tli < 256) p.tl[wid * 256 + tli] = __builtin_readcyclecounter(); ++tli; } } while (0)
    CDL_TL();
    const int FA = MT * KS, FB = G * RT * KQ;
    const int numTiles = p.N * p.D * p.tilesY * p.tilesX;

    // ---- once per workgroup: weight fragments and the tap -> LDS offset table
    {
        uint4 *wdst = reinterpret_cast<uint4 *>(smem);
        if (PREC == 0) {
            // (A and B fragments are contiguous in the prepared list and in LDS: one copy, 4 loads in flight per thread --
            //  one load -> store at a time took 13k cycles per workgroup, 4 % of a cfg3 launch)
            const int nfr = 2 * (FA + FB) * 64;
            for (int i = tid; i < nfr; i += 4 * NT) {
                uint4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = p.frags[min(i + u * NT, nfr - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i + u * NT < nfr) wdst[i + u * NT] = v[u];
            }
        } else {                                             // plain bf16: hi parts only
            for (int i = tid; i < FA * 64; i += NT) wdst[i] = p.frags[i];
            uint4 *bdst = reinterpret_cast<uint4 *>(smem + cv.wb);
            for (int i = tid; i < FB * 64; i += NT) bdst[i] = p.frags[2 * FA * 64 + i];
        }
        for (int k = tid; k < KS * 16; k += NT) {
            int o = 0;
            if (k < K) {
                const int kj = k % P;
                const int q = k / P;
                o = (q / P) * PS + (q % P) * XW + kj;       // plane (c*Pd + kd), row ki, column kj
            }
            koff[k] = cv.xh + 2 * o;                        // BYTE address of the tap in the hi planes (lo: + cv.xl - cv.xh)
        }
    }
    const int OFF_AL = FA, OFF_BL = FB;                      // lo fragments follow the hi ones (split3 only)
    auto afrag = [&](int f) { return __builtin_bit_cast(bf16x8, wa[f * 64 + lane]); };
    auto bfrag = [&](int f) { return __builtin_bit_cast(bf16x8, wb[f * 64 + lane]); };
    float *wp = wp_all + (size_t)wid * G * WPE;
    // this thread's elements of a thin plane and of a tile patch row group: (row, column) computed once, so the
    // per-tile loops below run without integer divisions
    constexpr int NSTG = (XH * XW + NT - 1) / NT;
    int stg_row[NSTG], stg_col[NSTG];
#pragma unroll
    for (int k = 0; k < NSTG; ++k) {
        const int i = tid + k * NT;
        stg_row[k] = i < XH * XW ? i / XW : -1000000;       // rows far outside: the bounds test below drops them
        stg_col[k] = i % XW;
    }
    constexpr int CROWS = NT / PX;                           // patch rows handled per pass of the combine
    const int cmb_row = tid / PX, cmb_col = tid % PX;
    const int up_addr = ((lane & 31) + 32) * 4;              // ds_bpermute byte address of the lane 32 above
    const int lo_delta = cv.xl - cv.xh;                      // hi plane -> lo plane, bytes
    const bool has_base = (MODE == MODE_FWD) || (MODE == MODE_BWD && p.zin != nullptr);
    const int dhw4 = (int)DHW * 4;

    // thin planes of a tile: plane g = (c, kd) is depth zd - Pd/2 + kd of channel c.  Loaded into registers one tile
    // ahead (after the row loop of the previous tile, so the loads fly during its patch combine), converted and
    // stored to LDS at the top of the tile.
    // The loads are branch-free (clamped addresses); whether an element is inside the image (per thread, stg_ok) and
    // whether a plane exists (uniform, stg_planes) is applied when the values are converted, one tile later.
    float stg[G][NSTG];
    bool stg_ok[NSTG];
    unsigned stg_planes = 0;
    auto stage_load = [&](int t) {
        const bool skip = t >= numTiles || (CDL_DBG(p.dbg, 1) && t != (int)blockIdx.x);
        int bid = p.rev ? numTiles - 1 - t : t;
        bid = skip ? 0 : bid;
        const int txi = bid % p.tilesX; bid /= p.tilesX;
        const int tyi = bid % p.tilesY; bid /= p.tilesY;
        const int zd = bid % p.D, n = bid / p.D;
        int off[NSTG];
#pragma unroll
        for (int k = 0; k < NSTG; ++k) {
            const int yy = tyi * TH - HALO + stg_row[k], xx = txi * TW - HALO + stg_col[k];
            stg_ok[k] = yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
            off[k] = min(max(yy, 0), p.H - 1) * p.W + min(max(xx, 0), p.W - 1);
        }
        stg_planes = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int kd = g % p.Pd, cc = g / p.Pd;
            const int d = zd - p.Pd / 2 + kd;
            const bool dok = !skip && d >= 0 && d < p.D;     // uniform
            stg_planes |= (dok ? 1u : 0u) << g;
            const float *plane = p.r + (((size_t)n * p.C + cc) * p.D + (dok ? d : 0)) * HW;
#pragma unroll
            for (int k = 0; k < NSTG; ++k) stg[g][k] = plane[off[k]];
        }
    };
    auto stage_store = [&]() {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < NSTG; ++k) {
                const int i = tid + k * NT;
                const float v = (stg_ok[k] && ((stg_planes >> g) & 1u)) ? stg[g][k] : 0.0f;
                const __bf16 hh = (__bf16)v;
                if (i < XH * XW) {
                    xh[g * PS + i] = hh;
                    if (PREC == 0) xl[g * PS + i] = (__bf16)(v - (float)hh);
                }
            }
    };
    stage_load(blockIdx.x);

#pragma unroll 1
    for (int t = blockIdx.x; t < numTiles; t += gridDim.x) {
        int bid = p.rev ? numTiles - 1 - t : t;
        const int tile = bid;
        const int txi = bid % p.tilesX; bid /= p.tilesX;
        const int tyi = bid % p.tilesY; bid /= p.tilesY;
        const int zd = bid % p.D, n = bid / p.D;
        const int tx0 = txi * TW, ty0 = tyi * TH;
        CDL_TL();
        __syncthreads();                                     // previous tile's readers are done (and the tables are in)
        CDL_TL();
        stage_store();                                       // thin planes of this tile (loaded into registers earlier)
        if (MODE != MODE_BWD && tid < 64) {
            const int trow = p.tau_planes ? n * p.D + zd : n;   // every code element of a tile shares one frame
            tau_s[tid] = tid < M ? p.tau[(size_t)trow * M + tid] : 0.0f;
        }
        // (the wave's private patch needs no zeroing: the row loop stores rows 0 .. RB-1, the ring flush rows RB .. WPH-1,
        //  every column)
        CDL_TL();
        __syncthreads();
        CDL_TL();
        // thresholds are >= 0 whenever project() runs (net.py:70); a negative one (3-D trainer, never projected)
        // sends the whole tile through the general shrinkage -- wave-uniform, so the common case pays 3 instructions
        // per element instead of 10
        const bool tau_neg = MODE != MODE_BWD && __ballot(!(tau_s[lane] >= 0.0f)) != 0ull;   // negative OR NaN: the general, NaN-preserving form

        float ring[G][P];                                    // row-direction col2im sums, per group
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < P; ++i) ring[g][i] = 0.0f;
        float tsum[MT * 16];                                 // reverse: per-lane partial threshold gradients
#pragma unroll
        for (int i = 0; i < MT * 16; ++i) tsum[i] = 0.0f;

        const int x = tx0 + wxi * 32 + c;
        const bool xok = x < p.W;
        const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(
            has_base ? const_cast<float *>(p.zin) + (size_t)n * M * DHW : p.zout, 0, has_base ? (int)(M * DHW * 4) : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(
            p.zout + (size_t)n * M * DHW, 0, (int)(M * DHW * 4), 0x00020000);
        unsigned *const map_n = p.map ? p.map + (((size_t)n * 4 + 2 * h) * p.D + zd) * HW : nullptr;
        // per-lane part of a fat address: channel half 4h and pixel column (tile invariant); the row and the channel
        // travel in the scalar offset, built per row block by a running scalar sum (32 precomputed channel offsets
        // held across the row loop cost 100+ spilled SGPRs in the first version)
        const int voff_x = xok ? (int)((4 * h) * DHW + x) * 4 : OOB;

#pragma unroll 1
        for (int b = 0; b < RB; ++b) {
            const int yl = wyi * RB + b, y = ty0 + yl;
            const bool rowok = y < p.H;                          // uniform
            const bool valid = xok && rowok;
            const int voff = rowok ? voff_x : OOB;
            const int voff_st = CDL_DBG(p.dbg, 16) ? OOB : voff;
            // (y depends on the wave index: wave-uniform, but only readfirstlane makes that provable -- otherwise every
            //  buffer access below gets a waterfall loop around its scalar offset)
            const int s_row = __builtin_amdgcn_readfirstlane((int)((size_t)zd * HW + (size_t)y * p.W) * 4);
            // (M is a multiple of 8: a register quad of 4 channels x 2 lane halves is either all real or all padding,
            //  so padding channels are skipped by uniform branches and never reach an address)

            // -- fat inputs of this block, issued first
            float zc[MT][16];
            if (MODE != MODE_FIRST && CDL_DBG(p.dbg, 8)) {
#pragma unroll
                for (int R = 0; R < MT; ++R)
#pragma unroll
                    for (int v = 0; v < 16; ++v) zc[R][v] = 0.25f;
            } else if (MODE != MODE_FIRST) {
                int so = s_row;
#pragma unroll
                for (int R = 0; R < MT; ++R)
#pragma unroll
                    for (int qv = 0; qv < 4; ++qv) {
                        if (32 * R + 8 * qv < M) {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                zc[R][4 * qv + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                    rs_in, voff, so + e * dhw4, 0));
                        }
                        so += 8 * dhw4;
                    }
            }
            unsigned sup = 0, sgb = 0;
            if (MODE == MODE_BWD && valid) {
                sup = map_n[(size_t)y * p.W + x];
                sgb = map_n[DHW + (size_t)y * p.W + x];
            }

            // -- analysis-like GEMM: im2col gathered through the offset table
            const int pixbase = 2 * (yl * XW + wxi * 32 + c);   // bytes
            f32x16 acc[MT];
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[R][v] = 0.0f;
            // Software pipeline, depth 2, everything static (KS is a compile-time constant): the im2col operand and the
            // weight fragments of k-step ks+1 are read from LDS into the OTHER register set while the matrix pipe works on
            // k-step ks, and the products alternate between the accumulator tiles.  (Rolled, with one register set, every
            // k-step was  table read -> wait -> 16 gathers -> wait -> fragments -> wait -> 3 dependent MFMAs -> ...:
            // 940 cycles per k-step for 192 cycles of matrix work, tools/timeline_fusedg.py.)
            auto gather_b = [&](int ks, bf16x8 &bh, bf16x8 &bl) {
                const int4 o0 = *reinterpret_cast<const int4 *>(koff + 16 * ks + 8 * h);
                const int4 o1 = *reinterpret_cast<const int4 *>(koff + 16 * ks + 8 * h + 4);
                const int oo[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
                // one address add per tap; the lo plane is the same address + a constant that fits the DS offset field
                // (ds_read_u16_d16 / _d16_hi would save the v_perm_b32 per pair, but with SRAM ECC -- gfx950 -- a d16 load
                //  zeroes the other half of the register instead of keeping it: tried through inline asm, wrong results)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned char *pt = smem + (oo[i] + pixbase);
                    bh[i] = *reinterpret_cast<const __bf16 *>(pt);
                    bl[i] = *reinterpret_cast<const __bf16 *>(pt + lo_delta);
                }
            };

            {
                // (the im2col operand is double-buffered; the weight fragments only where the groups' col2im rings leave
                //  the registers: G * P <= 21)
                constexpr int FS = G * P <= 21 ? 2 : 1;
                bf16x8 bh[2], bl[2], ah[FS][MT], al[FS][MT];
                gather_b(0, bh[0], bl[0]);
                if (FS == 2) {
#pragma unroll
                    for (int R = 0; R < MT; ++R) {
                        ah[0][R] = afrag(R * KS);
                        al[0][R] = afrag(OFF_AL + R * KS);
                    }
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int cu = ks & 1, nx = cu ^ 1, fc = FS == 2 ? cu : 0, fn = FS == 2 ? nx : 0;
                    if (FS == 1) {
#pragma unroll
                        for (int R = 0; R < MT; ++R) {
                            ah[0][R] = afrag(R * KS + ks);
                            al[0][R] = afrag(OFF_AL + R * KS + ks);
                        }
                    }
                    if (ks + 1 < KS) {
                        gather_b(ks + 1, bh[nx], bl[nx]);
                        if (FS == 2) {
#pragma unroll
                            for (int R = 0; R < MT; ++R) {
                                ah[fn][R] = afrag(R * KS + ks + 1);
                                al[fn][R] = afrag(OFF_AL + R * KS + ks + 1);
                            }
                        }
                    }
#pragma unroll
                    for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[fc][R], bh[cu], acc[R], 0, 0, 0);
#pragma unroll
                    for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[fc][R], bl[cu], acc[R], 0, 0, 0);
                    if (FOUR) {
#pragma unroll
                        for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[fc][R], bl[cu], acc[R], 0, 0, 0);
                    }
#pragma unroll
                    for (int R = 0; R < MT; ++R) acc[R] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[fc][R], bh[cu], acc[R], 0, 0, 0);
                }
            }

            __builtin_amdgcn_sched_barrier(0);
            CDL_TL();
            // -- epilogue: register v of tile R is channel 32R + 8(v>>2) + 4h + (v&3) of pixel column c
            auto epilogue = [&](auto general_shrink) {
            int so = s_row;
#pragma unroll
            for (int R = 0; R < MT; ++R)
#pragma unroll
                for (int qv = 0; qv < 4; ++qv, so += 8 * dhw4) {
                    if (32 * R + 8 * qv >= M) {              // uniform: both channel quads of this register quad are padding
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[R][4 * qv + e] = 0.0f;
                        continue;
                    }
                    float t4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (MODE != MODE_BWD) {
                        const float4 tt = *reinterpret_cast<const float4 *>(&tau_s[32 * R + 8 * qv + 4 * h]);
                        t4[0] = tt.x; t4[1] = tt.y; t4[2] = tt.z; t4[3] = tt.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int v = 4 * qv + e;
                        float zz;
                        if (MODE == MODE_BWD) {
                            const bool on = (sup >> (16 * R + v)) & 1u;   // never set for out-of-image lanes / padding channels
                            zz = on ? zc[R][v] + acc[R][v] : 0.0f;
                            tsum[16 * R + v] += ((sgb >> (16 * R + v)) & 1u) ? zz : -zz;      // -sign(z') * du
                        } else {
                            const float base = (MODE == MODE_FWD) ? zc[R][v] : 0.0f;
                            const float u = fmaf(p.sgn, acc[R][v], base);
                            // t >= 0: sign(u) relu(|u| - t) == u - clamp(u, -t, t), same rounding, NaN in u stays NaN
                            zz = decltype(general_shrink)::value ? cdl_shrink(u, t4[e])
                                                                 : u - __builtin_amdgcn_fmed3f(u, -t4[e], t4[e]);
                            zz = valid ? zz : 0.0f;
                        }
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, zz), rs_out, voff_st, so + e * dhw4, 0);
                        acc[R][v] = zz;
                    }
                }
            };
            if (tau_neg) epilogue(std::true_type{});         // wave-uniform
            else epilogue(std::false_type{});
            if (MODE != MODE_BWD && map_n) {                 // uniform: training forward only
                unsigned ws = 0, wg = 0;
#pragma unroll
                for (int R = 0; R < MT; ++R)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const float zz = acc[R][v];
                        ws |= (zz != 0.0f ? 1u : 0u) << (16 * R + v);
                        wg |= (__builtin_bit_cast(unsigned, zz) >> 31) << (16 * R + v);
                    }
                if (valid) {
                    map_n[(size_t)y * p.W + x] = ws;
                    map_n[DHW + (size_t)y * p.W + x] = wg;
                }
            }
            if (MODE == MODE_BWD && !p.do_synth) continue;
            if CDL_DBG(p.dbg, 4) { ring[0][0] += acc[0][0] + acc[MT - 1][15]; continue; }

            __builtin_amdgcn_sched_barrier(0);
            CDL_TL();
            // -- synthesis-like GEMM: the accumulator tiles are the B operand (k = channel) as they stand; split once,
            //    reused by every group
            bf16x8 zh[2 * MT], zl[2 * MT];
#pragma unroll
            for (int q = 0; q < 2 * MT; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float val = acc[q >> 1][8 * (q & 1) + e];
                    const __bf16 hh = (__bf16)val;
                    zh[q][e] = hh;
                    if (PREC == 0) zl[q][e] = (__bf16)(val - (float)hh);
                }
            // One 32-row tap tile at a time (P = 7: filter rows 0-3 live in tile 0, rows 4-6 in tile 1).  col2im, column
            // direction: for filter row i, sum over j of tap (i, j) shifted right by j lanes; lane L (0 .. 32+P-2) ends with
            // the contribution to output column x0 - HALO + L.  The rows of a tile run as independent Horner chains side by
            // side (no DPP wait states to pad); taps that sit in the upper lane half are fetched with one cross-lane read
            // each.  Row direction: tap row i of image row y lands on output row y - HALO + i = ring slot i.
            // The tap tiles t = g * RT + Rt form a depth-2 pipeline: the products of tile t+1 are issued (into the other
            // accumulator) before the col2im of tile t, so the matrix pipe works under the DPP chains; the number of
            // 16-channel k-steps is a compile-time constant inside (two instantiations under one uniform branch).
            auto synth = [&](auto nq_c) {
                constexpr int NQ = decltype(nq_c)::value;
                constexpr int NTT = G * RT;
                auto mm = [&](int t) {
                    f32x16 Dt = f32x16{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        const int f = t * NQ + q;
                        const bf16x8 wh = bfrag(f), wl = bfrag(OFF_BL + f);
                        if (FOUR) Dt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, zl[q], Dt, 0, 0, 0);
                        Dt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, zh[q], Dt, 0, 0, 0);
                        Dt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, zl[q], Dt, 0, 0, 0);
                        Dt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, zh[q], Dt, 0, 0, 0);
                    }
                    return Dt;
                };
                auto c2i = [&](int t, const f32x16 &Dt) {
                    const int g = t / RT, Rt = t % RT;
                    float sr[P];
#pragma unroll
                    for (int i = 0; i < P; ++i) sr[i] = 0.0f;
#pragma unroll
                    for (int j = P - 1; j >= 0; --j)
#pragma unroll
                        for (int i = 0; i < P; ++i) {
                            const int slot = tap_slot<P>(i, j);
                            if ((slot >> 5) != Rt) continue;     // compile time: this row's taps are in the other tile
                            const int v = 4 * ((slot >> 3) & 3) + (slot & 3), hh = (slot >> 2) & 1;
                            float val = Dt[v];
                            if (hh)                              // lanes 0..31 read lanes 32..63
                                val = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(up_addr, __builtin_bit_cast(int, val)));
                            sr[i] = wave_shr1(sr[i]) + (h == 0 ? val : 0.0f);
                        }
#pragma unroll
                    for (int i = 0; i < P; ++i)
                        if ((tap_slot<P>(i, 0) >> 5) == Rt) ring[g][i] += sr[i];
                    if (Rt == RT - 1) {
                        // ring slot 0 is complete: one plain LDS store per lane into the wave's own patch
                        if (lane < WPW) wp[g * WPE + b * WPW + lane] = ring[g][0];
#pragma unroll
                        for (int i = 0; i + 1 < P; ++i) ring[g][i] = ring[g][i + 1];
                        ring[g][P - 1] = 0.0f;
                    }
                };
                // (the reverse mode of the 5-group shapes keeps 32 threshold-gradient registers besides the rings: the
                //  second accumulator tile spills there and costs more than it hides -- cfg3 fwd+bwd 10.2 vs 10.7 ms)
                constexpr bool SPIPE = !(MODE == MODE_BWD && G * P > 21);
                f32x16 D[2];
                D[0] = mm(0);
#pragma unroll
                for (int t = 0; t < NTT; ++t) {
                    if (SPIPE) {
                        if (t + 1 < NTT) D[(t + 1) & 1] = mm(t + 1);
                        c2i(t, D[t & 1]);
                    } else {
                        c2i(t, D[0]);
                        if (t + 1 < NTT) D[0] = mm(t + 1);
                    }
                }
            };
            if (KQ == 2 * MT) synth(std::integral_constant<int, 2 * MT>{});      // uniform
            else synth(std::integral_constant<int, 2 * MT - 1>{});
            CDL_TL();
        }
        // ---- the P-1 output rows below the wave's last image row are still in the ring
        if (MODE != MODE_BWD || p.do_synth) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
#pragma unroll
                for (int i = 0; i + 1 < P; ++i)
                    if (lane < WPW) wp[g * WPE + (RB + i) * WPW + lane] = ring[g][i];
            }
        }
        if (MODE == MODE_BWD) {
            const float tacc = LaneTransposeSum<MT * 16>::run(tsum, c) ;
            float tot = tacc;
            if (MT == 1) tot += __shfl_xor(tot, 16, 64);     // lanes c and c^16 hold halves of the same index
            if (c < MT * 16) {
                const int R = c >> 4, v = c & 15;
                tacc_s[wid * 64 + 32 * R + 8 * (v >> 2) + 4 * h + (v & 3)] = tot;
            }
        }
        CDL_TL();
        stage_load(t + gridDim.x);                           // next tile's thin loads fly during the combine below
        CDL_TL();
        __syncthreads();                                     // every wave's patch (and tacc) is complete
        CDL_TL();
        if (MODE == MODE_BWD && tid < 64) {
            float sacc = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w) sacc += tacc_s[w * 64 + tid];
            if (tid < M) p.dtau[(size_t)tile * M + tid] = sacc;
        }
        if ((MODE != MODE_BWD || p.do_synth) && !CDL_DBG(p.dbg, 32)) {
            // tile patch = fixed-order sum (wave row, then wave column) of the wave patches covering each element;
            // CROWS patch rows per pass, one thread per element
            float *patch = p.patches + (size_t)tile * G * (PY * PX);
            // (the empty asm keeps everything derived from the thread's patch position INSIDE the tile loop: hoisted, the
            //  offsets live across the row loop and spill)
            int ccol = cmb_col, crow = cmb_row;
            asm volatile("" : "+v"(ccol), "+v"(crow));
            if (crow < CROWS) {
                // an element is covered by at most NCY = ceil(WPH / RB) wave rows x 2 wave columns.  A thread owns one
                // patch column and the rows Y = cmb_row + CROWS j; which wave rows cover Y does not depend on the group,
                // so the candidate offsets are worked out once per j and the G groups follow at constant offsets, their
                // reads issued side by side; terms are added in the same order as before (wave row, then wave column;
                // absent candidates skipped).
                const int wx_lo = ccol >= 32 ? 1 : 0, wx_hi = ccol < WPW ? 0 : 1;      // waves (x) covering this column
                const bool two_x = wx_hi < wx_lo;
                constexpr int NCY = (WPH + RB - 1) / RB;
                constexpr int NJ = (PY + CROWS - 1) / CROWS;
                const float *col_hi = wp_all + (size_t)wx_hi * G * WPE + (ccol - wx_hi * 32);
                const float *col_lo = wp_all + (size_t)wx_lo * G * WPE + (ccol - wx_lo * 32);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int Y = crow + CROWS * j;
                    const bool rowok = Y < PY;
                    const int Yc = min(Y, PY - 1);
                    const int wy1 = min(Yc / RB, WY - 1);                             // the last covering wave row
                    int off[NCY];
                    bool oky[NCY];
#pragma unroll
                    for (int a = 0; a < NCY; ++a) {                                   // ascending wave rows
                        const int wy = wy1 - (NCY - 1) + a, ry = Yc - wy * RB;
                        oky[a] = wy >= 0 && ry < WPH;
                        off[a] = max(wy, 0) * (WX * G * WPE) + min(ry, WPH - 1) * WPW;
                    }
                    float v[G][2 * NCY];
#pragma unroll
                    for (int g = 0; g < G; ++g)
#pragma unroll
                        for (int a = 0; a < NCY; ++a) {
                            v[g][2 * a] = col_hi[off[a] + g * WPE];
                            v[g][2 * a + 1] = col_lo[off[a] + g * WPE];
                        }
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        float sum = 0.0f;
#pragma unroll
                        for (int a = 0; a < NCY; ++a) {
                            if (oky[a]) sum += v[g][2 * a];
                            if (oky[a] && two_x) sum += v[g][2 * a + 1];
                        }
                        if (rowok) patch[(g * PY + Y) * PX + ccol] = sum;
                    }
                }
            }
        }
        CDL_TL();
    }
#undef CDL_TL
}

// out[n,c,d,Y,X] = (mask ? mask : 1) * alpha * (sum over depth taps kd and covering tiles of the patches) - (sub ? sub : 0)
template <int P>
__global__ __launch_bounds__(256) void k_assemble_g(const float *__restrict__ patches, const float *__restrict__ mask,
                                                    const float *__restrict__ sub, float alpha, float *__restrict__ out,
                                                    int N, int C, int D, int H, int W, int Pd, int tilesX, int tilesY, float *__restrict__ accum,
                                                    int acc_add)
{
    constexpr int HALO = P / 2, PY = TH + P - 1, PX = TW + P - 1;
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= W) return;
    int r = blockIdx.z;
    const int d = r % D; r /= D;
    const int c = r % C, n = r / C;
    const int G = C * Pd;
    const int ay = Y + HALO, ax = X + HALO;                  // position in the patch grid of tile 0
    const int ty_hi = min(tilesY - 1, ay / TH), ty_lo = max(0, (ay - PY + TH) / TH);
    const int tx_hi = min(tilesX - 1, ax / TW), tx_lo = max(0, (ax - PX + TW) / TW);
    float sum = 0.0f;
    for (int kd = 0; kd < Pd; ++kd) {
        const int zd = d + Pd / 2 - kd;                      // the code depth whose tap kd lands on d
        if (zd < 0 || zd >= D) continue;
        const int g = c * Pd + kd;
        for (int ty = ty_lo; ty <= ty_hi; ++ty)
            for (int tx = tx_lo; tx <= tx_hi; ++tx) {
                const size_t tile = (((size_t)n * D + zd) * tilesY + ty) * tilesX + tx;
                sum += patches[((tile * G + g) * PY + (ay - ty * TH)) * PX + (ax - tx * TW)];
            }
    }
    const size_t i = ((((size_t)n * C + c) * D + d) * H + Y) * W + X;
    if (accum) accum[i] = acc_add ? accum[i] + sum : sum;     // the unmasked, unscaled sum (data gradient)
    if (!out) return;
    float v = alpha * sum;
    if (mask) v *= mask[i];
    if (sub) v -= sub[i];
    out[i] = v;
}

// Batch form (W % 4 == 0): a thread owns 4 consecutive pixels (16-byte thin accesses); the covering tiles of a
// 4-pixel group differ only when the group straddles a tile border, so each pixel still sums its own patches in the
// same (kd, tile row, tile column) order as k_assemble_g: bit-identical.
template <int P>
__global__ __launch_bounds__(256) void k_assemble_g4(const float *__restrict__ patches, const float *__restrict__ mask,
                                                     const float *__restrict__ sub, float alpha, float *__restrict__ out,
                                                     int N, int C, int D, int H, int W, int Pd, int tilesX, int tilesY, float *__restrict__ accum,
                                                     int acc_add)
{
    constexpr int HALO = P / 2, PY = TH + P - 1, PX = TW + P - 1;
    const int X0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X0 >= W || Y >= H) return;
    int r = blockIdx.z;
    const int d = r % D; r /= D;
    const int c = r % C, n = r / C;
    const int G = C * Pd;
    const int ay = Y + HALO;
    const int ty_hi = min(tilesY - 1, ay / TH), ty_lo = max(0, (ay - PY + TH) / TH);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool has_lo[4];
    for (int kd = 0; kd < Pd; ++kd) {
        const int zd = d + Pd / 2 - kd;
        if (zd < 0 || zd >= D) continue;
        const int g = c * Pd + kd;
        const size_t plane = ((size_t)n * D + zd) * tilesY;
        // a pixel lies in at most 2 x 2 patches (P - 1 < TH); the row candidates are wave-uniform, the column ones
        // are loaded side by side (8 independent loads) and added in the scalar form's order
        for (int ty = ty_lo; ty <= ty_hi; ++ty) {
            const float *row = patches + ((((plane + ty) * tilesX) * G + g) * PY + (ay - ty * TH)) * PX;
            float lo[4], hi[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ax = X0 + e + HALO;
                const int tx_hi = min(tilesX - 1, ax / TW), tx_lo = max(0, (ax - PX + TW) / TW);
                hi[e] = row[(size_t)tx_hi * (G * PY * PX) + (ax - tx_hi * TW)];
                lo[e] = tx_lo < tx_hi ? row[(size_t)tx_lo * (G * PY * PX) + (ax - tx_lo * TW)] : 0.0f;
                has_lo[e] = tx_lo < tx_hi;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (has_lo[e]) acc[e] += lo[e];
                acc[e] += hi[e];
            }
        }
    }
    const size_t i = ((((size_t)n * C + c) * D + d) * H + Y) * W + X0;
    if (accum) {                                              // the unmasked, unscaled sum (data gradient)
        float4 a = make_float4(acc[0], acc[1], acc[2], acc[3]);
        if (acc_add) {
            const float4 o = *reinterpret_cast<const float4 *>(accum + i);
            a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
        }
        *reinterpret_cast<float4 *>(accum + i) = a;
    }
    if (!out) return;
    float4 v = make_float4(alpha * acc[0], alpha * acc[1], alpha * acc[2], alpha * acc[3]);
    if (mask) {
        const float4 m = *reinterpret_cast<const float4 *>(mask + i);
        v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
    }
    if (sub) {
        const float4 sv = *reinterpret_cast<const float4 *>(sub + i);
        v.x -= sv.x; v.y -= sv.y; v.z -= sv.z; v.w -= sv.w;
    }
    *reinterpret_cast<float4 *>(out + i) = v;
}

// dt0[m] = sum over tiles; dt1[m] = sum_n c[n] * (sum over the tiles of sample n): fixed-order tree (cdl_fused2d.hip)
__global__ __launch_bounds__(1024) void k_dtau_reduce_g(const float *__restrict__ partial, const float *__restrict__ c,
                                                        float *__restrict__ dt0, float *__restrict__ dt1, int N,
                                                        int per_img, int M)
{
    __shared__ float r0[256][4], r1[256][4];
    const int mi = threadIdx.x & 3, part = threadIdx.x >> 2;
    const int m = blockIdx.x * 4 + mi;
    float a0 = 0.0f, a1 = 0.0f;
    const int rows = N * per_img;
    if (m < M)
        for (int row = part; row < rows; row += 256) {
            const float v = partial[(size_t)row * M + m];
            a0 += v;
            if (c) a1 = fmaf(c[row / per_img], v, a1);
        }
    r0[part][mi] = a0;
    r1[part][mi] = a1;
    __syncthreads();
    for (int stride = 128; stride >= 1; stride >>= 1) {
        if (part < stride) { r0[part][mi] += r0[part + stride][mi]; r1[part][mi] += r1[part + stride][mi]; }
        __syncthreads();
    }
    if (part == 0 && m < M) { dt0[m] = r0[0][mi]; dt1[m] = r1[0][mi]; }
}


typedef cdl_fusedg_plan Plan;                               // cdl_strip.h: one plan for the three kernels

bool tile_plan_for(const cdl_geom *g, Plan *pl)
{
    if (!cdl_grouped_plan_base(g, pl)) return false;
    pl->kind = CDL_PLAN_TILE;
    pl->tilesX = (g->W + TW - 1) / TW;
    pl->tilesY = (g->H + TH - 1) / TH;
    pl->items = (size_t)g->N * g->D * pl->tilesX * pl->tilesY;
    pl->per_img = (int)(pl->items / g->N);
    pl->prows = TH + g->Ph - 1;
    pl->pxw = TW + g->Pw - 1;
    pl->patch_floats = pl->items * pl->G * pl->prows * pl->pxw;
    if (pl->items >= ((size_t)1 << 30)) return false;
    int lds = 0;
    if (g->Ph == 3) lds = carve<3>(pl->MT, pl->KS, pl->KQ, pl->G, 0).total;
    if (g->Ph == 5) lds = carve<5>(pl->MT, pl->KS, pl->KQ, pl->G, 0).total;
    if (g->Ph == 7) lds = carve<7>(pl->MT, pl->KS, pl->KQ, pl->G, 0).total;
    return lds <= 160 * 1024;
}

// The first plan that accepts the geometry: the tile kernel's -- cdl_stripg.hip's in its place with CDL_FUSEDG_STRIP=1,
// where that accepts too (measured at parity with the tile kernel forward and behind it in the reverse mode, DESIGN.md
// section 5.2d) --, else cdl_strip.hip's.
bool route_for(const cdl_geom *g, Plan *pl)
{
    if (tile_plan_for(g, pl)) {
        Plan sg;
        if (cdl_opts().fusedg_strip && cdl_stripg_plan_for(g, &sg)) *pl = sg;
        return true;
    }
    return cdl_strip_plan_for(g, pl);
}

template <int P, int G, int MT, int MODE, bool FOUR = false>
int launch_one(const GParams &p, const Plan &pl, hipStream_t st)
{
    const int lds = carve<P>(MT, pl.KS, pl.KQ, G, 0).total;
    if (int rc = cdl_ensure_dynamic_lds((const void *)k_stage_g<P, G, MT, MODE, FOUR>, lds)) return rc;
    const unsigned grid = cdl_persistent_grid(pl.items);
    k_stage_g<P, G, MT, MODE, FOUR><<<grid, NT, lds, st>>>(p);
    CDL_LAUNCH_CHECK();
    return 0;
}

template <int P, int G, int MT>
int launch_mode(const GParams &p, const Plan &pl, int mode, hipStream_t st)
{
    if (mode == MODE_FWD) return launch_one<P, G, MT, MODE_FWD>(p, pl, st);
    if (mode == MODE_FIRST) return launch_one<P, G, MT, MODE_FIRST>(p, pl, st);
    if (mode == MODE_BWD) return launch_one<P, G, MT, MODE_BWD>(p, pl, st);
    // + 3: split-bf16 x4
    if (mode == MODE_FWD + 3) return launch_one<P, G, MT, MODE_FWD, true>(p, pl, st);
    if (mode == MODE_FIRST + 3) return launch_one<P, G, MT, MODE_FIRST, true>(p, pl, st);
    return launch_one<P, G, MT, MODE_BWD, true>(p, pl, st);
}

template <int P, int G>
int launch_g(const GParams &p, const Plan &pl, int mode, hipStream_t st)
{
    return pl.MT == 2 ? launch_mode<P, G, 2>(p, pl, mode, st) : launch_mode<P, G, 1>(p, pl, mode, st);
}

template <int P>
int launch_p(const GParams &p, const Plan &pl, int mode, hipStream_t st)
{
    if (pl.G == 1) return launch_g<P, 1>(p, pl, mode, st);
    if (pl.G == 3) return launch_g<P, 3>(p, pl, mode, st);
    if (pl.G == 5) return launch_g<P, 5>(p, pl, mode, st);
    return launch_g<P, 7>(p, pl, mode, st);
}

std::atomic<unsigned long long *> g_timeline{nullptr};

// fragments of K (analysis-like, synthesis-like) pairs of the tile and the stripg kernel, pair k at frags + k * frag bytes
int prep_pairs(const cdl_geom *g, const Plan &pl, const float *const *w1, const float *const *w2, int K, int shift2,
               void *frags, hipStream_t st)
{
    if (!cdl_aligned16(frags)) return CDL_EUNSUPPORTED;      // the library-sized fragment buffer is written 16 bytes at a time (cdlnet_hip.h)
    const int threads = (int)(pl.frag_uint4 / 2);           // one thread per (fragment, lane); hi and lo together
    for (int k0 = 0; k0 < K; k0 += PREP_BATCH) {
        PrepBatch b;
        const int nb = cdl_pair_batch(&b, w1, w2, K, shift2, k0);
        dim3 grid((unsigned)((threads + 255) / 256), (unsigned)nb);
        uint4 *out = reinterpret_cast<uint4 *>(frags) + (size_t)k0 * pl.frag_uint4;
        CDL_TRACE_NOTE("k_prep_g<%d>", pl.P == 3 || pl.P == 5 ? pl.P : 7);
        if (pl.P == 3) k_prep_g<3><<<grid, 256, 0, st>>>(b, out, (int)pl.frag_uint4, g->M, g->C, g->Pd, pl.MT, pl.KS, pl.KQ);
        else if (pl.P == 5) k_prep_g<5><<<grid, 256, 0, st>>>(b, out, (int)pl.frag_uint4, g->M, g->C, g->Pd, pl.MT, pl.KS, pl.KQ);
        else k_prep_g<7><<<grid, 256, 0, st>>>(b, out, (int)pl.frag_uint4, g->M, g->C, g->Pd, pl.MT, pl.KS, pl.KQ);
        CDL_LAUNCH_CHECK();
    }
    return 0;
}

int prep(const cdl_geom *g, const Plan &pl, const float *const *w1, const float *const *w2, int K, int shift2, void *frags,
         hipStream_t st)
{
    return pl.kind == CDL_PLAN_STRIP ? cdl_strip_prep_pairs(g, pl, w1, w2, K, shift2, frags, st)
                                     : prep_pairs(g, pl, w1, w2, K, shift2, frags, st);
}

// One stage launch behind cdl_fusedg_iter_fwd (MODE_FWD, MODE_FIRST: z' = ST(zin + sgn * A r, tau); map nullable) and
// cdl_fusedg_stage_bwd (MODE_BWD: du = [map](zin + acc), dtau).  precision: the entry points' word -- arithmetic in
// bits 0-3 (tile kernel: 0 = split-bf16 x3, 2 = x4; strip kernels: 0), CDL_TILES_REVERSED, and for the strip kernels
// CDL_LAYOUT_IN / CDL_LAYOUT_OUT (CDL_LAY_NCHW or CDL_LAY_RSC) of zin / zout; CDL_TAU_PER_PLANE: tau is (N*D, M) (tile and
// stripg kernels; the reverse mode reads no threshold and ignores it).
int stage(const cdl_geom *g, const Plan &pl, int mode, const float *r, const float *zin, const float *tau,
          const void *frags, float sgn, float *zout, float *patches, unsigned *map, float *dtau, int do_synth,
          int precision, hipStream_t st)
{
    if (!r || !frags || !zout || zout == zin) return CDL_EINVAL;
    if (mode == MODE_BWD ? (!map || !dtau) : (!tau || !patches)) return CDL_EINVAL;
    if (!cdl_aligned16(frags, patches)) return CDL_EUNSUPPORTED;     // library-sized buffers: 16-byte accesses (cdlnet_hip.h)
    if (do_synth && !patches) return CDL_EINVAL;
    const int rev = (precision >> 4) & 1;
    const int planes = (precision & CDL_TAU_PER_PLANE) ? 1 : 0;
    if (planes && pl.kind == CDL_PLAN_STRIP) return CDL_EINVAL;      // k_strip (2-D, D == 1) has no per-plane form
    precision &= ~CDL_TAU_PER_PLANE;
    if (pl.kind != CDL_PLAN_TILE) {
        const int li = (precision >> 5) & 3, lo = (precision >> 7) & 3;
        if ((precision >> 9) != 0) return CDL_EINVAL;
        if ((li != CDL_LAY_NCHW && li != CDL_LAY_RSC) || (lo != CDL_LAY_NCHW && lo != CDL_LAY_RSC)) return CDL_EINVAL;
        if ((precision & 15) != 0) return CDL_EUNSUPPORTED;
        const int rsc_in = li == CDL_LAY_RSC, rsc_out = lo == CDL_LAY_RSC;
        if ((rsc_in && !cdl_aligned16(zin)) || (rsc_out && !cdl_aligned16(zout))) return CDL_EUNSUPPORTED;   // rsc codes: 16-byte accesses
        if (pl.kind == CDL_PLAN_STRIP)
            return cdl_strip_stage(g, pl, mode, r, zin, tau, frags, sgn, zout, patches, map, dtau, do_synth, rev, rsc_in, rsc_out, st);
        return cdl_stripg_stage(g, pl, mode, r, zin, tau, frags, sgn, zout, patches, map, dtau, do_synth, rev, rsc_in, rsc_out,
                                planes, st);
    }
    if ((precision >> 5) != 0) return CDL_EINVAL;
    if ((precision & 15) == 2) mode += 3;                    // split-bf16 x4
    else if ((precision & 15) != 0) return CDL_EUNSUPPORTED;  // otherwise split-bf16 x3
    GParams p = {};
    p.r = r; p.zin = zin; p.map = map; p.zout = zout; p.tau = tau; p.dtau = dtau;
    p.frags = reinterpret_cast<const uint4 *>(frags);
    p.patches = patches; p.sgn = sgn; p.do_synth = do_synth;
    p.tl = g_timeline.load();
    p.rev = rev;
    p.tau_planes = planes;
    CDL_DBG_FIELD(p.dbg = cdl_opts().fused_debug;)
    p.N = g->N; p.C = g->C; p.M = g->M; p.D = g->D; p.H = g->H; p.W = g->W; p.Pd = g->Pd;
    p.tilesX = pl.tilesX; p.tilesY = pl.tilesY; p.KS = pl.KS;
    if (pl.P == 3) return launch_p<3>(p, pl, mode, st);
    if (pl.P == 5) return launch_p<5>(p, pl, mode, st);
    return launch_p<7>(p, pl, mode, st);
}

// CDL_LAYOUT_IN(precision) of a whole sweep: the layout of the codes that stay inside it (z[0..K-2], the du buffers);
// CDL_LAY_RSC for the strip kernels only, and only where the caller's other kernels read it (rsc_ok)
bool sweep_layout(const Plan &pl, int precision, bool rsc_ok, int *lay)
{
    precision &= ~CDL_TAU_PER_PLANE;
    *lay = (precision >> 5) & 3;
    return (precision >> 7) == 0 && (*lay == CDL_LAY_NCHW || (pl.kind != CDL_PLAN_TILE && *lay == CDL_LAY_RSC && rsc_ok));
}

// The precision word of one stage launch of a sweep.  Arithmetic of the tile kernel: split-bf16 x3 unless the caller
// (precision 2) or CDL_FUSEDG_PREC=2 asks for all four products.  (Round 3 tested the round-2 hypothesis that the dropped
// lo * lo products are what shows as 2e-4 in cfg4's dB_k: with x4 in both sweeps the figure does not move --
// tools/debug_cfg4.py, DESIGN.md section 3 -- so x3 stays.)  reversed: the snake order of cdl_fused2d.hip's sweeps.
int sweep_flags(const Plan &pl, int precision, bool reversed, int lay_in, int lay_out)
{
    const int forced = cdl_opts().fusedg_bwd_prec;
    const int prec = (pl.kind == CDL_PLAN_TILE && (forced == 0 || forced == 2)) ? forced : (precision & 15);
    return prec | (reversed ? CDL_TILES_REVERSED : 0) | CDL_LAYOUT_IN(lay_in) | CDL_LAYOUT_OUT(lay_out) |
           (precision & CDL_TAU_PER_PLANE);
}

// The two reductions behind cdl_fusedg_dtau_reduce and its per-plane sibling: `samples` groups of `per` consecutive partial
// rows -- the N samples of per_img rows each, or (planes) the N * D planes of per_img / D rows each: the rows are in
// [n][zd][ty][tx] order, so either grouping sums the same rows in the same order, c[group] weighting dt1.
int dtau_reduce(const cdl_geom *g, const Plan &pl, const float *dtau_partial, const float *c, float *dt0, float *dt1,
                float *dtau_n, bool planes, void *stream)
{
    if (!dtau_partial || !dt0 || !dt1) return CDL_EINVAL;
    if (planes && pl.kind == CDL_PLAN_STRIP) return CDL_EINVAL;
    const int samples = planes ? g->N * g->D : g->N, per = planes ? pl.per_img / g->D : pl.per_img;
    k_dtau_reduce_g<<<(g->M + 3) / 4, 1024, 0, S(stream)>>>(dtau_partial, c, dt0, dt1, samples, per, g->M);
    CDL_LAUNCH_CHECK();
    if (!dtau_n) return 0;
    // partial rows: [n][tile][m], as k_dtau_reduce_g reads them
    return cdl_dtau_per_sample(dtau_partial, samples, g->M, per, (size_t)per * g->M, 1, g->M, dtau_n, stream);
}

}  // namespace

extern "C" {

/* Profiling hook: while buf != NULL every fused generic stage launch records s_memtime stamps of workgroup 0 into
 * buf[wave][256] (8 x 256 x 8 bytes of device memory); tools/timeline_fusedg.py names the stamps.  NULL switches it off. */
int cdl_fusedg_set_timeline(void *buf)
{
    g_timeline.store(static_cast<unsigned long long *>(buf));
    return 0;
}

/* Shapes outside the tile kernel's that the strip kernel takes (cdl_strip.hip: one image channel, stride 1 or 2, up to 192
 * subbands -- the shipped CDLNet-s2030 architecture) go through the same entry points.  The size queries: 0 when no
 * kernel takes the geometry. */
int cdl_fusedg_supported(const cdl_geom *g)
{
    Plan pl;
    return route_for(g, &pl) ? 1 : 0;
}

size_t cdl_fusedg_frag_bytes(const cdl_geom *g)
{
    Plan pl;
    return route_for(g, &pl) ? pl.frag_uint4 * 16 : 0;
}

size_t cdl_fusedg_patch_floats(const cdl_geom *g)
{
    Plan pl;
    return route_for(g, &pl) ? pl.patch_floats : 0;
}

size_t cdl_fusedg_tiles(const cdl_geom *g)
{
    Plan pl;
    return route_for(g, &pl) ? pl.items : 0;
}

size_t cdl_fusedg_map_words(const cdl_geom *g)
{
    Plan pl;
    return route_for(g, &pl) ? pl.map_words : 0;
}

/* The layout the sweeps should keep z[0..K-2] and the du buffers in: CDL_LAY_RSC for the strip kernels' shapes (training:
 * when the matrix-core filter-gradient kernel takes the geometry), CDL_LAY_NCHW otherwise; cdl_fusedg_code_floats: floats of one
 * code tensor in that layout. */
int cdl_fusedg_code_layout(const cdl_geom *g, int training)
{
    Plan pl;
    if (!route_for(g, &pl) || pl.kind == CDL_PLAN_TILE) return CDL_LAY_NCHW;
    // a forward-only sweep has no filter gradients to feed: the strip kernels' own layout always
    return (!training || cdl_mfma_wgrad_takes(g)) ? CDL_LAY_RSC : CDL_LAY_NCHW;
}

size_t cdl_fusedg_code_floats(const cdl_geom *g, int layout)
{
    Plan pl;
    if (layout == CDL_LAY_RSC) return route_for(g, &pl) ? pl.rsc_floats : 0;
    return (size_t)g->N * g->M * (g->D / g->sd) * (g->H / g->sh) * (g->W / g->sw);
}

int cdl_fusedg_prep(const cdl_geom *g, const float *wA, const float *wB, void *frags, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    if (!wA || !wB || !frags) return CDL_EINVAL;
    const float *a[1] = {wA}, *b[1] = {wB};
    return prep(g, pl, a, b, 1, 1, frags, S(stream));
}

int cdl_fusedg_iter_fwd(const cdl_geom *g, const float *r, const float *zin, const float *tau, const void *frags,
                        float sgn, float *zout, float *patches, unsigned *map_out, int precision, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    return stage(g, pl, zin ? MODE_FWD : MODE_FIRST, r, zin, tau, frags, sgn, zout, patches, map_out, nullptr, 1, precision,
                 S(stream));
}

int cdl_fusedg_stage_bwd(const cdl_geom *g, const float *thin, const float *base, const unsigned *map,
                         const void *frags, float *du_out, float *patches, float *dtau_partial, int do_synth,
                         int precision, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    return stage(g, pl, MODE_BWD, thin, base, nullptr, frags, 1.0f, du_out, patches, const_cast<unsigned *>(map),
                 dtau_partial, do_synth ? 1 : 0, precision, S(stream));
}

int cdl_fusedg_assemble(const cdl_geom *g, const float *patches, const float *mask, const float *sub, float alpha,
                        float *out, float *acc, int acc_add, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    if (!patches || (!out && !acc)) return CDL_EINVAL;
    if (pl.kind == CDL_PLAN_STRIP) return cdl_strip_assemble(g, pl, patches, mask, sub, alpha, out, acc, acc_add, S(stream));
    if (pl.kind == CDL_PLAN_STRIPG) return cdl_stripg_assemble(g, pl, patches, mask, sub, alpha, out, acc, acc_add, S(stream));
    if (cdl_assemble16(g->W, out, mask, sub, acc)) {
        dim3 grid((unsigned)((g->W + 255) / 256), (unsigned)((g->H + 3) / 4), (unsigned)(g->N * g->C * g->D));
#define CDL_ASM4(P_) k_assemble_g4<P_><<<grid, 256, 0, S(stream)>>>(patches, mask, sub, alpha, out, g->N, g->C, g->D, g->H, g->W, g->Pd, pl.tilesX, pl.tilesY, acc, acc_add)
        CDL_TRACE_NOTE("k_assemble_g4<%d>", pl.P == 3 || pl.P == 5 ? pl.P : 7);
        if (pl.P == 3) CDL_ASM4(3); else if (pl.P == 5) CDL_ASM4(5); else CDL_ASM4(7);
#undef CDL_ASM4
    } else {
        dim3 grid((unsigned)((g->W + 255) / 256), (unsigned)g->H, (unsigned)(g->N * g->C * g->D));
#define CDL_ASM(P_) k_assemble_g<P_><<<grid, 256, 0, S(stream)>>>(patches, mask, sub, alpha, out, g->N, g->C, g->D, g->H, g->W, g->Pd, pl.tilesX, pl.tilesY, acc, acc_add)
        CDL_TRACE_NOTE("k_assemble_g<%d>", pl.P == 3 || pl.P == 5 ? pl.P : 7);
        if (pl.P == 3) CDL_ASM(3); else if (pl.P == 5) CDL_ASM(5); else CDL_ASM(7);
#undef CDL_ASM
    }
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_fusedg_dtau_reduce(const cdl_geom *g, const float *dtau_partial, const float *c, float *dt0, float *dt1,
                           float *dtau_n, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    return dtau_reduce(g, pl, dtau_partial, c, dt0, dt1, dtau_n, false, stream);
}

int cdl_fusedg_dtau_reduce_planes(const cdl_geom *g, const float *dtau_partial, const float *c, float *dt0, float *dt1,
                                  float *dtau_nd, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    return dtau_reduce(g, pl, dtau_partial, c, dt0, dt1, dtau_nd, true, stream);
}

/* ---- whole sweeps (one C call each), the counterparts of cdl_fused2d_forward / _backward ------------------------ */
int cdl_fusedg_forward(const cdl_geom *g, int K, const float *yp, const float *mask, const float *tau,
                       const float *const *wA, const float *const *wB, float *const *z, float *const *r,
                       unsigned *const *maps, float *xp, void *frags, float *patches, int precision, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    if (K < 1 || !yp || !tau || !wA || !wB || !z || !xp || !frags || !patches || (K > 1 && !r)) return CDL_EINVAL;
    if ((precision & CDL_TAU_PER_PLANE) && pl.kind == CDL_PLAN_STRIP) return CDL_EINVAL;
    const size_t nm = (size_t)g->N * g->M * ((precision & CDL_TAU_PER_PLANE) ? g->D : 1);      // tau rows of one iteration
    int rc = prep(g, pl, wA, wB, K, 1, frags, S(stream));             // (A_k, B_{k+1}) for every k
    if (rc) return rc;
    int lay;                                                 // of z[0..K-2]; z[K-1] is always the reference's (N,M,..) layout
    if (!sweep_layout(pl, precision, true, &lay)) return CDL_EINVAL;
    return cdl_forward_order_sweep(
        K, frags, pl.frag_uint4 * 16, yp, mask, yp, 1.0f, r, xp, cdl_opts().fused_snake, lay, CDL_LAY_NCHW,
        [&](int k, const void *fk, const float *thin, bool reversed, int lay_in, int lay_out) {
            return stage(g, pl, k ? MODE_FWD : MODE_FIRST, thin, k ? z[k - 1] : nullptr, tau + k * nm, fk, k ? -1.0f : 1.0f,
                         z[k], patches, maps ? maps[k] : nullptr, nullptr, 1,
                         sweep_flags(pl, precision, reversed, lay_in, lay_out), S(stream));
        },
        [&](const float *m, const float *sub, float alpha, float *out) {
            return cdl_fusedg_assemble(g, patches, m, sub, alpha, out, nullptr, 0, stream);
        });
}

/* Forward-mode tangent sweep at the primal's supports: the reverse stage with the FORWARD's prepared
 * pairs (A_k, B_{k+1}), base = zd_k, thin = -rd_k and the primal's bit map of z_{k+1}; the assemble with alpha = -1 and
 * sub = -vp forms the next thin operand -rd_{k+1}.  Codes stay in the reference's (N,M,..) layout.  The threshold partials
 * of the stages (dtau_partial) are never reduced. */
int cdl_fusedg_tangent(const cdl_geom *g, int K, const float *vp, const float *nvp, const float *mask,
                       const float *const *wA, const float *const *wB, const unsigned *const *maps, float *const *zd,
                       float *const *nrd, float *xdp, void *frags, float *patches, float *dtau_partial, int precision,
                       void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    if (K < 1 || !vp || !nvp || !wA || !wB || !maps || !zd || !xdp || !frags || !patches || !dtau_partial || (K > 1 && !nrd))
        return CDL_EINVAL;
    if ((precision >> 5) != 0) return CDL_EINVAL;             // CDL_LAY_NCHW codes only
    int rc = prep(g, pl, wA, wB, K, 1, frags, S(stream));             // (A_k, B_{k+1}), the forward's pairs
    if (rc) return rc;
    return cdl_forward_order_sweep(
        K, frags, pl.frag_uint4 * 16, vp, mask, nvp, -1.0f, nrd, xdp, cdl_opts().fused_snake, CDL_LAY_NCHW, CDL_LAY_NCHW,
        [&](int k, const void *fk, const float *thin, bool reversed, int lay_in, int lay_out) {
            return stage(g, pl, MODE_BWD, thin, k ? zd[k - 1] : nullptr, nullptr, fk, 1.0f, zd[k], patches,
                         const_cast<unsigned *>(maps[k]), dtau_partial, 1, sweep_flags(pl, precision, reversed, lay_in, lay_out),
                         S(stream));
        },
        [&](const float *m, const float *sub, float alpha, float *out) {
            return cdl_fusedg_assemble(g, patches, m, sub, alpha, out, nullptr, 0, stream);
        });
}

/* Reverse sweep: the fused stage produces du_k (one fat write), the threshold partials and the patches of q_k; the
 * filter gradients dA_k = -du_k (x) r_k and dB_k = z_k (x) q_k come from the shape-generic cdl_wgrad (its matrix-core
 * kernel where the shape has one).  wgrad_ws: cdl_wgrad_workspace_floats(g) floats. */
int cdl_fusedg_backward(const cdl_geom *g, int K, const float *yp, const float *mask, const float *c,
                        const float *const *wA, const float *const *wB, const float *const *z, const float *const *r,
                        const unsigned *const *maps, const float *g_xp, const float *g_z, float *const *dA,
                        float *const *dB, float *dt, float *du0, float *du1, float *q, void *frags, float *patches,
                        float *dtau_partial, float *wgrad_ws, size_t wgrad_ws_floats, int precision, float *dyp,
                        float *dtau, void *stream)
{
    Plan pl;
    if (!route_for(g, &pl)) return CDL_EUNSUPPORTED;
    if (K < 1 || !yp || !wA || !wB || !z || !maps || !g_xp || !dA || !dB || !dt || !du0 || !du1 || !q || !frags ||
        !patches || !dtau_partial || (K > 1 && !r))
        return CDL_EINVAL;
    const bool planes = (precision & CDL_TAU_PER_PLANE) != 0;      // c (N*D), dtau (K, N*D, M)
    if (planes && pl.kind == CDL_PLAN_STRIP) return CDL_EINVAL;
    const int M = g->M;
    float *du[2] = {du0, du1};
    // the layout of z[0..K-2] and of the du buffers: CDL_LAY_RSC when the matrix-core filter-gradient kernel takes the
    // geometry (its VALU fallbacks read the reference layout only)
    int lay;
    if (!sweep_layout(pl, precision, cdl_mfma_wgrad_takes(g), &lay)) return CDL_EINVAL;
    const int rsc = lay == CDL_LAY_RSC;
    const int snake = cdl_opts().fused_snake;
    int rc = cdl_wgrad(g, z[K - 1], nullptr, g_xp, 1.0f, dB[0], wgrad_ws, wgrad_ws_floats, stream);      // dB_0 = z_K (x) dL/d(D z_K)
    if (rc) return rc;
    const float *thin = g_xp, *base = g_z;
    rc = prep(g, pl, wB, wA, K, 0, frags, S(stream));                 // (B_{k+1}, A_k) for every k
    if (rc) return rc;
    for (int k = K - 1, flip = 0; k >= 0; --k, flip ^= 1) {
        const void *fk = static_cast<const char *>(frags) + (size_t)k * pl.frag_uint4 * 16;
        float *duk = du[flip];
        // stage k walks the way the forward's stage k did; with the snake off the direction still alternates from the
        // first reverse stage on
        const bool reversed = snake ? (k & 1) : ((K - 1 - k) & 1);
        rc = stage(g, pl, MODE_BWD, thin, base, nullptr, fk, 1.0f, duk, patches, const_cast<unsigned *>(maps[k]), dtau_partial,
                   k >= 1 || dyp, sweep_flags(pl, precision, reversed, k == K - 1 ? CDL_LAY_NCHW : lay, lay), S(stream));
        if (rc) return rc;
        rc = dtau_reduce(g, pl, dtau_partial, c, dt + (size_t)k * 2 * M, dt + (size_t)k * 2 * M + M,
                         dtau ? dtau + (size_t)k * g->N * (planes ? g->D : 1) * M : nullptr, planes, stream);
        if (rc) return rc;
        if (k == 0 && dyp) {                                    // u_0 = A_0 yp: dyp += A_0^T du_0 (no q at k = 0)
            rc = cdl_fusedg_assemble(g, patches, nullptr, nullptr, 1.0f, nullptr, dyp, K > 1, stream);
            if (rc) return rc;
        }
        if (k >= 1) {
            // q_k = -mask A_k^T du_k; with dyp the same sum, unmasked, goes to dyp (= at k = K-1, += after)
            rc = cdl_fusedg_assemble(g, patches, mask, nullptr, -1.0f, q, dyp, k < K - 1, stream);
            if (rc) return rc;
            const cdl_wgrad_op ops[2] = {{duk, r[k - 1], -1.0f, dA[k]}, {z[k - 1], q, 1.0f, dB[k]}};
            rc = rsc ? cdl_mfma_wgrad(g, ops, 2, nullptr, 1, wgrad_ws, wgrad_ws_floats, stream)
                     : cdl_wgrad_pair(g, duk, r[k - 1], -1.0f, dA[k], z[k - 1], q, 1.0f, dB[k], wgrad_ws, wgrad_ws_floats, stream);
            thin = q;
        } else {
            const cdl_wgrad_op op{duk, yp, 1.0f, dA[0]};
            rc = rsc ? cdl_mfma_wgrad(g, &op, 1, nullptr, 1, wgrad_ws, wgrad_ws_floats, stream)
                     : cdl_wgrad(g, duk, nullptr, yp, 1.0f, dA[0], wgrad_ws, wgrad_ws_floats, stream);
        }
        if (rc) return rc;
        base = duk;
    }
    return 0;
}

}  // extern "C"
