// SSIM on the device (reference loss.py:39-56 through pytorch_msssim, analyzemri.py:257-291 through skimage): per-plane
// means of the SSIM and cs maps of a separable window, and their reverse sweep.
//
// A call covers P independent contiguous H x W fp32 planes.  The window is `taps` 1-D weights w (odd, 3..15), applied
// along both axes with "valid" filtering: position (p, q), 0 <= p < Ho = H - taps + 1, 0 <= q < Wo, sees the pixels
// (p + u, q + v), weight w[u] w[v].  With the five moments E[x], E[y], E[x^2], E[y^2], E[xy] of a position,
//     sx = kappa (E[x^2] - E[x]^2), sy, sxy likewise,   C1 = (K1 R)^2, C2 = (K2 R)^2   (R = data_range[plane]),
//     L = (2 mx my + C1) / (mx^2 + my^2 + C1),   cs = (2 sxy + C2) / (sx + sy + C2),   S = L cs.
//
// Centring.  The variance terms cancel: E[x^2] and E[x]^2 agree in their leading digits when the local variance is
// small against the mean (data_range 255 images, flat regions).  Every workgroup subtracts one pixel of x (and one
// of y) from its tile -- d = x - m_x, e = y - m_y -- and forms the moments of d and e: the covariances do not change,
// mx = E[d] + m_x.  The reverse sweep differentiates with respect to the moments of d and e (below), so the same
// centring serves both directions and needs no agreement between them.
//
// Forward (k_ssim_fwd): a workgroup owns TH x TW positions.  It stages the TH + taps - 1 rows and TW + taps - 1
// columns of centred x and y in LDS, runs the horizontal pass of the five moments into LDS, then the vertical pass
// in registers (each thread slides down four positions of one column), forms S and cs and reduces them in the
// workgroup in fp64.  k_ssim_reduce adds the per-tile partials of one plane in a fixed order.  No atomics anywhere:
// repeated calls are bit-identical.
//
// Reverse (k_ssim_bwd): a workgroup owns TH x TW PIXELS.  The positions that see them are the tile widened by
// taps - 1 up and left, and their moments need the pixels of the tile widened by taps - 1 on every side
// (2 (taps - 1) halo in all).  Per position, with the upstream gradient g of the plane's SSIM mean and n = Ho Wo:
//     dS/dmx = 2 cs (my - mx L) / B1,  dS/dsx = -S / B2,  dS/dsxy = 2 L / B2       (B1, B2 the denominators)
//     b = kappa dS/dsx,  c = kappa dS/dsxy,  a = dS/dmx - 2 E[d] b - E[e] c             (each times g / n)
// so that dL/dx = W^T a + 2 d (W^T b) + e (W^T c), W^T the adjoint ("full") window filter; dL/dy is the same with
// (ay, by) from the y side.  The workgroup forms a, b, c (and ay, by) in LDS, runs the horizontal then vertical
// adjoint pass and writes dx (dy).  dL/dR comes through C1 and C2: dS/dR = 2 R (K1^2 cs (1 - L) / B1 +
// K2^2 L (1 - cs) / B2), summed over the positions the workgroup owns (its own tile's) in fp64, per plane in order.
#include "cdl_common.h"

namespace {

constexpr int T_MIN = 3, T_MAX = 15;
constexpr int TH = 16, TW = 64;              // positions (forward) / pixels (reverse) per workgroup tile
constexpr int NTHREADS = 256;                // 4 waves: wave = a quarter of the tile's rows, lane = its column
constexpr int RPT = TH / (NTHREADS / TW);    // rows per thread in the vertical passes
static_assert(RPT == 4 && TW == 64, "one wave per four rows of 64 columns");
constexpr int RED_THREADS = 256;

struct Args {
    int P, H, W, T, Ho, Wo, th, tw;          // th x tw tiles per plane
    int cr, cc;                              // the tile's centre pixel, as an offset from its first (0, 0: the first itself)
    float K1, K2, kappa;
    float w[T_MAX];
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// fixed-order sum over the workgroup's four waves; every thread gets the result
__device__ __forceinline__ double block_sum(double v, double *red)
{
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

__device__ __forceinline__ void load_window(const Args &a, float *sw)
{
#pragma unroll
    for (int t = 0; t < T_MAX; ++t)          // compile-time indices into the argument block
        if ((int)threadIdx.x == t) sw[t] = a.w[t];
}

// moments of the centred pixels -> S, cs and the partial derivatives used by the reverse pass
struct Pos {
    float L, cs, B1, B2, mx, my;
};

__device__ __forceinline__ Pos ssim_at(const float m[5], float sx0, float sy0, float kappa, float C1, float C2)
{
    Pos o;
    o.mx = m[0] + sx0;
    o.my = m[1] + sy0;
    const float vx = kappa * (m[2] - m[0] * m[0]);
    const float vy = kappa * (m[3] - m[1] * m[1]);
    const float vxy = kappa * (m[4] - m[0] * m[1]);
    o.B1 = o.mx * o.mx + o.my * o.my + C1;
    o.B2 = vx + vy + C2;
    o.L = (2.0f * o.mx * o.my + C1) / o.B1;
    o.cs = (2.0f * vxy + C2) / o.B2;
    return o;
}

// Stage rows r0.., columns c0.. (IR x IC) of the centred x and y of plane `pl` in LDS (zero outside the image);
// the centres are the pixels at (min(ar, H-1), min(ac, W-1)).
__device__ __forceinline__ void stage_tile(const Args &a, const float *__restrict__ x, const float *__restrict__ y,
                                           size_t pl, int r0, int c0, int IR, int IC, int ar, int ac, float *sx,
                                           float *sy, float &x0, float &y0)
{
    const float *xp = x + pl * (size_t)a.H * a.W, *yp = y + pl * (size_t)a.H * a.W;
    const size_t ctr = (size_t)min(ar, a.H - 1) * a.W + min(ac, a.W - 1);
    x0 = xp[ctr];
    y0 = yp[ctr];
    for (int e = threadIdx.x; e < IR * IC; e += NTHREADS) {
        const int i = e / IC, j = e % IC;
        const int gi = r0 + i, gj = c0 + j;
        const bool in = gi >= 0 && gi < a.H && gj >= 0 && gj < a.W;
        const size_t o = in ? (size_t)gi * a.W + gj : 0;
        sx[e] = in ? xp[o] - x0 : 0.0f;
        sy[e] = in ? yp[o] - y0 : 0.0f;
    }
}

// horizontal pass of the five moments: h[m][i][j] = sum_t w[t] f_m(i, j + t), i < rows, j < cols (pitch cols)
__device__ __forceinline__ void moments_h(const float *sx, const float *sy, int IC, int rows, int cols, int T,
                                          const float *sw, float *h)
{
    const int plane = rows * cols;
    for (int e = threadIdx.x; e < plane; e += NTHREADS) {
        const int i = e / cols, j = e % cols;
        const float *px = sx + i * IC + j, *py = sy + i * IC + j;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
        for (int t = 0; t < T; ++t) {
            const float wt = sw[t], d = px[t], f = py[t];
            const float wd = wt * d, wf = wt * f;
            m0 += wd;
            m1 += wf;
            m2 = fmaf(wd, d, m2);
            m3 = fmaf(wf, f, m3);
            m4 = fmaf(wd, f, m4);
        }
        h[e] = m0;
        h[plane + e] = m1;
        h[2 * plane + e] = m2;
        h[3 * plane + e] = m3;
        h[4 * plane + e] = m4;
    }
}

// 2x2 average pooling of plane `pl` for the next MS-SSIM level (torch's avg_pool2d(kernel 2, padding [H % 2, W % 2]),
// count_include_pad): pooled pixel (i, j) covers the rows 2i - H % 2, +1 and the columns 2j - W % 2, +1; the pad row
// and column of an odd axis are raw zeros and the divisor stays 4.  Tile (tr, tc) of the forward grid writes the
// pooled pixels whose block's FIRST pixel lies in its TH x TW tile; the last tile along an axis takes everything up
// to the image edge and the first one the pad block, so every pooled pixel has exactly one writer.  The four pixels
// are read again from the image (the tile has just staged them: they sit in the cache), not rebuilt from the centred
// LDS copy: (x - m) + m does not round back to x.  Sum in torch's order, ((p00 + p01) + p10) + p11, then * 0.25.
__device__ __forceinline__ void pool_tile(const Args &a, const float *__restrict__ x, const float *__restrict__ y,
                                          size_t pl, int tr, int tc, float *__restrict__ px, float *__restrict__ py)
{
    const int ph = a.H & 1, pw = a.W & 1, Hn = (a.H + ph) >> 1, Wn = (a.W + pw) >> 1;
    const int lo_r = tr == 0 ? -1 : tr * TH, hi_r = tr == a.th - 1 ? a.H : (tr + 1) * TH;
    const int lo_c = tc == 0 ? -1 : tc * TW, hi_c = tc == a.tw - 1 ? a.W : (tc + 1) * TW;
    const int i0 = (lo_r + ph + 1) >> 1, i1 = min(Hn, (hi_r + ph + 1) >> 1);
    const int j0 = (lo_c + pw + 1) >> 1, j1 = min(Wn, (hi_c + pw + 1) >> 1);
    const int nj = j1 - j0, n = (i1 - i0) * nj;
    const float *xp = x + pl * (size_t)a.H * a.W, *yp = y + pl * (size_t)a.H * a.W;
    float *qx = px + pl * (size_t)Hn * Wn, *qy = py + pl * (size_t)Hn * Wn;
    for (int e = threadIdx.x; e < n; e += NTHREADS) {
        const int i = i0 + e / nj, j = j0 + e % nj;
        const int r = 2 * i - ph, c = 2 * j - pw;                 // r + 1 <= H - 1 and c + 1 <= W - 1 since i < Hn, j < Wn
        const size_t o = (size_t)max(r, 0) * a.W + max(c, 0);
        const bool top = r >= 0, left = c >= 0;
        const float x00 = top && left ? xp[o] : 0.0f, y00 = top && left ? yp[o] : 0.0f;
        const float x01 = top ? xp[(size_t)r * a.W + c + 1] : 0.0f, y01 = top ? yp[(size_t)r * a.W + c + 1] : 0.0f;
        const float x10 = left ? xp[(size_t)(r + 1) * a.W + c] : 0.0f, y10 = left ? yp[(size_t)(r + 1) * a.W + c] : 0.0f;
        const float x11 = xp[(size_t)(r + 1) * a.W + c + 1], y11 = yp[(size_t)(r + 1) * a.W + c + 1];
        qx[(size_t)i * Wn + j] = (((x00 + x01) + x10) + x11) * 0.25f;
        qy[(size_t)i * Wn + j] = (((y00 + y01) + y10) + y11) * 0.25f;
    }
}

// px, py (both or neither): the pooled planes of the next MS-SSIM level, written beside the sums (launch-uniform)
__global__ __launch_bounds__(NTHREADS) void k_ssim_fwd(const float *__restrict__ x, const float *__restrict__ y,
                                                       Args a, const float *__restrict__ range,
                                                       double *__restrict__ part, float *__restrict__ px,
                                                       float *__restrict__ py)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float sw[T_MAX];
    __shared__ double red[4];
    const int T = a.T;
    const int IR = TH + T - 1, IC = TW + T - 1;
    float *sx = reinterpret_cast<float *>(smem), *sy = sx + IR * IC, *h = sy + IR * IC;

    const int tiles = a.th * a.tw;
    const size_t pl = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int r0 = (tile / a.tw) * TH, c0 = (tile % a.tw) * TW;
    load_window(a, sw);
    float x0, y0;
    stage_tile(a, x, y, pl, r0, c0, IR, IC, r0 + a.cr, c0 + a.cc, sx, sy, x0, y0);
    if (px) pool_tile(a, x, y, pl, tile / a.tw, tile % a.tw, px, py);
    __syncthreads();
    moments_h(sx, sy, IC, IR, TW, T, sw, h);
    __syncthreads();

    // vertical pass: thread (lane = column, wave = four rows) slides down T + 3 rows of h
    const int col = threadIdx.x & 63, rb = (threadIdx.x >> 6) * RPT;
    const int hp = IR * TW;
    float acc[RPT][5];
#pragma unroll
    for (int o = 0; o < RPT; ++o)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[o][m] = 0.0f;
    for (int j = 0; j < T + RPT - 1; ++j) {
        const int e = (rb + j) * TW + col;
        float v[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) v[m] = h[m * hp + e];
#pragma unroll
        for (int o = 0; o < RPT; ++o) {
            const int t = j - o;
            if (t >= 0 && t < T) {
                const float wt = sw[t];
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[o][m] = fmaf(wt, v[m], acc[o][m]);
            }
        }
    }
    const float R = range[pl];
    const float C1 = (a.K1 * R) * (a.K1 * R), C2 = (a.K2 * R) * (a.K2 * R);
    float s_ssim = 0.0f, s_cs = 0.0f;
    const int q = c0 + col;
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const int p = r0 + rb + o;
        if (p < a.Ho && q < a.Wo) {
            const Pos z = ssim_at(acc[o], x0, y0, a.kappa, C1, C2);
            s_ssim += z.L * z.cs;
            s_cs += z.cs;
        }
    }
    const double t_ssim = block_sum((double)s_ssim, red);
    const double t_cs = block_sum((double)s_cs, red);
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = t_ssim;
        part[2 * (size_t)blockIdx.x + 1] = t_cs;
    }
}

// one workgroup per plane: out_v[pl] = scale * (sum over the plane's tiles of part[.][v]) / count, in a fixed order;
// scale = g[pl * gs] when g is given, else 1; out_v is written at [pl * os].  With g1 (the MS-SSIM reverse, nv = 2: the
// dS/dR and dcs/dR sums) the two values are scaled by g and g1 and ADDED into out0[pl], on top of what out0 holds when
// `accum` (the coarser levels' share; one thread per plane, launches of a stream in order).
__global__ __launch_bounds__(RED_THREADS) void k_ssim_reduce(const double *__restrict__ part, int tiles, int nv,
                                                             double count, const float *__restrict__ g,
                                                             const float *__restrict__ g1, int gs, float *out0,
                                                             float *__restrict__ out1, int os, int accum)
{
    __shared__ double red[RED_THREADS];
    const size_t pl = blockIdx.x;
    double both = 0.0;
    for (int v = 0; v < nv; ++v) {
        double s = 0.0;
        for (int t = threadIdx.x; t < tiles; t += RED_THREADS) s += part[(pl * tiles + t) * nv + v];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int k = RED_THREADS / 2; k > 0; k >>= 1) {
            if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const float *gv = v == 0 ? g : g1;
            const double r = red[0] / count * (gv ? (double)gv[pl * gs] : 1.0);
            float *out = v == 0 ? out0 : out1;
            if (g1)
                both += r;
            else if (out)
                out[pl * os] = (float)r;
        }
        __syncthreads();
    }
    if (g1 && threadIdx.x == 0) out0[pl] = (float)(accum ? both + (double)out0[pl] : both);
}

// the pixel's own dx / dy from the adjoint sums, the expressions of the plain form (the MS form adds the up-sampled term
// to their value)
__device__ __forceinline__ float own_x(const float G[5], float d, float f)
{
    return G[0] + 2.0f * d * G[1] + f * G[2];
}

__device__ __forceinline__ float own_y(const float G[5], float d, float f)
{
    return G[3] + 2.0f * f * G[4] + d * G[2];
}

// One tile of the reverse sweep.  MS = false is cdl_ssim_bwd's form, statement for statement what it has always run;
// MS = true adds the MS-SSIM forms (below, at k_ssim_bwd_form) as further statements on the same values.
template <bool MS>
__device__ __forceinline__ void bwd_tile(const float *__restrict__ x, const float *__restrict__ y, const Args &a,
                                         const float *__restrict__ range, const float *__restrict__ gsum,
                                         const float *__restrict__ gcs, int gs, float *__restrict__ dx,
                                         float *__restrict__ dy, double *__restrict__ part, int nc,
                                         const float *__restrict__ up_x, const float *__restrict__ up_y,
                                         unsigned char *smem, float *sw, double *red)
{
    const int T = a.T;
    const int IR = TH + 2 * (T - 1), IC = TW + 2 * (T - 1);       // pixels staged
    const int PR = TH + T - 1, PC = TW + T - 1;                   // positions whose windows meet the tile
    float *sx = reinterpret_cast<float *>(smem), *sy = sx + IR * IC;
    float *h = sy + IR * IC;                                      // 5 x IR x PC, later nc x PR x TW
    float *cf = h + 5 * IR * PC;                                  // nc x PR x PC

    const int tiles = a.th * a.tw;
    const size_t pl = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles;
    const int r0 = (tile / a.tw) * TH, c0 = (tile % a.tw) * TW;   // first pixel of the tile
    const int pr0 = r0 - (T - 1), pc0 = c0 - (T - 1);             // first position / staged pixel
    load_window(a, sw);
    float x0, y0;
    stage_tile(a, x, y, pl, pr0, pc0, IR, IC, r0 + a.cr, c0 + a.cc, sx, sy, x0, y0);
    __syncthreads();
    moments_h(sx, sy, IC, IR, PC, T, sw, h);
    __syncthreads();

    const float R = range[pl];
    const float C1 = (a.K1 * R) * (a.K1 * R), C2 = (a.K2 * R) * (a.K2 * R);
    const float scale = gsum[pl * gs] / ((float)a.Ho * (float)a.Wo);
    const float scale_c = MS ? gcs[pl * gs] / ((float)a.Ho * (float)a.Wo) : 0.0f;
    const float kappa = a.kappa;
    const int hp = IR * PC, cp = PR * PC;
    float s_dr = 0.0f, s_dc = 0.0f;
    for (int e = threadIdx.x; e < cp; e += NTHREADS) {
        const int i = e / PC, j = e % PC;
        const int p = pr0 + i, q = pc0 + j;
        float ca = 0.f, cb = 0.f, cc = 0.f, cay = 0.f, cby = 0.f;
        float ea = 0.f, eb = 0.f, ec = 0.f, eay = 0.f;            // the cs terms (MS)
        if (p >= 0 && q >= 0 && p < a.Ho && q < a.Wo) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int t = 0; t < T; ++t) {
                const float wt = sw[t];
                const int o = (i + t) * PC + j;
#pragma unroll
                for (int k = 0; k < 5; ++k) m[k] = fmaf(wt, h[k * hp + o], m[k]);
            }
            const Pos z = ssim_at(m, x0, y0, kappa, C1, C2);
            const float Sv = z.L * z.cs;
            const float d_sx = -Sv / z.B2;                        // = dS/dsy
            const float d_sxy = 2.0f * z.L / z.B2;
            const float d_mx = 2.0f * z.cs * (z.my - z.mx * z.L) / z.B1;
            const float d_my = 2.0f * z.cs * (z.mx - z.my * z.L) / z.B1;
            cb = kappa * d_sx;
            cc = kappa * d_sxy;
            ca = d_mx - 2.0f * m[0] * cb - m[1] * cc;
            cby = cb;
            cay = d_my - 2.0f * m[1] * cby - m[0] * cc;
            if (i >= T - 1 && j >= T - 1)                         // this tile's own positions
                s_dr += 2.0f * R * (a.K1 * a.K1 * z.cs * (1.0f - z.L) / z.B1 + a.K2 * a.K2 * z.L * (1.0f - z.cs) / z.B2);
            if constexpr (MS) {
                eb = kappa * (-z.cs / z.B2);
                ec = kappa * (2.0f / z.B2);
                ea = -2.0f * m[0] * eb - m[1] * ec;
                eay = -2.0f * m[1] * eb - m[0] * ec;
                if (i >= T - 1 && j >= T - 1) s_dc += 2.0f * R * (a.K2 * a.K2 * (1.0f - z.cs) / z.B2);
            }
        }
        if constexpr (MS) {
            cf[e] = ca * scale + ea * scale_c;
            cf[cp + e] = cb * scale + eb * scale_c;
            cf[2 * cp + e] = cc * scale + ec * scale_c;
            if (nc == 5) {
                cf[3 * cp + e] = cay * scale + eay * scale_c;
                cf[4 * cp + e] = cby * scale + eb * scale_c;
            }
        } else {
            cf[e] = ca * scale;
            cf[cp + e] = cb * scale;
            cf[2 * cp + e] = cc * scale;
            if (nc == 5) {
                cf[3 * cp + e] = cay * scale;
                cf[4 * cp + e] = cby * scale;
            }
        }
    }
    __syncthreads();                                              // h is free from here
    // horizontal adjoint: g[k][i][j] = sum_t w[t] cf[k][i][j + T - 1 - t], j < TW
    const int gp = PR * TW;
    for (int e = threadIdx.x; e < gp; e += NTHREADS) {
        const int i = e / TW, j = e % TW;
        for (int k = 0; k < nc; ++k) {
            const float *src = cf + k * cp + i * PC + j + T - 1;
            float s = 0.0f;
            for (int t = 0; t < T; ++t) s = fmaf(sw[t], src[-t], s);
            h[k * gp + e] = s;
        }
    }
    __syncthreads();
    // vertical adjoint and the pixel terms: thread (lane = column, wave = four rows)
    const int col = threadIdx.x & 63, rb = (threadIdx.x >> 6) * RPT;
    const int gj = c0 + col;
#pragma unroll
    for (int o = 0; o < RPT; ++o) {
        const int li = rb + o, gi = r0 + li;
        float G[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < T; ++t) {
            const float wt = sw[t];
            const int src = (li + T - 1 - t) * TW + col;
            for (int k = 0; k < nc; ++k) G[k] = fmaf(wt, h[k * gp + src], G[k]);
        }
        if (gi < a.H && gj < a.W) {
            const int si = (li + T - 1) * IC + col + T - 1;
            const float d = sx[si], f = sy[si];
            const size_t o_ = pl * (size_t)a.H * a.W + (size_t)gi * a.W + gj;
            if constexpr (MS) {
                const int ph = a.H & 1, pw = a.W & 1, Hn = (a.H + ph) >> 1, Wn = (a.W + pw) >> 1;
                const size_t u_ = pl * (size_t)Hn * Wn + (size_t)((gi + ph) >> 1) * Wn + ((gj + pw) >> 1);
                const float ux = up_x ? 0.25f * up_x[u_] : 0.0f, uy = up_y ? 0.25f * up_y[u_] : 0.0f;
                if (dx) dx[o_] = own_x(G, d, f) + ux;
                if (dy) dy[o_] = own_y(G, d, f) + uy;
            } else {
                if (dx) dx[o_] = G[0] + 2.0f * d * G[1] + f * G[2];
                if (dy) dy[o_] = G[3] + 2.0f * f * G[4] + d * G[2];
            }
        }
    }
    if (part) {
        const double t_dr = block_sum((double)s_dr, red);
        if constexpr (MS) {
            const double t_dc = block_sum((double)s_dc, red);
            if (threadIdx.x == 0) {
                part[2 * (size_t)blockIdx.x] = t_dr;
                part[2 * (size_t)blockIdx.x + 1] = t_dc;
            }
        } else {
            if (threadIdx.x == 0) part[blockIdx.x] = t_dr;
        }
    }
}

// The reverse kernel, in two compiled forms (launch_bwd picks one and launches it from its one launch line, where the
// chosen form goes by the name k_ssim_bwd): MS = false is cdl_ssim_bwd's kernel with its registers and occupancy,
// MS = true the MS-SSIM form.  nc = 3: dx only (a, b, c); nc = 5: also the y side (ay, by).  The upstream gradient of
// plane pl's SSIM mean is gsum[pl * gs].  The MS-SSIM form also takes
// * gcs[pl * gs], the upstream gradient of the plane's cs mean.  cs sees the moments only through sx, sy, sxy --
//   dcs/dsxy = 2 / B2, dcs/dsx = dcs/dsy = -cs / B2 -- so its terms add into b, c, by and, through the centring, into
//   a, ay; `part` then holds two sums per workgroup, dS/dR and dcs/dR = 2 R K2^2 (1 - cs) / B2;
// * up_x, up_y (nullable, with dx / dy): the next coarser level's gradients on the pooled grid; pixel (r, c) adds a
//   quarter of its pooled pixel ((r + H % 2) / 2, (c + W % 2) / 2) to its own result (avg_pool2d's adjoint).
template <bool MS>
__global__ __launch_bounds__(NTHREADS) void k_ssim_bwd_form(const float *__restrict__ x, const float *__restrict__ y,
                                                            Args a, const float *__restrict__ range,
                                                            const float *__restrict__ gsum,
                                                            const float *__restrict__ gcs, int gs,
                                                            float *__restrict__ dx, float *__restrict__ dy,
                                                            double *__restrict__ part, int nc,
                                                            const float *__restrict__ up_x,
                                                            const float *__restrict__ up_y)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float sw[T_MAX];
    __shared__ double red[4];
    bwd_tile<MS>(x, y, a, range, gsum, gcs, gs, dx, dy, part, nc, up_x, up_y, smem, sw, red);
}

bool make_args(int P, int H, int W, const float *win, int taps, float K1, float K2, float kappa, int th_, int tw_,
               bool pixels, Args &a)
{
    if (P <= 0 || !win || taps < T_MIN || taps > T_MAX || (taps & 1) == 0 || H < taps || W < taps) return false;
    a.P = P; a.H = H; a.W = W; a.T = taps;
    a.Ho = H - taps + 1;
    a.Wo = W - taps + 1;
    const int rows = pixels ? H : a.Ho, cols = pixels ? W : a.Wo;
    a.th = (rows + th_ - 1) / th_;
    a.tw = (cols + tw_ - 1) / tw_;
    a.K1 = K1; a.K2 = K2; a.kappa = kappa;
    a.cr = a.cc = 0;
    for (int t = 0; t < T_MAX; ++t) a.w[t] = t < taps ? win[t] : 0.0f;
    return true;
}

// The centring takes mx = E[d] + m_x and drops the derivative through the centre pixel; both are exact only for a
// window of unit sum, so the entry points refuse any other (1e-5: the rounding of a normalised fp32 window).
bool window_normalised(const float *win, int taps)
{
    double s = 0.0;
    for (int t = 0; t < taps; ++t) s += (double)win[t];
    return fabs(s - 1.0) <= 1e-5;
}

int fwd_lds_bytes(int T) { return (int)sizeof(float) * (2 * (TH + T - 1) * (TW + T - 1) + 5 * (TH + T - 1) * TW); }

int bwd_lds_bytes(int T, int nc)
{
    const int IR = TH + 2 * (T - 1), IC = TW + 2 * (T - 1), PR = TH + T - 1, PC = TW + T - 1;
    return (int)sizeof(float) * (2 * IR * IC + 5 * IR * PC + nc * PR * PC);
}

// partials (fp64) of the larger of the two passes, on a 256-byte boundary
size_t scratch_floats_of(int P, int H, int W, int taps)
{
    const float w1[T_MAX] = {};
    Args f, b;
    if (!make_args(P, H, W, w1, taps, 0.f, 0.f, 1.f, TH, TW, false, f)) return 0;
    make_args(P, H, W, w1, taps, 0.f, 0.f, 1.f, TH, TW, true, b);
    const size_t nf = 2 * (size_t)P * f.th * f.tw, nb = (size_t)P * b.th * b.tw;
    return 2 * (nf > nb ? nf : nb) + 64;
}

double *carve(float *scratch) { return reinterpret_cast<double *>(((uintptr_t)scratch + 255) & ~(uintptr_t)255); }

// ---- MS-SSIM: level i + 1 is the 2x2 average pooling of level i, an odd axis padded by one zero row / column in front
constexpr int LEVELS_MAX = 8;

struct Pyramid {
    int levels, H[LEVELS_MAX], W[LEVELS_MAX];
    size_t off[LEVELS_MAX + 1];              // of level i >= 1 in a pyramid buffer (levels 1.., back to back); off[levels]: its size
};

// false: levels outside 1..8, or a level that cannot hold the window
bool make_pyramid(int P, int H, int W, int taps, int levels, Pyramid &py)
{
    if (P <= 0 || levels < 1 || levels > LEVELS_MAX || taps < T_MIN || taps > T_MAX || (taps & 1) == 0) return false;
    py.levels = levels;
    py.off[0] = py.off[1] = 0;
    for (int i = 0; i < levels; ++i) {
        if (H < taps || W < taps) return false;
        py.H[i] = H;
        py.W[i] = W;
        if (i >= 1) py.off[i + 1] = py.off[i] + (size_t)P * H * W;
        H = (H + 1) >> 1;
        W = (W + 1) >> 1;
    }
    return true;
}

// The first row and column of a pooled plane are darkened by the zero pad of every odd axis on the way down (by 2 per
// level: 1/128 of a typical pixel at level 4 of 177 x 162), so the tile's first pixel is no centre there: E[d] would be
// the whole mean and the variances would cancel as if nothing had been subtracted.  Pooled levels centre on the middle
// pixel of the tile (clamped into the plane); level 0 keeps the first pixel, and with it cdl_ssim_*'s bits.
void centre_pooled(Args &a, int level)
{
    if (level > 0) {
        a.cr = TH / 2;
        a.cc = TW / 2;
    }
}

// level 0 has the most tiles; the reverse pass keeps two sums per workgroup (dS/dR and dcs/dR)
size_t ms_scratch_floats_of(int P, int H, int W, int taps, int levels)
{
    Pyramid py;
    if (!make_pyramid(P, H, W, taps, levels, py)) return 0;
    const float w1[T_MAX] = {};
    Args f, b;
    make_args(P, H, W, w1, taps, 0.f, 0.f, 1.f, TH, TW, false, f);
    make_args(P, H, W, w1, taps, 0.f, 0.f, 1.f, TH, TW, true, b);
    const size_t nf = 2 * (size_t)P * f.th * f.tw, nb = 2 * (size_t)P * b.th * b.tw;
    return 2 * (nf > nb ? nf : nb) + 64;
}

// ---- the launches, shared by the cdl_ssim_* and cdl_msssim_* entry points (arguments checked by the caller)
// means of S -> out0[pl * os], of cs -> out1[pl * os] (nullable); px, py: the next level's planes (both or neither)
int launch_fwd(const float *x, const float *y, const Args &a, const float *data_range, double *part, float *px,
               float *py, float *out0, float *out1, int os, int level, void *stream)
{
    const long long blocks = (long long)a.P * a.th * a.tw;
    if (blocks > 0x7fffffffLL) return CDL_EUNSUPPORTED;
    const int lds = fwd_lds_bytes(a.T);
    int rc = cdl_ensure_dynamic_lds((const void *)k_ssim_fwd, lds);
    if (rc) return rc;
    CDL_TRACE_NOTE("k_ssim_fwd level=%d pool=%d", level, px ? 1 : 0);
    k_ssim_fwd<<<(unsigned)blocks, NTHREADS, lds, S(stream)>>>(x, y, a, data_range, part, px, py);
    CDL_LAUNCH_CHECK();
    CDL_TRACE_NOTE("k_ssim_reduce level=%d", level);
    k_ssim_reduce<<<a.P, RED_THREADS, 0, S(stream)>>>(part, a.th * a.tw, 2, (double)a.Ho * a.Wo, nullptr, nullptr, 1,
                                                      out0, out1, os, 0);
    CDL_LAUNCH_CHECK();
    return 0;
}

// g_ssim[pl * gs] (and g_cs[pl * gs], nullable) -> dx, dy (each nullable; plus a quarter of up_x, up_y where given) and,
// when d_range is given, the plane's dL/dR (added to what d_range holds when `accum`)
int launch_bwd(const float *x, const float *y, const Args &a, const float *data_range, const float *g_ssim,
               const float *g_cs, int gs, float *dx, float *dy, float *d_range, int accum, const float *up_x,
               const float *up_y, float *scratch, int level, void *stream)
{
    const long long blocks = (long long)a.P * a.th * a.tw;
    if (blocks > 0x7fffffffLL) return CDL_EUNSUPPORTED;
    double *part = d_range ? carve(scratch) : nullptr;
    const int nc = dy ? 5 : 3;
    const int lds = bwd_lds_bytes(a.T, nc);
    auto *const k_ssim_bwd = g_cs ? k_ssim_bwd_form<true> : k_ssim_bwd_form<false>;     // the compiled form of this launch
    int rc = cdl_ensure_dynamic_lds((const void *)k_ssim_bwd, lds);
    if (rc) return rc;
    CDL_TRACE_NOTE("k_ssim_bwd<%d> level=%d cs=%d up=%d", g_cs ? 1 : 0, level, g_cs ? 1 : 0, up_x || up_y ? 1 : 0);
    k_ssim_bwd<<<(unsigned)blocks, NTHREADS, lds, S(stream)>>>(x, y, a, data_range, g_ssim, g_cs, gs, dx, dy, part, nc,
                                                              up_x, up_y);
    CDL_LAUNCH_CHECK();
    if (d_range) {
        CDL_TRACE_NOTE("k_ssim_reduce level=%d d_range", level);
        k_ssim_reduce<<<a.P, RED_THREADS, 0, S(stream)>>>(part, a.th * a.tw, g_cs ? 2 : 1, (double)a.Ho * a.Wo, g_ssim,
                                                          g_cs, gs, d_range, nullptr, 1, accum);
        CDL_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" {

size_t cdl_ssim_scratch_floats(int P, int H, int W, int taps) { return scratch_floats_of(P, H, W, taps); }

int cdl_ssim_fwd(const float *x, const float *y, int P, int H, int W, const float *win, int taps, float K1, float K2,
                 float kappa, const float *data_range, float *ssim, float *cs, float *scratch, size_t scratch_floats,
                 void *stream)
{
    Args a;
    if (!x || !y || !data_range || !ssim || !scratch) return CDL_EINVAL;
    if (!make_args(P, H, W, win, taps, K1, K2, kappa, TH, TW, false, a)) return CDL_EINVAL;
    if (!window_normalised(win, taps)) return CDL_EINVAL;
    if (scratch_floats < scratch_floats_of(P, H, W, taps)) return CDL_EINVAL;
    return launch_fwd(x, y, a, data_range, carve(scratch), nullptr, nullptr, ssim, cs, 1, 0, stream);
}

int cdl_ssim_bwd(const float *x, const float *y, int P, int H, int W, const float *win, int taps, float K1, float K2,
                 float kappa, const float *data_range, const float *g_ssim, float *dx, float *dy, float *d_range,
                 float *scratch, size_t scratch_floats, void *stream)
{
    Args a;
    if (!x || !y || !data_range || !g_ssim || !scratch || (!dx && !dy && !d_range)) return CDL_EINVAL;
    if (!make_args(P, H, W, win, taps, K1, K2, kappa, TH, TW, true, a)) return CDL_EINVAL;
    if (!window_normalised(win, taps)) return CDL_EINVAL;
    if (scratch_floats < scratch_floats_of(P, H, W, taps)) return CDL_EINVAL;
    return launch_bwd(x, y, a, data_range, g_ssim, nullptr, 1, dx, dy, d_range, 0, nullptr, nullptr, scratch, 0, stream);
}

size_t cdl_msssim_pyramid_floats(int P, int H, int W, int levels)
{
    Pyramid py;
    return make_pyramid(P, H, W, T_MIN, levels, py) ? py.off[levels] : 0;
}

size_t cdl_msssim_scratch_floats(int P, int H, int W, int taps, int levels)
{
    return ms_scratch_floats_of(P, H, W, taps, levels);
}

int cdl_msssim_fwd(const float *x, const float *y, int P, int H, int W, const float *win, int taps, float K1, float K2,
                   const float *data_range, int levels, float *pyr_x, float *pyr_y, float *vals, float *scratch,
                   size_t scratch_floats, void *stream)
{
    Pyramid py;
    Args a[LEVELS_MAX];
    if (!x || !y || !win || !data_range || !vals || !scratch) return CDL_EINVAL;
    if (!make_pyramid(P, H, W, taps, levels, py)) return CDL_EINVAL;
    if (levels > 1 && (!pyr_x || !pyr_y)) return CDL_EINVAL;
    if (!window_normalised(win, taps)) return CDL_EINVAL;
    if (scratch_floats < ms_scratch_floats_of(P, H, W, taps, levels)) return CDL_EINVAL;
    for (int i = 0; i < levels; ++i) {
        if (!make_args(P, py.H[i], py.W[i], win, taps, K1, K2, 1.0f, TH, TW, false, a[i])) return CDL_EINVAL;
        centre_pooled(a[i], i);
        if ((long long)P * a[i].th * a[i].tw > 0x7fffffffLL) return CDL_EUNSUPPORTED;
    }
    for (int i = 0; i < levels; ++i) {
        const float *xi = i ? pyr_x + py.off[i] : x, *yi = i ? pyr_y + py.off[i] : y;
        const bool pool = i + 1 < levels;
        float *v = vals + 2 * (size_t)i * P;
        int rc = launch_fwd(xi, yi, a[i], data_range, carve(scratch), pool ? pyr_x + py.off[i + 1] : nullptr,
                            pool ? pyr_y + py.off[i + 1] : nullptr, v, v + 1, 2, i, stream);
        if (rc) return rc;
    }
    return 0;
}

int cdl_msssim_bwd(const float *x, const float *y, const float *pyr_x, const float *pyr_y, int P, int H, int W,
                   const float *win, int taps, float K1, float K2, const float *data_range, int levels,
                   const float *g_vals, float *dx, float *dy, float *d_range, float *work, float *scratch,
                   size_t scratch_floats, void *stream)
{
    Pyramid py;
    Args a[LEVELS_MAX];
    if (!x || !y || !win || !data_range || !g_vals || !scratch || (!dx && !dy && !d_range)) return CDL_EINVAL;
    if (!make_pyramid(P, H, W, taps, levels, py)) return CDL_EINVAL;
    if (levels > 1 && (!pyr_x || !pyr_y || ((dx || dy) && !work))) return CDL_EINVAL;
    if (!window_normalised(win, taps)) return CDL_EINVAL;
    if (scratch_floats < ms_scratch_floats_of(P, H, W, taps, levels)) return CDL_EINVAL;
    for (int i = 0; i < levels; ++i) {
        if (!make_args(P, py.H[i], py.W[i], win, taps, K1, K2, 1.0f, TH, TW, true, a[i])) return CDL_EINVAL;
        centre_pooled(a[i], i);
        if ((long long)P * a[i].th * a[i].tw > 0x7fffffffLL) return CDL_EUNSUPPORTED;
    }
    float *wx = work, *wy = work ? work + py.off[levels] : nullptr;       // level i >= 1: at off[i], as in pyr_*
    for (int i = levels - 1; i >= 0; --i) {
        const float *xi = i ? pyr_x + py.off[i] : x, *yi = i ? pyr_y + py.off[i] : y;
        const bool top = i == levels - 1;
        float *dxi = !dx ? nullptr : i ? wx + py.off[i] : dx;
        float *dyi = !dy ? nullptr : i ? wy + py.off[i] : dy;
        const float *g = g_vals + 2 * (size_t)i * P;
        int rc = launch_bwd(xi, yi, a[i], data_range, g, g + 1, 2, dxi, dyi, d_range, top ? 0 : 1,
                            dx && !top ? wx + py.off[i + 1] : nullptr, dy && !top ? wy + py.off[i + 1] : nullptr, scratch,
                            i, stream);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
