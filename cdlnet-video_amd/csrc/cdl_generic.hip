// Shape-generic fp32 kernels (any C, M, odd P per axis, stride, 2-D or 3-D).
// LDS-tiled direct correlation on the vector ALUs: the always-available path and the
// on-device yardstick for the MFMA kernels in cdl_fused2d.hip.  One code path serves
// CDLNet (D = 1), the Bayer-masked JDD variant (C = 3, mask), CDLNetVideo and GDLNet.
#include "cdl_common.h"

namespace {

constexpr int TILE = 16;          // 16 x 16 output pixels per 256-thread workgroup
constexpr int MCHUNK = 8;         // code channels accumulated per thread per pass

// ------------------------------------------------------------------------------------------
// analysis: acc[m] = sum_{c,kd,ki,kj} x[c, zd*sd-pd+kd, zy*sh-ph+ki, zx*sw-pw+kj] * w[m,c,kd,ki,kj]
// One workgroup = one (n, zd, 16x16 tile of (zy,zx)); the image patch (all C, Pd slices, halo)
// is staged once in LDS and reused for every code channel; filter taps are wave-uniform
// scalar loads.  MAP: the thresholds follow a noise-level map (cdl_map_args), read once per pixel.
template <bool MAP>
__global__ __launch_bounds__(256) void k_analysis(cdl_geom g, const float *__restrict__ x,
                                                  const float *__restrict__ w, float alpha,
                                                  const float *__restrict__ zin,
                                                  const float *__restrict__ gate,
                                                  const float *__restrict__ tau,
                                                  float *__restrict__ out, int tilesX, int tilesY, cdl_prox_args px,
                                                  cdl_map_args mp)
{
    extern __shared__ float patch[];
    const int Dz = g.D / g.sd, Hz = g.H / g.sh, Wz = g.W / g.sw;
    const int PH = (TILE - 1) * g.sh + g.Ph, PW = (TILE - 1) * g.sw + g.Pw;
    int b = blockIdx.x;
    const int tx = b % tilesX; b /= tilesX;
    const int ty = b % tilesY; b /= tilesY;
    const int zd = b;
    const int n = blockIdx.y;
    const int ly = threadIdx.x / TILE, lx = threadIdx.x % TILE;
    const int zy = ty * TILE + ly, zx = tx * TILE + lx;
    const int y0 = ty * TILE * g.sh - g.ph, x0 = tx * TILE * g.sw - g.pw, d0 = zd * g.sd - g.pd;

    const int plane = PH * PW, pvol = g.C * g.Pd * plane;
    for (int i = threadIdx.x; i < pvol; i += 256) {
        int px = i % PW, r = i / PW;
        int py = r % PH; r /= PH;
        int kd = r % g.Pd, c = r / g.Pd;
        int d = d0 + kd, yy = y0 + py, xx = x0 + px;
        float v = 0.0f;
        if (d >= 0 && d < g.D && yy >= 0 && yy < g.H && xx >= 0 && xx < g.W)
            v = x[((((size_t)n * g.C + c) * g.D + d) * g.H + yy) * g.W + xx];
        patch[i] = v;
    }
    __syncthreads();

    const int taps = g.Pd * g.Ph * g.Pw, wrow = g.C * taps;
    const bool live = zy < Hz && zx < Wz;
    const float *pbase = patch + (ly * g.sh) * PW + lx * g.sw;
    float cm = 0.0f;
    if (MAP && live) cm = mp.cmap[(((size_t)n * Dz + zd) * Hz + zy) * Wz + zx];
    for (int m0 = 0; m0 < g.M; m0 += MCHUNK) {
        float acc[MCHUNK];
#pragma unroll
        for (int j = 0; j < MCHUNK; ++j) acc[j] = 0.0f;
        const float *wp[MCHUNK];
#pragma unroll
        for (int j = 0; j < MCHUNK; ++j) wp[j] = w + (size_t)min(m0 + j, g.M - 1) * wrow;
        int widx = 0;
        for (int c = 0; c < g.C; ++c)
            for (int kd = 0; kd < g.Pd; ++kd) {
                const float *prow = pbase + (c * g.Pd + kd) * plane;
                for (int ki = 0; ki < g.Ph; ++ki, prow += PW)
                    for (int kj = 0; kj < g.Pw; ++kj, ++widx) {
                        float v = prow[kj];
#pragma unroll
                        for (int j = 0; j < MCHUNK; ++j) acc[j] = fmaf(v, wp[j][widx], acc[j]);
                    }
            }
        if (live) {
#pragma unroll
            for (int j = 0; j < MCHUNK; ++j) {
                int m = m0 + j;
                if (m < g.M) {
                    size_t idx = ((((size_t)n * g.M + m) * Dz + zd) * Hz + zy) * Wz + zx;
                    float base = 0.0f;
                    if (zin) {
                        base = zin[idx];
                        if (gate && gate[idx] == 0.0f) base = 0.0f;
                    }
                    float u = fmaf(alpha, acc[j], base);
                    if (MAP)
                        out[idx] = px.zp ? cdl_prox_apply_map(px, mp, u, idx, n * g.M + m, m, g.M, cm)
                                         : cdl_shrink(u, cdl_map_threshold(tau[n * g.M + m], cm, mp.tslope[m]));
                    else
                    out[idx] = px.zp ? cdl_prox_apply(px, u, idx, n * g.M + m)
                                     : (tau ? cdl_shrink(u, tau[n * g.M + m]) : u);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// synthesis: v[c,d,y,x] = sum_{m,kd,ki,kj} zg[m,(d+pd-kd)/sd,(y+ph-ki)/sh,(x+pw-kj)/sw] * w[m,c,kd,ki,kj]
// over taps whose numerators are multiples of the stride.  One workgroup = one (n, d, 16x16
// tile of (y,x)); code channels are staged through LDS MCHUNK at a time (with the support
// gate applied on the way in); up to 4 image channels accumulate per pass.
__global__ __launch_bounds__(256) void k_synthesis(cdl_geom g, const float *__restrict__ z,
                                                   const float *__restrict__ gate,
                                                   const float *__restrict__ w, float alpha,
                                                   const float *__restrict__ mask,
                                                   const float *__restrict__ sub,
                                                   float *__restrict__ out, int tilesX, int tilesY,
                                                   int PZD, int PZH, int PZW)
{
    extern __shared__ float patch[];
    const int Dz = g.D / g.sd, Hz = g.H / g.sh, Wz = g.W / g.sw;
    int b = blockIdx.x;
    const int tx = b % tilesX; b /= tilesX;
    const int ty = b % tilesY; b /= tilesY;
    const int d = b;
    const int n = blockIdx.y;
    const int ly = threadIdx.x / TILE, lx = threadIdx.x % TILE;
    const int y = ty * TILE + ly, xo = tx * TILE + lx;
    const int zd_lo = cdl_floordiv(d + g.pd - (g.Pd - 1), g.sd);
    const int zy_lo = cdl_floordiv(ty * TILE + g.ph - (g.Ph - 1), g.sh);
    const int zx_lo = cdl_floordiv(tx * TILE + g.pw - (g.Pw - 1), g.sw);
    const int plane = PZH * PZW, pvol = PZD * plane;
    const int taps = g.Pd * g.Ph * g.Pw;
    const bool live = y < g.H && xo < g.W;

    for (int c0 = 0; c0 < g.C; c0 += 4) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int m0 = 0; m0 < g.M; m0 += MCHUNK) {
            __syncthreads();
            for (int i = threadIdx.x; i < MCHUNK * pvol; i += 256) {
                int px = i % PZW, r = i / PZW;
                int py = r % PZH; r /= PZH;
                int pd_ = r % PZD, mm = r / PZD;
                int m = m0 + mm, zd = zd_lo + pd_, zy = zy_lo + py, zx = zx_lo + px;
                float v = 0.0f;
                if (m < g.M && zd >= 0 && zd < Dz && zy >= 0 && zy < Hz && zx >= 0 && zx < Wz) {
                    size_t idx = ((((size_t)n * g.M + m) * Dz + zd) * Hz + zy) * Wz + zx;
                    v = z[idx];
                    if (gate && gate[idx] == 0.0f) v = 0.0f;
                }
                patch[i] = v;
            }
            __syncthreads();
            for (int kd = 0; kd < g.Pd; ++kd) {
                int td = d + g.pd - kd + g.sd * g.Pd;              // shifted positive
                if (td % g.sd) continue;
                int zd = td / g.sd - g.Pd - zd_lo;
                for (int ki = 0; ki < g.Ph; ++ki) {
                    int tyy = y + g.ph - ki + g.sh * g.Ph;
                    if (tyy % g.sh) continue;
                    int zy = tyy / g.sh - g.Ph - zy_lo;
                    for (int kj = 0; kj < g.Pw; ++kj) {
                        int txx = xo + g.pw - kj + g.sw * g.Pw;
                        if (txx % g.sw) continue;
                        int zx = txx / g.sw - g.Pw - zx_lo;
                        int tap = (kd * g.Ph + ki) * g.Pw + kj;
                        const float *pp = patch + (zd * PZH + zy) * PZW + zx;
                        const int mlim = min(MCHUNK, g.M - m0);
                        for (int mm = 0; mm < mlim; ++mm) {
                            float v = pp[mm * pvol];
                            const float *wr = w + ((size_t)(m0 + mm) * g.C + c0) * taps + tap;
#pragma unroll
                            for (int cc = 0; cc < 4; ++cc)
                                if (c0 + cc < g.C) acc[cc] = fmaf(v, wr[cc * taps], acc[cc]);
                        }
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                int c = c0 + cc;
                if (c < g.C) {
                    size_t idx = ((((size_t)n * g.C + c) * g.D + d) * g.H + y) * g.W + xo;
                    float v = alpha * acc[cc];
                    if (mask) v *= mask[idx];
                    if (sub) v -= sub[idx];
                    out[idx] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// filter gradient: one workgroup per (m, c, kd, ki) filter row, Pw taps accumulated per
// thread over a strided sweep of every code pixel; zeros of the (sparse / gated) code are
// skipped.  Fixed reduction order -> deterministic.
constexpr int PWMAX = 16;

__global__ __launch_bounds__(256) void k_wgrad(cdl_geom g, const float *__restrict__ z,
                                               const float *__restrict__ gate,
                                               const float *__restrict__ x, float alpha,
                                               float *__restrict__ dw)
{
    __shared__ float red[4][PWMAX];
    const int Dz = g.D / g.sd, Hz = g.H / g.sh, Wz = g.W / g.sw;
    const int m = blockIdx.x;
    int r = blockIdx.y;
    const int ki = r % g.Ph; r /= g.Ph;
    const int kd = r % g.Pd;
    const int c = r / g.Pd;
    float acc[PWMAX];
#pragma unroll
    for (int j = 0; j < PWMAX; ++j) acc[j] = 0.0f;

    const int rows = g.N * Dz * Hz;                  // (n, zd, zy) rows of the code
    for (int row = threadIdx.x / 64; row < rows; row += 4) {      // one wave per code row
        int zy = row % Hz, t = row / Hz;
        int zd = t % Dz, n = t / Dz;
        int d = zd * g.sd - g.pd + kd, y = zy * g.sh - g.ph + ki;
        if (d < 0 || d >= g.D || y < 0 || y >= g.H) continue;
        const float *zr = z + ((((size_t)n * g.M + m) * Dz + zd) * Hz + zy) * Wz;
        const float *gr = gate ? gate + ((((size_t)n * g.M + m) * Dz + zd) * Hz + zy) * Wz : nullptr;
        const float *xr = x + ((((size_t)n * g.C + c) * g.D + d) * g.H + y) * g.W;
        for (int zx = threadIdx.x % 64; zx < Wz; zx += 64) {
            float zv = zr[zx];
            if (gr && gr[zx] == 0.0f) zv = 0.0f;
            if (zv == 0.0f) continue;
            int xb = zx * g.sw - g.pw;
#pragma unroll
            for (int kj = 0; kj < PWMAX; ++kj) {
                int xx = xb + kj;
                if (kj < g.Pw && xx >= 0 && xx < g.W) acc[kj] = fmaf(zv, xr[xx], acc[kj]);
            }
        }
    }
    const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
#pragma unroll
    for (int kj = 0; kj < PWMAX; ++kj) {
        float v = acc[kj];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[wv][kj] = v;
    }
    __syncthreads();
    if (threadIdx.x < g.Pw) {
        float v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        dw[((((size_t)m * g.C + c) * g.Pd + kd) * g.Ph + ki) * g.Pw + threadIdx.x] = alpha * v;
    }
}

// ------------------------------------------------------------------------------------------
// threshold gradient, stage 1: s[n,m] = -sum_pix sign(zout) * g over the support of zout.  MAP: a second partial,
// weighted by the noise-level map cmap[n,pix], goes to s[rows * S + .] (dt1 of a map call).
template <bool GATE_INPLACE, bool MAP>
__global__ __launch_bounds__(256) void k_tau_partial(float *__restrict__ gup,
                                                     const float *__restrict__ zout,
                                                     float *__restrict__ s, size_t per_m, int S,
                                                     const float *__restrict__ cmap, int M)
{
    // one workgroup per (row, split): the N*M rows alone are too few workgroups for a batch of a few clips, and
    // 4 independent accumulators keep 8 loads in flight per thread
    __shared__ float red[4], redw[4];
    const int row = blockIdx.x / S, sp = blockIdx.x % S;
    const size_t chunk = (per_m + S - 1) / S;
    const size_t lo = (size_t)sp * chunk, hi = lo + chunk < per_m ? lo + chunk : per_m;
    const size_t base = (size_t)row * per_m;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, aw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float *cm = MAP ? cmap + (size_t)(row / M) * per_m : nullptr;
    size_t i = lo + threadIdx.x;
    for (; i + 3 * 256 < hi; i += 4 * 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float zv = zout[base + i + u * 256], gv = gup[base + i + u * 256];
            const float t = zv > 0.0f ? -gv : (zv < 0.0f ? gv : 0.0f);
            a[u] += t;
            if (MAP) aw[u] = fmaf(cm[i + u * 256], t, aw[u]);
            if (GATE_INPLACE && zv == 0.0f && gv != 0.0f) gup[base + i + u * 256] = 0.0f;
        }
    }
    for (; i < hi; i += 256) {
        const float zv = zout[base + i], gv = gup[base + i];
        const float t = zv > 0.0f ? -gv : (zv < 0.0f ? gv : 0.0f);
        a[0] += t;
        if (MAP) aw[0] = fmaf(cm[i], t, aw[0]);
        if (GATE_INPLACE && zv == 0.0f && gv != 0.0f) gup[base + i] = 0.0f;
    }
    float acc = (a[0] + a[1]) + (a[2] + a[3]);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (threadIdx.x % 64 == 0) red[threadIdx.x / 64] = acc;
    if (MAP) {
        float accw = (aw[0] + aw[1]) + (aw[2] + aw[3]);
        for (int off = 32; off > 0; off >>= 1) accw += __shfl_down(accw, off, 64);
        if (threadIdx.x % 64 == 0) redw[threadIdx.x / 64] = accw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        if (MAP) s[(size_t)gridDim.x + blockIdx.x] = (redw[0] + redw[1]) + (redw[2] + redw[3]);
    }
}

// stage 2: dt0[m] = sum_n sum_splits s[n,m,.]; dt1[m] = sum_n c[n] * (sum_splits s[n,m,.]), or (MAP) the sum of the
// map-weighted partials sw[n,m,.]
template <bool MAP>
__global__ void k_tau_final(const float *__restrict__ s, const float *__restrict__ c,
                            float *__restrict__ dt0, float *__restrict__ dt1, int N, int M, int S,
                            const float *__restrict__ sw)
{
    int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float a0 = 0.0f, a1 = 0.0f;
    for (int n = 0; n < N; ++n) {
        float v = 0.0f;
        for (int k = 0; k < S; ++k) v += s[(size_t)(n * M + m) * S + k];
        a0 += v;
        if (MAP) {
            float vw = 0.0f;
            for (int k = 0; k < S; ++k) vw += sw[(size_t)(n * M + m) * S + k];
            a1 += vw;
        } else
        if (c) a1 = fmaf(c[n], v, a1);
    }
    dt0[m] = a0;
    dt1[m] = a1;
}

// gradient of the noise-level map, one iteration: dcmap[n,pix] (+)= sum_m tslope[m] * (-sign(z) * du)[n,m,pix].  A
// channel reduction: one thread per code pixel walks the M channels in order (coalesced across the wave, four loads of
// each tensor in flight) -- deterministic.
template <bool ACC>
__global__ __launch_bounds__(256) void k_sigma_grad(const float *__restrict__ du, const float *__restrict__ z,
                                                    const float *__restrict__ tslope, float *__restrict__ dcmap,
                                                    int M, size_t per_m)
{
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= per_m) return;
    const int n = blockIdx.y;
    const size_t base = (size_t)n * M * per_m + pix;
    float a = 0.0f;
    int m = 0;
    for (; m + 4 <= M; m += 4) {
        float zv[4], gv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            zv[u] = z[base + (size_t)(m + u) * per_m];
            gv[u] = du[base + (size_t)(m + u) * per_m];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) a = fmaf(tslope[m + u], zv[u] > 0.0f ? -gv[u] : (zv[u] < 0.0f ? gv[u] : 0.0f), a);
    }
    for (; m < M; ++m) {
        const float zv = z[base + (size_t)m * per_m], gv = du[base + (size_t)m * per_m];
        a = fmaf(tslope[m], zv > 0.0f ? -gv : (zv < 0.0f ? gv : 0.0f), a);
    }
    const size_t o = (size_t)n * per_m + pix;
    dcmap[o] = ACC ? dcmap[o] + a : a;
}

// ST(x, tau) with tau in the row form (M == 0: tau[i / per_m]) or of any broadcast shape (M > 0 channels, strides st:
// cdl_bcast).  gup != nullptr: the reverse pass instead -- out = gup where autograd's d ST / dx is 1, else 0, and (nullable)
// dtau_el = -sign(x) * out, the per-element threshold gradient.
__global__ void k_shrink(const float *__restrict__ x, const float *__restrict__ tau,
                         float *__restrict__ out, size_t total, size_t per_m, int M, cdl_bcast st,
                         const float *__restrict__ gup, float *__restrict__ dtau_el)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / per_m;
    size_t it = row;
    if (M > 0) {
        const size_t n = row / (size_t)M, m = row - n * (size_t)M;
        it = n * (size_t)st.n + m * (size_t)st.m + (i - row * per_m) * (size_t)st.p;
    }
    if (!gup) {
        out[i] = cdl_shrink(x[i], tau[it]);
        return;
    }
    const float xv = x[i], gx = cdl_st_dx(xv, tau[it]) ? gup[i] : 0.0f;
    out[i] = gx;
    if (dtau_el) dtau_el[i] = xv > 0.0f ? -gx : gx;
}

__global__ void k_thresholds(const float *__restrict__ t, const float *__restrict__ c,
                             float *__restrict__ tau, int K, int N, int M)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K * N * M) return;
    int m = i % M, n = (i / M) % N, k = i / (M * N);
    float v = t[(k * 2 + 0) * M + m];
    if (c) {
#pragma clang fp contract(off)                     // mul then add (two roundings), as torch does
        float prod = c[n] * t[(k * 2 + 1) * M + m];
        v = v + prod;
    }
    tau[i] = v;
}

// ------------------------------------------------------------------------------------------
// pre / post processing
__global__ __launch_bounds__(1024) void k_sample_sums(const float *__restrict__ y,
                                                      const float *__restrict__ mask,
                                                      float *__restrict__ mean, size_t per_n)
{
    // one workgroup per sample; 4 independent double accumulators per thread so that the loads of a
    // single frame (65536 pixels) are not one dependent chain per thread (was 94 us for a 256 x 256 frame)
    __shared__ double red[2][16];
    const size_t base = (size_t)blockIdx.x * per_n;
    double sy[4] = {0.0, 0.0, 0.0, 0.0}, sm[4] = {0.0, 0.0, 0.0, 0.0};
    size_t i = threadIdx.x;
    for (; i + 3 * 1024 < per_n; i += 4 * 1024) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sy[u] += y[base + i + u * 1024];
            if (mask) sm[u] += mask[base + i + u * 1024];
        }
    }
    for (; i < per_n; i += 1024) {
        sy[0] += y[base + i];
        if (mask) sm[0] += mask[base + i];
    }
    double ty = (sy[0] + sy[1]) + (sy[2] + sy[3]), tm = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    for (int off = 32; off > 0; off >>= 1) {
        ty += __shfl_down(ty, off, 64);
        tm += __shfl_down(tm, off, 64);
    }
    if (threadIdx.x % 64 == 0) { red[0][threadIdx.x / 64] = ty; red[1][threadIdx.x / 64] = tm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < 16; ++k) { a += red[0][k]; b += red[1][k]; }
        mean[blockIdx.x] = (float)(a / (mask ? b : (double)per_n));
    }
}

// Few large samples (a batch of 8 clips): SPLIT workgroups per sample write double partials (into the not yet written
// output buffer), one thread per sample adds them in order -- one workgroup per sample took 106 us for 8 x 3 x 256 x 256.
constexpr int SUM_SPLIT = 16;
__global__ __launch_bounds__(1024) void k_sample_sums_split(const float *__restrict__ y, const float *__restrict__ mask,
                                                            double *__restrict__ part, size_t per_n)
{
    __shared__ double red[2][16];
    const int n = blockIdx.x / SUM_SPLIT, sp = blockIdx.x % SUM_SPLIT;
    const size_t chunk = (per_n + SUM_SPLIT - 1) / SUM_SPLIT;
    const size_t lo = (size_t)sp * chunk, hi = lo + chunk < per_n ? lo + chunk : per_n;
    const size_t base = (size_t)n * per_n;
    double sy[4] = {0.0, 0.0, 0.0, 0.0}, sm[4] = {0.0, 0.0, 0.0, 0.0};
    size_t i = lo + threadIdx.x;
    for (; i + 3 * 1024 < hi; i += 4 * 1024) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sy[u] += y[base + i + u * 1024];
            if (mask) sm[u] += mask[base + i + u * 1024];
        }
    }
    for (; i < hi; i += 1024) {
        sy[0] += y[base + i];
        if (mask) sm[0] += mask[base + i];
    }
    double ty = (sy[0] + sy[1]) + (sy[2] + sy[3]), tm = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    for (int off = 32; off > 0; off >>= 1) {
        ty += __shfl_down(ty, off, 64);
        tm += __shfl_down(tm, off, 64);
    }
    if (threadIdx.x % 64 == 0) { red[0][threadIdx.x / 64] = ty; red[1][threadIdx.x / 64] = tm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < 16; ++k) { a += red[0][k]; b += red[1][k]; }
        part[2 * blockIdx.x] = a;
        part[2 * blockIdx.x + 1] = b;
    }
}

__global__ void k_sample_sums_final(const double *__restrict__ part, float *__restrict__ mean, int N, size_t per_n,
                                    int masked)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < SUM_SPLIT; ++k) { a += part[2 * (n * SUM_SPLIT + k)]; b += part[2 * (n * SUM_SPLIT + k) + 1]; }
    mean[n] = (float)(a / (masked ? b : (double)per_n));
}

__device__ __forceinline__ int reflect(int q, int lo, int L)
{
    int u = q - lo;
    if (u < 0) u = -u;
    if (u >= L) u = 2 * (L - 1) - u;
    return u;
}

__global__ void k_pad_center(const float *__restrict__ y, const float *__restrict__ mask,
                             const float *__restrict__ mean, float *__restrict__ yp,
                             float *__restrict__ mask_p, int N, int C, int D, int H, int W,
                             int d_lo, int h_lo, int w_lo, int Dp, int Hp, int Wp)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)N * C * Dp * Hp * Wp;
    if (i >= total) return;
    int xq = i % Wp; size_t r = i / Wp;
    int yq = r % Hp; r /= Hp;
    int dq = r % Dp; r /= Dp;
    int c = r % C, n = r / C;
    size_t src = ((((size_t)n * C + c) * D + reflect(dq, d_lo, D)) * H + reflect(yq, h_lo, H)) * W +
                 reflect(xq, w_lo, W);
    float v = y[src] - mean[n];
    if (mask) {
        float mv = mask[src];
        v *= mv;
        mask_p[i] = mv;
    }
    yp[i] = v;
}

__global__ void k_crop_add(const float *__restrict__ xp, const float *__restrict__ mean,
                           float *__restrict__ xhat, int N, int C, int D, int H, int W,
                           int d_lo, int h_lo, int w_lo, int Dp, int Hp, int Wp)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)N * C * D * H * W;
    if (i >= total) return;
    int xq = i % W; size_t r = i / W;
    int yq = r % H; r /= H;
    int dq = r % D; r /= D;
    int c = r % C, n = r / C;
    size_t src = ((((size_t)n * C + c) * Dp + dq + d_lo) * Hp + yq + h_lo) * Wp + xq + w_lo;
    xhat[i] = xp[src] + mean[n];
}

__global__ void k_embed(const float *__restrict__ gx, float *__restrict__ gxp, int N, int C, int D,
                        int H, int W, int d_lo, int h_lo, int w_lo, int Dp, int Hp, int Wp)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)N * C * Dp * Hp * Wp;
    if (i >= total) return;
    int xq = (int)(i % Wp) - w_lo; size_t r = i / Wp;
    int yq = (int)(r % Hp) - h_lo; r /= Hp;
    int dq = (int)(r % Dp) - d_lo; r /= Dp;
    float v = 0.0f;
    if (xq >= 0 && xq < W && yq >= 0 && yq < H && dq >= 0 && dq < D)
        v = gx[((r * D + dq) * H + yq) * W + xq];            // r = n*C + c
    gxp[i] = v;
}

// ------------------------------------------------------------------------------------------
// unit-ball projection: one wave per filter, up to 64 banks of identical shape in one launch (bank = blockIdx.y):
// project() of a K = 30 net is 60 banks, i.e. 60 launches of a 4 us kernel otherwise
constexpr int PROJECT_BATCH = 64;
struct ProjectBatch {
    float *w[PROJECT_BATCH];
};
__global__ __launch_bounds__(64) void k_project_batch(ProjectBatch b, int flen)
{
    float *f = b.w[blockIdx.y] + (size_t)blockIdx.x * flen;
    float ss = 0.0f;
    for (int i = threadIdx.x; i < flen; i += 64) ss = fmaf(f[i], f[i], ss);
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    float scale = fminf(1.0f / sqrtf(ss), 1.0f);
    if (scale < 1.0f)
        for (int i = threadIdx.x; i < flen; i += 64) f[i] *= scale;
}

// ------------------------------------------------------------------------------------------
// Gabor dictionary synthesis and its adjoint: every bank of a net in ONE launch (blockIdx.y = bank): GDLNet re-synthesises its 2K banks on every forward
// (gabor.py:46-51 via net.py:659-675) -- per-bank launches made that 2K launches + 2K autograd nodes per sweep
constexpr int GABOR_BATCH = 48;
struct GaborBatch {
    const float *alpha[GABOR_BATCH], *a[GABOR_BATCH], *w0[GABOR_BATCH], *psi[GABOR_BATCH];
    const float *dw[GABOR_BATCH];            // backward: upstream filter gradient (nullptr: this bank got none)
    float *out[GABOR_BATCH];                 // forward: filters (M,C,P,P); backward: [dalpha | da | dw0 | dpsi] block
    float sgn[GABOR_BATCH];                  // -1 for the analysis (transpose) filter
};

__global__ void k_gabor_batch(GaborBatch b, int order, int MC, int P)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= MC * P * P) return;
    const float *alpha = b.alpha[k], *a = b.a[k], *w0 = b.w0[k], *psi = b.psi[k];
    const float sgn = b.sgn[k];
    int kj = i % P, ki = (i / P) % P, mc = i / (P * P);
    float gy = (float)ki - 0.5f * (P - 1), gx = (float)kj - 0.5f * (P - 1);
    float acc = 0.0f;
    for (int o = 0; o < order; ++o) {
        int q = o * MC + mc;
        float e0 = a[2 * q] * gy, e1 = a[2 * q + 1] * gx;
        float env = expf(-(e0 * e0 + e1 * e1));
        float ph = sgn * w0[2 * q] * gy + sgn * w0[2 * q + 1] * gx + sgn * psi[q];
        acc += alpha[q] * (env * cosf(ph));
    }
    b.out[k][i] = acc;
}

// out block of bank k: dalpha (order*MC) | da (2*order*MC) | dw0 (2*order*MC) | dpsi (order*MC); zeros when dw is null
__global__ void k_gabor_bwd_batch(GaborBatch b, int order, int MC, int P)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    const int nq = order * MC;
    if (q >= nq) return;
    float *out = b.out[k];
    float g_al = 0, g_a0 = 0, g_a1 = 0, g_f0 = 0, g_f1 = 0, g_ps = 0;
    const float *dw = b.dw[k];
    if (dw) {
        const float sgn = b.sgn[k];
        const int mc = q % MC;
        const float al = b.alpha[k][q], a0 = b.a[k][2 * q], a1 = b.a[k][2 * q + 1];
        const float f0 = sgn * b.w0[k][2 * q], f1 = sgn * b.w0[k][2 * q + 1], ps = sgn * b.psi[k][q];
        for (int ki = 0; ki < P; ++ki)
            for (int kj = 0; kj < P; ++kj) {
                float gy = (float)ki - 0.5f * (P - 1), gx = (float)kj - 0.5f * (P - 1);
                float e0 = a0 * gy, e1 = a1 * gx;
                float env = expf(-(e0 * e0 + e1 * e1));
                float ph = f0 * gy + f1 * gx + ps;
                float cs = cosf(ph), sn = sinf(ph);
                float up = dw[(size_t)mc * P * P + ki * P + kj];
                g_al += up * env * cs;
                float de = up * al * cs * env;
                g_a0 += de * (-2.0f * a0 * gy * gy);
                g_a1 += de * (-2.0f * a1 * gx * gx);
                float dp = -up * al * env * sn;
                g_f0 += dp * sgn * gy;
                g_f1 += dp * sgn * gx;
                g_ps += dp * sgn;
            }
    }
    out[q] = g_al;
    out[nq + 2 * q] = g_a0; out[nq + 2 * q + 1] = g_a1;
    out[3 * nq + 2 * q] = g_f0; out[3 * nq + 2 * q + 1] = g_f1;
    out[5 * nq + q] = g_ps;
}

}  // namespace

// ---- the plain tier: the last rung of the operators' ladder (cdl_operators.hip, which has checked the arguments).  No
// workspace; CDL_EUNSUPPORTED where a tile's patch exceeds the LDS or the filter row the kernel's registers.
int cdl_plain_analysis(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin, const float *gate,
                       const float *tau, float *out, const cdl_prox_args &px, void *stream, const cdl_map_args &mp)
{
    const int Dz = g->D / g->sd, Hz = g->H / g->sh, Wz = g->W / g->sw;
    const int tilesX = (Wz + TILE - 1) / TILE, tilesY = (Hz + TILE - 1) / TILE;
    const int PH = (TILE - 1) * g->sh + g->Ph, PW = (TILE - 1) * g->sw + g->Pw;
    size_t lds = (size_t)g->C * g->Pd * PH * PW * sizeof(float);
    if (lds > 160 * 1024) return CDL_EUNSUPPORTED;
    if (lds > 64 * 1024)
        CDL_TRY(cdl_ensure_dynamic_lds(mp.cmap ? (const void *)k_analysis<true> : (const void *)k_analysis<false>, (int)lds));
    dim3 grid((unsigned)(tilesX * tilesY * Dz), (unsigned)g->N);
    CDL_TRACE_NOTE("k_analysis<%s>", mp.cmap ? "true" : "false");
    if (mp.cmap)
        k_analysis<true><<<grid, 256, lds, S(stream)>>>(*g, x, w, alpha, zin, gate, tau, out, tilesX, tilesY, px, mp);
    else
        k_analysis<false><<<grid, 256, lds, S(stream)>>>(*g, x, w, alpha, zin, gate, tau, out, tilesX, tilesY, px, mp);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_plain_synthesis(const cdl_geom *g, const float *z, const float *gate, const float *w, float alpha,
                        const float *mask, const float *sub, float *out, void *stream)
{
    const int tilesX = (g->W + TILE - 1) / TILE, tilesY = (g->H + TILE - 1) / TILE;
    // upper bound on the code patch a 16x16 output tile (one d) can touch, per axis
    const int PZD = (g->Pd - 1) / g->sd + 2;
    const int PZH = (TILE - 1 + g->Ph - 1) / g->sh + 2;
    const int PZW = (TILE - 1 + g->Pw - 1) / g->sw + 2;
    size_t lds = (size_t)MCHUNK * PZD * PZH * PZW * sizeof(float);
    if (lds > 160 * 1024) return CDL_EUNSUPPORTED;
    if (lds > 64 * 1024) CDL_TRY(cdl_ensure_dynamic_lds((const void *)k_synthesis, (int)lds));
    dim3 grid((unsigned)(tilesX * tilesY * g->D), (unsigned)g->N);
    k_synthesis<<<grid, 256, lds, S(stream)>>>(*g, z, gate, w, alpha, mask, sub, out, tilesX, tilesY,
                                                PZD, PZH, PZW);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_plain_wgrad(const cdl_geom *g, const float *z, const float *gate, const float *x, float alpha, float *dw, void *stream)
{
    if (g->Pw > PWMAX) return CDL_EUNSUPPORTED;
    dim3 grid((unsigned)g->M, (unsigned)(g->C * g->Pd * g->Ph));
    k_wgrad<<<grid, 256, 0, S(stream)>>>(*g, z, gate, x, alpha, dw);
    CDL_LAUNCH_CHECK();
    return 0;
}

extern "C" {

const char *cdl_version(void) { return "cdlnet_hip 0.1 (gfx950)"; }

int cdl_preprocess(const float *y, const float *mask, float *yp, float *mask_p, float *mean,
                   int N, int C, int D, int H, int W, const int pads[6], void *stream)
{
    if (!y || !yp || !mean || !pads || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return CDL_EINVAL;
    if ((mask == nullptr) != (mask_p == nullptr)) return CDL_EINVAL;
    for (int i = 0; i < 6; ++i) if (pads[i] < 0) return CDL_EINVAL;
    // reflect padding needs pad < extent on that axis
    const int ext[3] = {D, H, W};
    for (int i = 0; i < 6; ++i) if (pads[i] && pads[i] >= ext[i / 2]) return CDL_EINVAL;
    size_t per_n = (size_t)C * D * H * W;
    int Dp = D + pads[0] + pads[1], Hp = H + pads[2] + pads[3], Wp = W + pads[4] + pads[5];
    size_t total = (size_t)N * C * Dp * Hp * Wp;
    // the split form parks its 2 * SUM_SPLIT doubles per sample at the start of yp, which k_pad_center overwrites next
    if (N < 32 && per_n >= 32768 && total * sizeof(float) >= (size_t)N * SUM_SPLIT * 2 * sizeof(double) &&
        (reinterpret_cast<size_t>(yp) & 7) == 0 && yp != y) {
        double *part = reinterpret_cast<double *>(yp);
        k_sample_sums_split<<<N * SUM_SPLIT, 1024, 0, S(stream)>>>(y, mask, part, per_n);
        CDL_LAUNCH_CHECK();
        k_sample_sums_final<<<(N + 63) / 64, 64, 0, S(stream)>>>(part, mean, N, per_n, mask ? 1 : 0);
        CDL_LAUNCH_CHECK();
    } else {
        k_sample_sums<<<N, 1024, 0, S(stream)>>>(y, mask, mean, per_n);
        CDL_LAUNCH_CHECK();
    }
    k_pad_center<<<(unsigned)((total + 255) / 256), 256, 0, S(stream)>>>(
        y, mask, mean, yp, mask_p, N, C, D, H, W, pads[0], pads[2], pads[4], Dp, Hp, Wp);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_postprocess(const float *xp, const float *mean, float *xhat, int N, int C, int D, int H,
                    int W, const int pads[6], void *stream)
{
    if (!xp || !mean || !xhat || !pads || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return CDL_EINVAL;
    int Dp = D + pads[0] + pads[1], Hp = H + pads[2] + pads[3], Wp = W + pads[4] + pads[5];
    size_t total = (size_t)N * C * D * H * W;
    k_crop_add<<<(unsigned)((total + 255) / 256), 256, 0, S(stream)>>>(
        xp, mean, xhat, N, C, D, H, W, pads[0], pads[2], pads[4], Dp, Hp, Wp);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_postprocess_bwd(const float *gxhat, float *gxp, int N, int C, int D, int H, int W,
                        const int pads[6], void *stream)
{
    if (!gxhat || !gxp || !pads || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return CDL_EINVAL;
    int Dp = D + pads[0] + pads[1], Hp = H + pads[2] + pads[3], Wp = W + pads[4] + pads[5];
    size_t total = (size_t)N * C * Dp * Hp * Wp;
    k_embed<<<(unsigned)((total + 255) / 256), 256, 0, S(stream)>>>(gxhat, gxp, N, C, D, H, W, pads[0],
                                                                  pads[2], pads[4], Dp, Hp, Wp);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_thresholds(const float *t, const float *c, float *tau, int K, int N, int M, void *stream)
{
    if (!t || !tau || K <= 0 || N <= 0 || M <= 0) return CDL_EINVAL;
    int total = K * N * M;
    k_thresholds<<<(total + 255) / 256, 256, 0, S(stream)>>>(t, c, tau, K, N, M);
    CDL_LAUNCH_CHECK();
    return 0;
}

static int launch_shrink(const float *x, const float *tau, float *out, size_t rows, size_t per_m, int M,
                         const cdl_bcast &st, const float *gup, float *dtau_el, void *stream)
{
    const size_t total = rows * per_m, blocks = (total + 255) / 256;
    if (blocks >= ((size_t)1 << 31)) return CDL_EUNSUPPORTED;
    k_shrink<<<(unsigned)blocks, 256, 0, S(stream)>>>(x, tau, out, total, per_m, M, st, gup, dtau_el);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_shrink(const float *x, const float *tau, float *out, int rows, size_t per_m, void *stream)
{
    if (!x || !tau || !out || rows <= 0 || per_m == 0) return CDL_EINVAL;
    return launch_shrink(x, tau, out, (size_t)rows, per_m, 0, cdl_bcast{0, 0, 0}, nullptr, nullptr, stream);
}

int cdl_shrink_b(const float *x, const float *tau, const cdl_bcast *s_tau, float *out, int N, int M, size_t per_m,
                 void *stream)
{
    if (!x || !tau || !out || N <= 0 || M <= 0 || per_m == 0 || !cdl_bcast_ok(s_tau, M, per_m)) return CDL_EINVAL;
    const bool row = s_tau->n == M && s_tau->m == 1 && s_tau->p == 0;
    return launch_shrink(x, tau, out, (size_t)N * M, per_m, row ? 0 : M, *s_tau, nullptr, nullptr, stream);
}

int cdl_shrink_b_bwd(const float *gup, const float *x, const float *tau, const cdl_bcast *s_tau, float *gx,
                     float *dtau_el, int N, int M, size_t per_m, void *stream)
{
    if (!gup || !x || !tau || !gx || N <= 0 || M <= 0 || per_m == 0 || !cdl_bcast_ok(s_tau, M, per_m))
        return CDL_EINVAL;
    return launch_shrink(x, tau, gx, (size_t)N * M, per_m, M, *s_tau, gup, dtau_el, stream);
}

static int tau_grad_impl(const cdl_geom *g, float *gup, const float *zout, const float *c, float *dt0, float *dt1,
                         float *scratch, bool gate_inplace, void *stream, float *dtau_n, const float *cmap)
{
    if (!cdl_geom_ok(g) || !gup || !zout || !dt0 || !dt1 || !scratch) return CDL_EINVAL;
    if (cmap && (c || dtau_n)) return CDL_EINVAL;               // a map replaces the per-sample scale
    size_t per_m = (size_t)(g->D / g->sd) * (g->H / g->sh) * (g->W / g->sw);
    // splits per (n, m) row: about 2048 workgroups of at least 4096 elements, at most CDL_TAU_SPLITS (the scratch)
    const int rows = g->N * g->M;
    int Sp = (2048 + rows - 1) / rows;
    const size_t most = (per_m + 4095) / 4096;
    if ((size_t)Sp > most) Sp = (int)most;
    if (Sp > CDL_TAU_SPLITS) Sp = CDL_TAU_SPLITS;
    if (Sp < 1) Sp = 1;
    if (cmap) {                                                   // weighted partials behind the plain ones
        CDL_TRACE_NOTE("k_tau_partial<%s,true>", gate_inplace ? "true" : "false");
        if (gate_inplace)
            k_tau_partial<true, true><<<(unsigned)(rows * Sp), 256, 0, S(stream)>>>(gup, zout, scratch, per_m, Sp, cmap, g->M);
        else
            k_tau_partial<false, true><<<(unsigned)(rows * Sp), 256, 0, S(stream)>>>(gup, zout, scratch, per_m, Sp, cmap, g->M);
        CDL_LAUNCH_CHECK();
        k_tau_final<true><<<(g->M + 63) / 64, 64, 0, S(stream)>>>(scratch, nullptr, dt0, dt1, g->N, g->M, Sp,
                                                                   scratch + (size_t)rows * Sp);
        CDL_LAUNCH_CHECK();
        return 0;
    }
    CDL_TRACE_NOTE("k_tau_partial<%s,false>", gate_inplace ? "true" : "false");
    if (gate_inplace)
        k_tau_partial<true, false><<<(unsigned)(rows * Sp), 256, 0, S(stream)>>>(gup, zout, scratch, per_m, Sp, nullptr, g->M);
    else
        k_tau_partial<false, false><<<(unsigned)(rows * Sp), 256, 0, S(stream)>>>(gup, zout, scratch, per_m, Sp, nullptr, g->M);
    CDL_LAUNCH_CHECK();
    k_tau_final<false><<<(g->M + 63) / 64, 64, 0, S(stream)>>>(scratch, c, dt0, dt1, g->N, g->M, Sp, nullptr);
    CDL_LAUNCH_CHECK();
    if (dtau_n)                                                   // per-sample: the Sp splits of row (n, m), in order
        return cdl_dtau_per_sample(scratch, g->N, g->M, Sp, (size_t)g->M * Sp, (size_t)Sp, 1, dtau_n, stream);
    return 0;
}

int cdl_tau_grad(const cdl_geom *g, const float *gup, const float *zout, const float *c, float *dt0, float *dt1,
                 float *dtau_n, float *scratch, const float *cmap, void *stream)
{
    return tau_grad_impl(g, const_cast<float *>(gup), zout, c, dt0, dt1, scratch, false, stream, dtau_n, cmap);
}

int cdl_tau_grad_gate(const cdl_geom *g, float *gup, const float *zout, const float *c, float *dt0, float *dt1,
                      float *dtau_n, float *scratch, const float *cmap, void *stream)
{
    return tau_grad_impl(g, gup, zout, c, dt0, dt1, scratch, true, stream, dtau_n, cmap);
}

int cdl_sigma_grad(const cdl_geom *g, const float *du, const float *z, const float *tslope, float *dcmap, int acc_add,
                   void *stream)
{
    if (!cdl_geom_ok(g) || !du || !z || !tslope || !dcmap) return CDL_EINVAL;
    const size_t per_m = (size_t)(g->D / g->sd) * (g->H / g->sh) * (g->W / g->sw);
    const size_t blocks = (per_m + 255) / 256;
    if (blocks >= ((size_t)1 << 31) || g->N > 65535) return CDL_EUNSUPPORTED;
    dim3 grid((unsigned)blocks, (unsigned)g->N);
    CDL_TRACE_NOTE("k_sigma_grad<%s>", acc_add ? "true" : "false");
    if (acc_add)
        k_sigma_grad<true><<<grid, 256, 0, S(stream)>>>(du, z, tslope, dcmap, g->M, per_m);
    else
        k_sigma_grad<false><<<grid, 256, 0, S(stream)>>>(du, z, tslope, dcmap, g->M, per_m);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_project_filter_banks(float *const *w, int nbanks, int nfilters, int flen, void *stream)
{
    if (!w || nbanks <= 0 || nfilters <= 0 || flen <= 0) return CDL_EINVAL;
    for (int b0 = 0; b0 < nbanks; b0 += PROJECT_BATCH) {
        const int nb = nbanks - b0 < PROJECT_BATCH ? nbanks - b0 : PROJECT_BATCH;
        ProjectBatch pb = {};
        for (int i = 0; i < nb; ++i) {
            if (!w[b0 + i]) return CDL_EINVAL;
            pb.w[i] = w[b0 + i];
        }
        k_project_batch<<<dim3((unsigned)nfilters, (unsigned)nb), 64, 0, S(stream)>>>(pb, flen);
        CDL_LAUNCH_CHECK();
    }
    return 0;
}

int cdl_gabor_filter_banks(int nbanks, const float *const *alpha, const float *const *a, const float *const *w0,
                           const float *const *psi, const int *transpose, float *const *w, int order, int M, int C,
                           int P, void *stream)
{
    if (nbanks <= 0 || !alpha || !a || !w0 || !psi || !transpose || !w || order <= 0 || M <= 0 || C <= 0 || P <= 0)
        return CDL_EINVAL;
    const int total = M * C * P * P;
    for (int k0 = 0; k0 < nbanks; k0 += GABOR_BATCH) {
        const int nb = nbanks - k0 < GABOR_BATCH ? nbanks - k0 : GABOR_BATCH;
        GaborBatch b = {};
        for (int i = 0; i < nb; ++i) {
            const int k = k0 + i;
            if (!alpha[k] || !a[k] || !w0[k] || !psi[k] || !w[k]) return CDL_EINVAL;
            b.alpha[i] = alpha[k]; b.a[i] = a[k]; b.w0[i] = w0[k]; b.psi[i] = psi[k]; b.out[i] = w[k];
            b.sgn[i] = transpose[k] ? -1.0f : 1.0f;
        }
        k_gabor_batch<<<dim3((unsigned)((total + 255) / 256), (unsigned)nb), 256, 0, S(stream)>>>(b, order, M * C, P);
        CDL_LAUNCH_CHECK();
    }
    return 0;
}

int cdl_gabor_filter_banks_bwd(int nbanks, const float *const *alpha, const float *const *a, const float *const *w0,
                               const float *const *psi, const int *transpose, const float *const *dw, float *const *grads,
                               int order, int M, int C, int P, void *stream)
{
    if (nbanks <= 0 || !alpha || !a || !w0 || !psi || !transpose || !dw || !grads || order <= 0 || M <= 0 || C <= 0 || P <= 0)
        return CDL_EINVAL;
    const int total = order * M * C;
    for (int k0 = 0; k0 < nbanks; k0 += GABOR_BATCH) {
        const int nb = nbanks - k0 < GABOR_BATCH ? nbanks - k0 : GABOR_BATCH;
        GaborBatch b = {};
        for (int i = 0; i < nb; ++i) {
            const int k = k0 + i;
            if (!alpha[k] || !a[k] || !w0[k] || !psi[k] || !grads[k]) return CDL_EINVAL;
            b.alpha[i] = alpha[k]; b.a[i] = a[k]; b.w0[i] = w0[k]; b.psi[i] = psi[k]; b.dw[i] = dw[k]; b.out[i] = grads[k];
            b.sgn[i] = transpose[k] ? -1.0f : 1.0f;
        }
        k_gabor_bwd_batch<<<dim3((unsigned)((total + 63) / 64), (unsigned)nb), 64, 0, S(stream)>>>(b, order, M * C, P);
        CDL_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
