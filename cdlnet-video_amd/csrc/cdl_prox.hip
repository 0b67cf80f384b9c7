// Proximal maps of the CSR temporal variants: prox_CSR and prox_CSR_f2
// of the reference's model/net.py:229-262, forward and reverse, as pointwise passes over the fat
// (N, M, D', H', W') code tensors with per-(sample, channel) thresholds.
//
// The maps are discontinuous when a threshold is negative (ST(x, t<0) jumps by 2|t| at x = 0), so the
// forward kernel keeps the reference's evaluation order term by term and forbids fma contraction: a
// re-association that moves an intermediate across 0 by one ulp would change the result by |t|.
#include "cdl_common.h"

namespace {

__device__ __forceinline__ float sgn(float x) { return cdl_sgn(x); }

// d ST(x,t) / dx and d ST(x,t) / dt as autograd sees sign(x) * relu(|x| - t)  (sign has zero gradient)
// (the gate itself, cdl_st_dx, lives in cdl_common.h beside the tangents of the two maps)
__device__ __forceinline__ float st_dx(float x, float t) { return cdl_st_dx(x, t) ? 1.0f : 0.0f; }
__device__ __forceinline__ float st_dt(float x, float t) { return (fabsf(x) - t > 0.0f) ? -sgn(x) : 0.0f; }

using Prox1 = cdl_prox1;
using Prox2 = cdl_prox2;
__device__ __forceinline__ Prox1 prox1(float u, float zp, float lam, float gam) { return cdl_prox_csr1(u, zp, lam, gam); }
__device__ __forceinline__ Prox2 prox2(float u, float zp, float za, float lam, float g1, float g2)
{
    return cdl_prox_csr2(u, zp, za, lam, g1, g2);
}

// Thresholds of any broadcast shape (cdl_bcast, include/cdlnet_hip.h): element (n, m, pix) reads thr[n*s.n + m*s.m + pix*s.p],
// a stride being 0 on a broadcast axis.  ROW is the form of the nets' own thresholds, one value per (sample, channel) row.
struct Bcast3 {
    cdl_bcast lam, g1, g2;
};
constexpr cdl_bcast ROW(int M) { return cdl_bcast{M, 1, 0}; }
__host__ __device__ __forceinline__ bool is_row(const cdl_bcast &s, int M) { return s.n == M && s.m == 1 && s.p == 0; }
__device__ __forceinline__ size_t at(const cdl_bcast &s, int n, int m, size_t pix)
{
    return (size_t)n * (size_t)s.n + (size_t)m * (size_t)s.m + pix * (size_t)s.p;
}

// ---- the tangent under a noise-level map: the thresholds of element (n, m, pix) are
// cdl_map_threshold(lam0[n,m], cmap[n,pix], tsl[0,m]) and the same with tsl[1,m], tsl[2,m] for gam1, gam2 -- the function of
// the primal's CSR epilogue, so the gates are the primal's bit for bit; no threshold enters a value.  The GRID is that of
// prox_bwd_map (map_chunks, map_msplits): one workgroup takes MAP_PIX pixels of one sample and a range of channels.  Within
// it the threads are laid out differently: a thread holds ONE pixel's map value in a register while it walks the channels,
// whose constant parts and slopes are wave-uniform (scalar loads), then steps 256 pixels on -- MAP_PXT pixels per thread one
// after the other, not MAP_PXT at once in registers as prox_bwd_map keeps them.  Entered from k_prox_fwd on a launch-uniform
// branch (TanMap::cmap) with a grid of its own shape.  out may alias in: a thread reads its element before it writes it.
struct TanMap {
    const float *cmap, *tsl;   // (N, pixels), (3, M); cmap == nullptr: the row / broadcast forms
    int chunks, MS;            // pixel chunks, channel ranges: the grid is chunks * MS * N workgroups
};
constexpr int MAP_PXT = 4;                 // pixels of a chunk per thread (prox_bwd_map: held in registers together)
constexpr int MAP_PIX = 256 * MAP_PXT;     // pixels of a chunk, both map kernels

template <bool F2>
__device__ __forceinline__ void prox_tangent_map(const float *in, const float *__restrict__ up, const float *__restrict__ zp,
                                                 const float *__restrict__ za, const float *__restrict__ lam,
                                                 const float *__restrict__ g1, const float *__restrict__ g2,
                                                 const float *__restrict__ zpd, const float *__restrict__ zad, float *out,
                                                 size_t per_m, int M, const TanMap &tm)
{
    const float *__restrict__ cmap = tm.cmap, *__restrict__ tsl = tm.tsl;
    const int chunks = tm.chunks, MS = tm.MS;
    int b = blockIdx.x;
    const int chunk = b % chunks;
    b /= chunks;
    const int ms = b % MS, n = b / MS;
    const int mper = (M + MS - 1) / MS, m_lo = ms * mper, m_hi = m_lo + mper < M ? m_lo + mper : M;
    const size_t lo = (size_t)chunk * MAP_PIX, hi = lo + MAP_PIX < per_m ? lo + MAP_PIX : per_m;
#pragma unroll 1
    for (size_t j = lo + threadIdx.x; j < hi; j += 256) {
        const float c = cmap[(size_t)n * per_m + j];
        for (int m = m_lo; m < m_hi; ++m) {
            const size_t row = (size_t)n * M + m, i = row * per_m + j;
            const float l = cdl_map_threshold(lam[row], c, tsl[m]), a1 = cdl_map_threshold(g1[row], c, tsl[M + m]);
            const float ud = in[i], dp = zpd ? zpd[i] : 0.0f;
            if (!F2)
                out[i] = cdl_prox_csr1_tangent(prox1(up[i], zp[i], l, a1), l, ud, dp);
            else
                out[i] = cdl_prox_csr2_tangent(prox2(up[i], zp[i], za[i], l, a1, cdl_map_threshold(g2[row], c, tsl[2 * M + m])),
                                               l, ud, dp, zad ? zad[i] : 0.0f);
        }
    }
}

// The map itself (up == nullptr: in = u, out = prox(u; zp[, za])) or its tangent at the primal (up, zp[, za]) along
// (in = ud, zpd, zad; a null neighbour tangent is a zero one): one kernel, one launch site (launch_prox).  out may alias in
// (each thread reads its element before it writes it).  M == 0: every threshold is in the row form (index = row); M > 0:
// the general broadcast form `bs` of the map itself (up == nullptr), M the channel count.  tm.cmap: the tangent under a
// noise-level map (prox_tangent_map above), M the channel count, the grid tm.chunks * tm.MS * N workgroups.
// (8 waves per SIMD asked for: the map branch's loop invariants otherwise fill the scalar file and cost every form a wave.)
__global__ __launch_bounds__(256, 8) void k_prox_fwd(const float *in, const float *__restrict__ up,
                                                  const float *__restrict__ zp, const float *__restrict__ za,
                                                  const float *__restrict__ lam, const float *__restrict__ g1,
                                                  const float *__restrict__ g2, const float *__restrict__ zpd,
                                                  const float *__restrict__ zad, float *out, size_t total, size_t per_m,
                                                  int M, Bcast3 bs, TanMap tm)
{
    if (tm.cmap) {                                                   // uniform: the whole launch takes the map form
        if (za)
            prox_tangent_map<true>(in, up, zp, za, lam, g1, g2, zpd, zad, out, per_m, M, tm);
        else
            prox_tangent_map<false>(in, up, zp, nullptr, lam, g1, nullptr, zpd, nullptr, out, per_m, M, tm);
        return;
    }
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / per_m;
    if (M > 0) {                                                     // uniform: the whole launch takes one form
        const size_t pix = i - row * per_m;                          // (the map only: the tangent's callers pass rows)
        const int n = (int)(row / (size_t)M), m = (int)(row - (size_t)n * M);
        const float l = lam[at(bs.lam, n, m, pix)], a1 = g1[at(bs.g1, n, m, pix)];
        out[i] = za ? prox2(in[i], zp[i], za[i], l, a1, g2[at(bs.g2, n, m, pix)]).z : prox1(in[i], zp[i], l, a1).z;
        return;
    }
    if (!up) {
        out[i] = za ? prox2(in[i], zp[i], za[i], lam[row], g1[row], g2[row]).z : prox1(in[i], zp[i], lam[row], g1[row]).z;
        return;
    }
    const float ud = in[i], l = lam[row], dp = zpd ? zpd[i] : 0.0f;
    if (!za) {
        out[i] = cdl_prox_csr1_tangent(prox1(up[i], zp[i], l, g1[row]), l, ud, dp);
        return;
    }
    out[i] = cdl_prox_csr2_tangent(prox2(up[i], zp[i], za[i], l, g1[row], g2[row]), l, ud, dp, zad ? zad[i] : 0.0f);
}

// One (row, split) of the reverse pass.  EL: some threshold has spatial extent -- it is read per element, and its
// per-element gradient goes to el_l / el_1 / el_2 (each nullable) for the host to reduce over its broadcast axes; the row
// sums are formed all the same.  !EL is the loop of the row form, thresholds in scalar registers.
struct Sums3 {
    float l, g1, g2;
};

template <bool EL>
__device__ __forceinline__ Sums3 prox_bwd_span(const float *__restrict__ gz, const float *__restrict__ u,
                                              const float *__restrict__ zp, const float *__restrict__ za,
                                              const float *__restrict__ lam, const float *__restrict__ g1,
                                              const float *__restrict__ g2, float *__restrict__ gu,
                                              float *__restrict__ gzp, float *__restrict__ gza, size_t base, size_t lo,
                                              size_t hi, size_t ol, size_t o1, size_t o2, bool el_lam, bool el_g1, bool el_g2,
                                              float *__restrict__ el_l, float *__restrict__ el_1,
                                              float *__restrict__ el_2)
{
    float sl = 0.0f, s1 = 0.0f, s2 = 0.0f;
    const float l0 = lam[ol], a10 = g1[o1], a20 = g2 ? g2[o2] : 0.0f;
    for (size_t j = lo + threadIdx.x; j < hi; j += 256) {
        const size_t i = base + j;
        const float l = (EL && el_lam) ? lam[ol + j] : l0;
        const float a1 = (EL && el_g1) ? g1[o1 + j] : a10;
        const float a2 = (EL && el_g2) ? g2[o2 + j] : a20;
        const float g = gz[i], uu = u[i], p = zp[i];
        if (!za) {
            const Prox1 q = prox1(uu, p, l, a1);
            const float gm = g * st_dx(q.m, l);
            const float ga = gm * st_dx(q.a, q.tg);
            const float gtg = gm * st_dt(q.a, q.tg);
            gu[i] = ga;
            if (gzp) gzp[i] += gm - ga;
            sl += g * st_dt(q.m, l) + gtg * a1 + (gm - ga) * q.s;
            s1 += gtg * l;
            if (EL) {
                if (el_l) el_l[i] = g * st_dt(q.m, l) + gtg * a1 + (gm - ga) * q.s;
                if (el_1) el_1[i] = gtg * l;
            }
        } else {
            const float a = za[i];
            const Prox2 q = prox2(uu, p, a, l, a1, a2);
            const float gm = g * st_dx(q.m, l);
            const float gb = gm * st_dx(q.b, q.t2);
            const float gt2 = gm * st_dt(q.b, q.t2);
            const float ga = gb * st_dx(q.a, q.t1);
            const float gt1 = gb * st_dt(q.a, q.t1);
            const float gcb = gm - gb;
            gu[i] = ga;
            if (gzp) gzp[i] -= ga;
            if (gza) gza[i] += gcb;
            const float p1 = (gb - gm) * q.sa + gcb * q.sap + gt1;      // gradient w.r.t. the product lam*g1
            const float p2 = -ga * q.spa + gt2;                          // ... lam*g2
            sl += g * st_dt(q.m, l) - ga * q.sp + gcb * q.sa_ + p1 * a1 + p2 * a2;
            s1 += p1 * l;
            s2 += p2 * l;
            if (EL) {
                if (el_l) el_l[i] = g * st_dt(q.m, l) - ga * q.sp + gcb * q.sa_ + p1 * a1 + p2 * a2;
                if (el_1) el_1[i] = p1 * l;
                if (el_2) el_2[i] = p2 * l;
            }
        }
    }
    return Sums3{sl, s1, s2};
}

// ---- the reverse pass under a noise-level map: lam = lam0[n,m] + cmap[n,pix] * tsl[m], and the
// same for gam1, gam2.  The threshold sums run over pixels, the map gradient over channels, so one workgroup takes MAP_PIX
// pixels of one sample (MAP_PXT per thread, the map values in registers) and walks a range of channels: the map gradient
// accumulates in registers, channel after channel, and each wave leaves its [sum s, sum cmap s] of every family per channel
// (no barrier, no LDS).  prox_fold_map and dcmap_fold add the partials in a fixed order; nothing fat is written beside
// gu and the neighbour gradients.  These are the map forms of k_prox_bwd and k_prox_fold: each is entered from its kernel
// on a launch-uniform branch (ProxMap::cmap), with a grid of its own shape, so the reverse pass stays one launch pair.
struct ProxMap {
    const float *cmap, *tsl;   // (N, pixels), (3, M); cmap == nullptr: the row / broadcast forms
    float *dcp, *dcmap;        // map-gradient partials of the channel ranges (scratch), dL/dcmap (both nullable)
    int N, chunks, MS;         // samples, pixel chunks, channel ranges: k_prox_bwd's grid is their product
    size_t NP;                 // N * pixels: the elements of dcmap
};

template <bool F2>
__device__ __forceinline__ void prox_bwd_map(const float *gz, const float *__restrict__ u, const float *__restrict__ zp,
                                             const float *__restrict__ za, const float *__restrict__ lam,
                                             const float *__restrict__ g1, const float *__restrict__ g2, float *gu,
                                             float *__restrict__ gzp, float *__restrict__ gza, float *__restrict__ part,
                                             size_t per_m, int M, const ProxMap &mp)
{
    constexpr int NQ = F2 ? 6 : 4;
    const float *__restrict__ cmap = mp.cmap, *__restrict__ tsl = mp.tsl;
    float *__restrict__ dcp = mp.dcp;
    const int N = mp.N, chunks = mp.chunks, MS = mp.MS;
    int b = blockIdx.x;
    const int chunk = b % chunks;
    b /= chunks;
    const int ms = b % MS, n = b / MS;
    const int mper = (M + MS - 1) / MS, m_lo = ms * mper, m_hi = m_lo + mper < M ? m_lo + mper : M;
    const size_t j0 = (size_t)chunk * MAP_PIX + threadIdx.x;
    float cm[MAP_PXT], dc[MAP_PXT];
#pragma unroll
    for (int p = 0; p < MAP_PXT; ++p) {
        const size_t j = j0 + (size_t)p * 256;
        cm[p] = j < per_m ? cmap[(size_t)n * per_m + j] : 0.0f;
        dc[p] = 0.0f;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int m = m_lo; m < m_hi; ++m) {
        const size_t row = (size_t)n * M + m, base = row * per_m;
        const float l0 = lam[row], a10 = g1[row], a20 = F2 ? g2[row] : 0.0f;
        const float tl = tsl[m], t1 = tsl[M + m], t2 = F2 ? tsl[2 * M + m] : 0.0f;
        float sq[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int p = 0; p < MAP_PXT; ++p) {
            const size_t j = j0 + (size_t)p * 256;
            if (j >= per_m) continue;
            const size_t i = base + j;
            const float c = cm[p];
            const float l = cdl_map_threshold(l0, c, tl), a1 = cdl_map_threshold(a10, c, t1);
            const float g = gz[i], uu = u[i], pv = zp[i];
            float el, e1, e2 = 0.0f;                                  // the element's threshold gradients (prox_bwd_span)
            if (!F2) {
                const Prox1 q = prox1(uu, pv, l, a1);
                const float gm = g * st_dx(q.m, l);
                const float ga = gm * st_dx(q.a, q.tg);
                const float gtg = gm * st_dt(q.a, q.tg);
                gu[i] = ga;
                if (gzp) gzp[i] += gm - ga;
                el = g * st_dt(q.m, l) + gtg * a1 + (gm - ga) * q.s;
                e1 = gtg * l;
            } else {
                const float a2 = cdl_map_threshold(a20, c, t2);
                const Prox2 q = prox2(uu, pv, za[i], l, a1, a2);
                const float gm = g * st_dx(q.m, l);
                const float gb = gm * st_dx(q.b, q.t2);
                const float gt2 = gm * st_dt(q.b, q.t2);
                const float ga = gb * st_dx(q.a, q.t1);
                const float gt1 = gb * st_dt(q.a, q.t1);
                const float gcb = gm - gb;
                gu[i] = ga;
                if (gzp) gzp[i] -= ga;
                if (gza) gza[i] += gcb;
                const float p1 = (gb - gm) * q.sa + gcb * q.sap + gt1;
                const float p2 = -ga * q.spa + gt2;
                el = g * st_dt(q.m, l) - ga * q.sp + gcb * q.sa_ + p1 * a1 + p2 * a2;
                e1 = p1 * l;
                e2 = p2 * l;
            }
            sq[0] += el;
            sq[1] = fmaf(c, el, sq[1]);
            sq[2] += e1;
            sq[3] = fmaf(c, e1, sq[3]);
            if (F2) {
                sq[4] += e2;
                sq[5] = fmaf(c, e2, sq[5]);
            }
            dc[p] += fmaf(t2, e2, fmaf(t1, e1, tl * el));
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            for (int off = 32; off > 0; off >>= 1) sq[q] += __shfl_down(sq[q], off, 64);
        if (lane == 0) {
            float *dst = part + ((row * chunks + chunk) * 4 + wv) * 6;
#pragma unroll
            for (int q = 0; q < NQ; ++q) dst[q] = sq[q];
        }
    }
    if (!dcp) return;
#pragma unroll
    for (int p = 0; p < MAP_PXT; ++p) {
        const size_t j = j0 + (size_t)p * 256;
        if (j < per_m) dcp[((size_t)ms * N + n) * per_m + j] = dc[p];
    }
}

// d(t[k,0,m]) = sum_{n,pix} s, d(t[k,1,m]) = sum_{n,pix} cmap s for the three families from the S wave partials of every
// (n, m) row: one wave (a 64-thread workgroup of k_prox_fold) per channel, the lanes split the partials, a fixed exchange
// tree adds them, samples in order.
__device__ __forceinline__ void prox_fold_map(const float *__restrict__ part, float *__restrict__ dlam,
                                              float *__restrict__ dg1, float *__restrict__ dg2, int N, int M, int S, int m)
{
    const int lane = threadIdx.x;
    const int NQ = dg2 ? 6 : 4;
    float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int n = 0; n < N; ++n) {
        const float *pr = part + ((size_t)n * M + m) * S * 6;
        for (int q = 0; q < NQ; ++q) {
            float v = 0.0f;
            for (int s = lane; s < S; s += 64) v += pr[(size_t)s * 6 + q];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            a[q] += v;
        }
    }
    if (lane != 0) return;
    dlam[m] = a[0], dlam[M + m] = a[1];
    dg1[m] = a[2], dg1[M + m] = a[3];
    if (dg2) dg2[m] = a[4], dg2[M + m] = a[5];
}

// dcmap[n,pix] += sum over the MS channel ranges of their partial map gradients, in order (element o of N * pixels)
__device__ __forceinline__ void dcmap_fold(const float *__restrict__ dcp, float *__restrict__ dcmap, size_t NP, int MS, size_t o)
{
    if (o >= NP) return;
    float v = 0.0f;
    for (int ms = 0; ms < MS; ++ms) v += dcp[(size_t)ms * NP + o];
    dcmap[o] += v;
}

// Reverse of the map for one (row, split): gu, the neighbour-code gradients (accumulated: a neighbour
// feeds every iteration) and this split's three threshold sums into part[(row*S + split)*3 + {0,1,2}].
// M == 0: thresholds in the row form (index = row); M > 0: in the broadcast form `bs`, M channels.  el_*: see prox_bwd_span.
// mp.cmap: the map form (prox_bwd_map), M the channel count, the grid mp.chunks * mp.MS * mp.N workgroups.
__global__ __launch_bounds__(256) void k_prox_bwd(const float *__restrict__ gz, const float *__restrict__ u,
                                                  const float *__restrict__ zp, const float *__restrict__ za,
                                                  const float *__restrict__ lam, const float *__restrict__ g1,
                                                  const float *__restrict__ g2, float *__restrict__ gu,
                                                  float *__restrict__ gzp, float *__restrict__ gza,
                                                  float *__restrict__ part, size_t per_m, int S, int M, Bcast3 bs,
                                                  float *__restrict__ el_l, float *__restrict__ el_1,
                                                  float *__restrict__ el_2, ProxMap mp)
{
    if (mp.cmap) {                                                   // uniform: the whole launch takes the map form
        if (za)
            prox_bwd_map<true>(gz, u, zp, za, lam, g1, g2, gu, gzp, gza, part, per_m, M, mp);
        else
            prox_bwd_map<false>(gz, u, zp, nullptr, lam, g1, nullptr, gu, gzp, nullptr, part, per_m, M, mp);
        return;
    }
    __shared__ float red[3][4];
    const int row = blockIdx.x / S, sp = blockIdx.x % S;
    const size_t chunk = (per_m + S - 1) / S;
    const size_t lo = (size_t)sp * chunk, hi = lo + chunk < per_m ? lo + chunk : per_m;
    const size_t base = (size_t)row * per_m;
    size_t ol = (size_t)row, o1 = ol, o2 = ol;                       // M == 0: every threshold in the row form
    if (M > 0) {
        const int n = row / M, m = row - n * M;
        ol = at(bs.lam, n, m, 0), o1 = at(bs.g1, n, m, 0), o2 = at(bs.g2, n, m, 0);
    }
    const bool el_lam = bs.lam.p != 0, el_g1 = bs.g1.p != 0, el_g2 = g2 && bs.g2.p != 0;
    const Sums3 sums =
        (el_lam | el_g1 | el_g2)
            ? prox_bwd_span<true>(gz, u, zp, za, lam, g1, g2, gu, gzp, gza, base, lo, hi, ol, o1, o2, el_lam, el_g1, el_g2,
                                  el_l, el_1, el_2)
            : prox_bwd_span<false>(gz, u, zp, za, lam, g1, g2, gu, gzp, gza, base, lo, hi, ol, o1, o2, false, false, false,
                                   nullptr, nullptr, nullptr);
    float sl = sums.l, s1 = sums.g1, s2 = sums.g2;
    for (int off = 32; off > 0; off >>= 1) {
        sl += __shfl_down(sl, off, 64);
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
    }
    if (threadIdx.x % 64 == 0) {
        red[0][threadIdx.x / 64] = sl;
        red[1][threadIdx.x / 64] = s1;
        red[2][threadIdx.x / 64] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        part[(size_t)blockIdx.x * 3 + threadIdx.x] =
            (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// d(t[k,0,m]) = sum_n s[n,m], d(t[k,1,m]) = sum_n c[n] s[n,m] for each of the three threshold families
// (lam = t[k,0] + c t[k,1] etc., net.py:444-452).  One thread per (family, m); fixed order.  slope == 0: only the first row
// is written (the per-row sums of the broadcast form: N = 1, M = rows).  dsum_n (nullable): see below.
__global__ void k_prox_fold(const float *__restrict__ part, const float *__restrict__ c, float *__restrict__ dlam,
                            float *__restrict__ dg1, float *__restrict__ dg2, int N, int M, int S, int slope,
                            float *__restrict__ dsum_n, ProxMap mp)
{
    if (mp.cmap) {               // the map form: workgroup m < M folds channel m (S wave partials per row), the others dcmap
        if ((int)blockIdx.x < M)
            prox_fold_map(part, dlam, dg1, dg2, N, M, S, (int)blockIdx.x);
        else if (mp.dcmap)
            dcmap_fold(mp.dcp, mp.dcmap, mp.NP, mp.MS, (size_t)(blockIdx.x - M) * 64 + threadIdx.x);
        return;
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * M) return;
    const int fam = i / M, m = i % M;
    float *dst = fam == 0 ? dlam : (fam == 1 ? dg1 : dg2);
    if (!dst) return;
    float a0 = 0.0f, a1 = 0.0f;
    for (int n = 0; n < N; ++n) {
        float v = 0.0f;
        for (int s = 0; s < S; ++s) v += part[((size_t)(n * M + m) * S + s) * 3 + fam];
        if (dsum_n) dsum_n[((size_t)fam * N + n) * M + m] = v;      // the sums per sample, (3, N, M): dL/dc[n] is formed from them
        a0 += v;
        if (c) a1 = fmaf(c[n], v, a1);
    }
    dst[m] = a0;
    if (slope) dst[M + m] = a1;
}

size_t map_chunks(size_t per_m) { return (per_m + MAP_PIX - 1) / MAP_PIX; }

// channel ranges of the map kernel: about 1024 workgroups, at least 8 channels each
int map_msplits(int N, int M, size_t chunks)
{
    const size_t wgs = (size_t)N * chunks;
    size_t MS = (1024 + wgs - 1) / wgs;
    const size_t most = (size_t)(M + 7) / 8;
    if (MS > most) MS = most;
    return MS < 1 ? 1 : (int)MS;
}

int splits_for(int rows, size_t per_m)
{
    int S = (2048 + rows - 1) / rows;                 // ~8 blocks per CU
    const size_t most = (per_m + 1023) / 1024;        // at least 1024 elements per block
    if ((size_t)S > most) S = (int)most;
    return S < 1 ? 1 : S;
}

size_t code_elems(const cdl_geom *g) { return (size_t)(g->D / g->sd) * (g->H / g->sh) * (g->W / g->sw); }

}  // namespace

extern "C" {

static int launch_prox(const cdl_geom *g, const float *in, const float *up, const float *z_prev, const float *z_after,
                       const float *lam, const float *gam1, const float *gam2, const float *zd_prev, const float *zd_after,
                       float *out, const Bcast3 &bs, void *stream, const TanMap &tm = TanMap{})
{
    const size_t per_m = code_elems(g), total = (size_t)g->N * g->M * per_m;
    const bool rows = is_row(bs.lam, g->M) && is_row(bs.g1, g->M) && (!z_after || is_row(bs.g2, g->M));
    // the tangent's map form: a grid of its own shape (prox_tangent_map), the constant parts in the row form
    const size_t blocks = tm.cmap ? (size_t)tm.chunks * tm.MS * g->N : (total + 255) / 256;
    if (blocks >= ((size_t)1 << 31) || (up && !rows) || (tm.cmap && !up)) return CDL_EUNSUPPORTED;
    if (tm.cmap) CDL_TRACE_NOTE("map MS=%d chunks=%d", tm.MS, tm.chunks);
    k_prox_fwd<<<(unsigned)blocks, 256, 0, S(stream)>>>(in, up, z_prev, z_after, lam, gam1, gam2, zd_prev,
                                                                         zd_after, out, total, per_m,
                                                                         (rows && !tm.cmap) ? 0 : g->M, bs, tm);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_prox_csr_b(const cdl_geom *g, const float *u, const float *z_prev, const float *z_after, const float *lam,
                   const cdl_bcast *s_lam, const float *gam1, const cdl_bcast *s_gam1, const float *gam2,
                   const cdl_bcast *s_gam2, float *out, void *stream)
{
    if (!cdl_geom_ok(g) || !u || !z_prev || !lam || !gam1 || !out) return CDL_EINVAL;
    if (z_after && !gam2) return CDL_EINVAL;
    const size_t per_m = code_elems(g);
    if (!cdl_bcast_ok(s_lam, g->M, per_m) || !cdl_bcast_ok(s_gam1, g->M, per_m)) return CDL_EINVAL;
    if (z_after && !cdl_bcast_ok(s_gam2, g->M, per_m)) return CDL_EINVAL;
    const Bcast3 bs{*s_lam, *s_gam1, z_after ? *s_gam2 : cdl_bcast{0, 0, 0}};
    return launch_prox(g, u, nullptr, z_prev, z_after, lam, gam1, gam2, nullptr, nullptr, out, bs, stream);
}

int cdl_prox_csr(const cdl_geom *g, const float *u, const float *z_prev, const float *z_after, const float *lam,
                 const float *gam1, const float *gam2, float *out, void *stream)
{
    if (!g) return CDL_EINVAL;
    const cdl_bcast r = ROW(g->M);
    return cdl_prox_csr_b(g, u, z_prev, z_after, lam, &r, gam1, &r, gam2, &r, out, stream);
}

int cdl_prox_csr_tangent(const cdl_geom *g, const float *ud, const float *u, const float *z_prev, const float *z_after,
                         const float *lam, const float *gam1, const float *gam2, const float *zd_prev,
                         const float *zd_after, float *out, const float *cmap, const float *tslope, void *stream)
{
    if (!cdl_geom_ok(g) || !ud || !u || !z_prev || !lam || !gam1 || !out) return CDL_EINVAL;
    if (z_after ? !gam2 : (zd_after != nullptr)) return CDL_EINVAL;
    if (out == u || out == z_prev || out == z_after || out == zd_prev || out == zd_after) return CDL_EINVAL;
    if ((cmap == nullptr) != (tslope == nullptr)) return CDL_EINVAL;
    TanMap tm{};
    if (cmap) {
        const size_t chunks = map_chunks(code_elems(g));
        if (chunks >= ((size_t)1 << 28)) return CDL_EUNSUPPORTED;
        tm = TanMap{cmap, tslope, (int)chunks, map_msplits(g->N, g->M, chunks)};
    }
    const Bcast3 bs{ROW(g->M), ROW(g->M), ROW(g->M)};
    return launch_prox(g, ud, u, z_prev, z_after, lam, gam1, gam2, zd_prev, zd_after, out, bs, stream, tm);
}

size_t cdl_prox_csr_scratch_floats(const cdl_geom *g)
{
    if (!cdl_geom_ok(g)) return 0;
    const size_t per_m = code_elems(g), chunks = map_chunks(per_m);
    const size_t rowf = (size_t)g->N * g->M * splits_for(g->N * g->M, per_m) * 3;
    // with a map: 4 wave partials of 6 sums per (row, pixel chunk), then the map-gradient partials of the channel ranges
    const size_t mapf = (size_t)g->N * g->M * chunks * 4 * 6 + (size_t)map_msplits(g->N, g->M, chunks) * g->N * per_m;
    return rowf > mapf ? rowf : mapf;
}

// The one launch pair of the reverse pass.  fold_N x fold_M = rows: (N, M) with c folds the row sums into the (2, M)
// parameter slices; (1, rows) without slope leaves them per row.  A NULL d* is not written.  mp.cmap: the map form of
// both kernels (prox_bwd_map; prox_fold_map with dcmap_fold behind it), each on a grid of its own shape.
static int launch_prox_bwd(const cdl_geom *g, const float *gz, const float *u, const float *z_prev, const float *z_after,
                           const float *lam, const float *gam1, const float *gam2, const Bcast3 &bs, const float *c,
                           float *gu, float *gz_prev, float *gz_after, float *dlam, float *dgam1, float *dgam2,
                           float *el_l, float *el_1, float *el_2, float *scratch, int fold_N, int fold_M, int slope,
                           void *stream, float *dsum_n = nullptr, const ProxMap &mp = ProxMap{})
{
    const size_t per_m = code_elems(g);
    const int rows = g->N * g->M;
    const bool rowform = is_row(bs.lam, g->M) && is_row(bs.g1, g->M) && (!z_after || is_row(bs.g2, g->M));
    // the partials per (n, m) row that the fold reads: the splits of the row forms, four waves per pixel chunk of the map's
    const int Sp = mp.cmap ? mp.chunks * 4 : splits_for(rows, per_m);
    const size_t wgs = mp.cmap ? (size_t)mp.chunks * mp.MS * mp.N : (size_t)rows * Sp;
    size_t folds = (size_t)(3 * fold_M + 63) / 64;
    if (mp.cmap) folds = (size_t)g->M + (mp.dcmap ? (mp.NP + 63) / 64 : 0);
    if (wgs >= ((size_t)1 << 31) || folds >= ((size_t)1 << 31)) return CDL_EUNSUPPORTED;
    if (mp.cmap) CDL_TRACE_NOTE("map MS=%d chunks=%d", mp.MS, mp.chunks);
    k_prox_bwd<<<(unsigned)wgs, 256, 0, S(stream)>>>(gz, u, z_prev, z_after, lam, gam1, gam2, gu, gz_prev, gz_after, scratch,
                                                     per_m, Sp, (rowform && !mp.cmap) ? 0 : g->M, bs, el_l, el_1, el_2, mp);
    CDL_LAUNCH_CHECK();
    if (!dlam && !dgam1 && !dgam2) return 0;
    k_prox_fold<<<(unsigned)folds, 64, 0, S(stream)>>>(scratch, c, dlam, dgam1, dgam2, fold_N, fold_M, Sp, slope, dsum_n, mp);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_prox_csr_bwd(const cdl_geom *g, const float *gz, const float *u, const float *z_prev,
                     const float *z_after, const float *lam, const float *gam1, const float *gam2,
                     const float *c, float *gu, float *gz_prev, float *gz_after, float *dlam, float *dgam1,
                     float *dgam2, float *scratch, size_t scratch_floats, const float *cmap, const float *tslope,
                     float *dcmap, float *dsum_n, void *stream)
{
    if (!cdl_geom_ok(g) || !gz || !u || !z_prev || !lam || !gam1 || !gu || !dlam || !dgam1 || !scratch)
        return CDL_EINVAL;
    if (z_after && (!gam2 || !dgam2)) return CDL_EINVAL;
    if (!z_after && gz_after) return CDL_EINVAL;
    if (scratch_floats < cdl_prox_csr_scratch_floats(g)) return CDL_EINVAL;
    if (cmap ? (!tslope || c || dsum_n) : (tslope || dcmap)) return CDL_EINVAL;   // a map replaces c; dcmap where dsum_n was
    ProxMap mp{};
    if (cmap) {
        const size_t per_m = code_elems(g), chunks = map_chunks(per_m);
        if (chunks >= ((size_t)1 << 28)) return CDL_EUNSUPPORTED;
        // scratch: the wave partials of every (row, pixel chunk), then the map-gradient partials of the channel ranges
        mp = ProxMap{cmap, tslope, dcmap ? scratch + (size_t)g->N * g->M * chunks * 4 * 6 : nullptr, dcmap, g->N, (int)chunks,
                     map_msplits(g->N, g->M, chunks), (size_t)g->N * per_m};
    }
    const Bcast3 bs{ROW(g->M), ROW(g->M), ROW(g->M)};
    return launch_prox_bwd(g, gz, u, z_prev, z_after, lam, gam1, gam2, bs, c, gu, gz_prev, gz_after, dlam, dgam1,
                           z_after ? dgam2 : nullptr, nullptr, nullptr, nullptr, scratch, g->N, g->M, 1, stream, dsum_n, mp);
}

int cdl_prox_csr_b_bwd(const cdl_geom *g, const float *gz, const float *u, const float *z_prev, const float *z_after,
                       const float *lam, const cdl_bcast *s_lam, const float *gam1, const cdl_bcast *s_gam1,
                       const float *gam2, const cdl_bcast *s_gam2, float *gu, float *gz_prev, float *gz_after,
                       float *dlam, float *dgam1, float *dgam2, float *scratch, size_t scratch_floats, void *stream)
{
    if (!cdl_geom_ok(g) || !gz || !u || !z_prev || !lam || !gam1 || !gu || !scratch) return CDL_EINVAL;
    if (z_after && !gam2) return CDL_EINVAL;
    if (!z_after && (gz_after || dgam2)) return CDL_EINVAL;
    const size_t per_m = code_elems(g);
    if (!cdl_bcast_ok(s_lam, g->M, per_m) || !cdl_bcast_ok(s_gam1, g->M, per_m)) return CDL_EINVAL;
    if (z_after && !cdl_bcast_ok(s_gam2, g->M, per_m)) return CDL_EINVAL;
    if (scratch_floats < cdl_prox_csr_scratch_floats(g)) return CDL_EINVAL;
    const Bcast3 bs{*s_lam, *s_gam1, z_after ? *s_gam2 : cdl_bcast{0, 0, 0}};
    // a threshold with spatial extent takes its gradient per element, the others as row sums
    const bool el = bs.lam.p != 0, e1 = bs.g1.p != 0, e2 = bs.g2.p != 0;
    return launch_prox_bwd(g, gz, u, z_prev, z_after, lam, gam1, gam2, bs, nullptr, gu, gz_prev, gz_after,
                           el ? nullptr : dlam, e1 ? nullptr : dgam1, e2 ? nullptr : dgam2, el ? dlam : nullptr,
                           e1 ? dgam1 : nullptr, e2 ? dgam2 : nullptr, scratch, 1, g->N * g->M, 0, stream);
}

}  // extern "C"
