// Gradients with respect to the observation and the noise level: the small kernels the reverse
// sweeps add when a caller asks for dL/dyp and the per-sample threshold gradients, and the adjoint of cdl_preprocess.
//   u_0 = A_0 yp,  u_k = z_k - A_k (mask B_k z_k - yp)   =>   dL/dyp = sum_k A_k^T du_k
//   tau[k,n,m] = t[k,0,m] + c[n] t[k,1,m]                =>   dL/dc[n] = sum_k sum_m t[k,1,m] dtau[k,n,m]  (host side)
#include "cdl_common.h"

namespace {

// dtau_n[n,m] = sum_{j<R} partial[n sN + m sM + j sR], j in order: one thread per (n, m), deterministic
__global__ __launch_bounds__(256) void k_dtau_per_sample(const float *__restrict__ partial, float *__restrict__ dtau_n,
                                                         int N, int M, int R, size_t sN, size_t sM, size_t sR)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * M) return;
    const int n = i / M, m = i - n * M;
    const float *p = partial + (size_t)n * sN + (size_t)m * sM;
    float a = 0.0f;
    for (int j = 0; j < R; ++j) a += p[(size_t)j * sR];
    dtau_n[i] = a;
}

// Generic sweep, iteration k >= 1, s = the UNMASKED A_k^T du_k (in q):  dyp (= or +=) s;  q = -mask s
__global__ __launch_bounds__(256) void k_dyp_split(float *__restrict__ q, const float *__restrict__ mask,
                                                   float *__restrict__ dyp, size_t total, int acc_add, int make_q)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float s = q[i];
    dyp[i] = acc_add ? dyp[i] + s : s;
    if (make_q) q[i] = mask ? -(mask[i] * s) : -s;
}

// The padded positions q whose reflect() source is u on one axis (cdl_generic.hip k_pad_center): u + lo itself, its
// mirror in the low pad and its mirror in the high pad.  Returns the count, positions in fixed order.
__device__ __forceinline__ int reflect_sources(int u, int lo, int hi, int L, int *q)
{
    int n = 0;
    if (u >= 1 && u <= lo) q[n++] = lo - u;
    q[n++] = u + lo;
    if (u <= L - 2 && u > L - 2 - hi) q[n++] = lo + 2 * (L - 1) - u;
    return n;
}

// G[n,c,d,h,w] = sum of dyp over the padded positions that copy (d,h,w): the adjoint of the reflect pad
__device__ __forceinline__ float pad_adjoint(const float *__restrict__ dyp_nc, int d, int h, int w, int D, int H, int W,
                                             const int *p, int Hp, int Wp)
{
    int qd[3], qh[3], qw[3];
    const int nd = reflect_sources(d, p[0], p[1], D, qd);
    const int nh = reflect_sources(h, p[2], p[3], H, qh);
    const int nw = reflect_sources(w, p[4], p[5], W, qw);
    float s = 0.0f;
    for (int a = 0; a < nd; ++a)
        for (int b = 0; b < nh; ++b)
            for (int e = 0; e < nw; ++e) s += dyp_nc[((size_t)qd[a] * Hp + qh[b]) * Wp + qw[e]];
    return s;
}

struct Pads6 { int p[6]; };

// One workgroup per sample.  Pass 1: the double sums of mask G, g_xhat and mask over the sample (fixed per-thread
// order, fixed tree); pass 2: dy = m G + (sum g_xhat - sum m G) / sum m, with m = mask, or 1 and sum m = C D H W.
__global__ __launch_bounds__(1024) void k_preprocess_bwd(const float *__restrict__ dyp, const float *__restrict__ g_xhat,
                                                         const float *__restrict__ mask, float *__restrict__ dy, int C,
                                                         int D, int H, int W, Pads6 pd)
{
    __shared__ double red[3][16];
    __shared__ float corr;
    const int n = blockIdx.x;
    const int Dp = D + pd.p[0] + pd.p[1], Hp = H + pd.p[2] + pd.p[3], Wp = W + pd.p[4] + pd.p[5];
    const size_t plane = (size_t)D * H * W, per_n = (size_t)C * plane, pplane = (size_t)Dp * Hp * Wp;
    const size_t base = (size_t)n * per_n;
    double smg = 0.0, sgx = 0.0, sm = 0.0;
    for (size_t j = threadIdx.x; j < per_n; j += 1024) {
        const int c = (int)(j / plane);
        size_t r = j - (size_t)c * plane;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H), d = (int)(r / H);
        const float G = pad_adjoint(dyp + ((size_t)n * C + c) * pplane, d, h, w, D, H, W, pd.p, Hp, Wp);
        const float m = mask ? mask[base + j] : 1.0f;
        smg += (double)(m * G);
        if (g_xhat) sgx += (double)g_xhat[base + j];
        if (mask) sm += (double)m;
    }
    for (int off = 32; off > 0; off >>= 1) {
        smg += __shfl_down(smg, off, 64);
        sgx += __shfl_down(sgx, off, 64);
        sm += __shfl_down(sm, off, 64);
    }
    if (threadIdx.x % 64 == 0) {
        red[0][threadIdx.x / 64] = smg;
        red[1][threadIdx.x / 64] = sgx;
        red[2][threadIdx.x / 64] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, e = 0.0;
        for (int k = 0; k < 16; ++k) { a += red[0][k]; b += red[1][k]; e += red[2][k]; }
        corr = (float)((b - a) / (mask ? e : (double)per_n));
    }
    __syncthreads();
    const float cr = corr;
    for (size_t j = threadIdx.x; j < per_n; j += 1024) {
        const int c = (int)(j / plane);
        size_t r = j - (size_t)c * plane;
        const int w = (int)(r % W); r /= W;
        const int h = (int)(r % H), d = (int)(r / H);
        const float G = pad_adjoint(dyp + ((size_t)n * C + c) * pplane, d, h, w, D, H, W, pd.p, Hp, Wp);
        dy[base + j] = (mask ? mask[base + j] * G : G) + cr;
    }
}

}  // namespace

int cdl_dtau_per_sample(const float *partial, int N, int M, int R, size_t sN, size_t sM, size_t sR, float *dtau_n,
                        void *stream)
{
    if (!partial || !dtau_n || N <= 0 || M <= 0 || R <= 0) return CDL_EINVAL;
    k_dtau_per_sample<<<(unsigned)((N * M + 255) / 256), 256, 0, S(stream)>>>(partial, dtau_n, N, M, R, sN, sM, sR);
    CDL_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int cdl_dyp_split(const cdl_geom *g, float *q, const float *mask, float *dyp, int acc_add, int make_q, void *stream)
{
    if (!cdl_geom_ok(g) || !q || !dyp) return CDL_EINVAL;
    const size_t total = (size_t)g->N * g->C * g->D * g->H * g->W;
    k_dyp_split<<<(unsigned)((total + 255) / 256), 256, 0, S(stream)>>>(q, mask, dyp, total, acc_add, make_q);
    CDL_LAUNCH_CHECK();
    return 0;
}

int cdl_preprocess_bwd(const float *dyp, const float *g_xhat, const float *mask, float *dy, int N, int C, int D, int H,
                       int W, const int pads[6], void *stream)
{
    if (!dyp || !dy || !pads || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return CDL_EINVAL;
    Pads6 pd;
    const int ext[3] = {D, H, W};
    for (int i = 0; i < 6; ++i) {
        if (pads[i] < 0 || (pads[i] && pads[i] >= ext[i / 2])) return CDL_EINVAL;
        pd.p[i] = pads[i];
    }
    k_preprocess_bwd<<<N, 1024, 0, S(stream)>>>(dyp, g_xhat, mask, dy, C, D, H, W, pd);
    CDL_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
