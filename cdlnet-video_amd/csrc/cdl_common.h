// Shared helpers for the gfx950 kernels of libcdlnet_hip.so.
#pragma once
#include <atomic>
#include <type_traits>
#include <hip/hip_runtime.h>
#include "../../include/cdlnet_hip.h"

// ---- launch trace (cdl_options.hip): host code only, off by default --------------------
// Every launch site ends in CDL_LAUNCH_CHECK(), which -- while the trace is on -- appends one record: source file and
// line, the enclosing launcher with the values of its template arguments (__PRETTY_FUNCTION__), and the note that
// CDL_TRACE_NOTE left on this host thread since the previous launch (the plan's run-time variant values; the kernel's
// name where one launcher holds several launches).  Off, a launch pays one relaxed atomic load.
extern __attribute__((visibility("hidden"))) std::atomic<int> cdl_trace_state;   // (not part of the C ABI) 0: off; 1: log (cdl_trace); 2: CDL_TRACE_FILE; < 0: environment not read yet
void cdl_trace_launch(const char *file, int line, const char *func);
void cdl_trace_note(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
#define CDL_TRACE_NOTE(...)                                                               \
    do {                                                                                  \
        if (cdl_trace_state.load(std::memory_order_relaxed) != 0) cdl_trace_note(__VA_ARGS__); \
    } while (0)

#define CDL_LAUNCH_CHECK()                                   \
    do {                                                     \
        if (cdl_trace_state.load(std::memory_order_relaxed) != 0)          \
            cdl_trace_launch(__FILE__, __LINE__, __PRETTY_FUNCTION__);     \
        hipError_t e_ = hipGetLastError();                   \
        if (e_ != hipSuccess) return -(int)e_;               \
    } while (0)

// ---- host plumbing every launcher uses: the ABI's opaque stream, a status that ends the caller, the larger size ----
static inline hipStream_t S(void *s) { return (hipStream_t)s; }
static inline size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

#define CDL_TRY(expr)              \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_ != 0) return rc_;  \
    } while (0)

// sign(u) * relu(|u| - t): exactly the reference's x.sign()*relu(|x|-t) (model/net.py:11-14), including
// t < 0 (|u|-t > 0 everywhere, sign(0) = 0) and non-finite values: a NaN in u or t comes out as NaN (torch's
// sign and relu both keep it; fmaxf would turn it into 0 and hide a diverging net from the trainer's nan / inf
// backtracking, train.py:113-142), +-inf stays +-inf.
__device__ __forceinline__ float cdl_shrink(float u, float t)
{
    float m = fabsf(u) - t;
    m = m > 0.0f ? m : (m != m ? m : 0.0f);                          // relu that keeps NaN
    const float s = u > 0.0f ? 1.0f : (u < 0.0f ? -1.0f : (u != u ? u : 0.0f));      // sign that keeps NaN
    return s * m;
}

// ---- CSR proximal maps (reference model/net.py:229-262), shared by cdl_prox.hip and the analysis
// epilogues.  The reference's evaluation order is kept term by term and fma contraction is off: the
// maps are discontinuous for negative thresholds, a one-ulp re-association can move an output by |t|.
__device__ __forceinline__ float cdl_sgn(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

struct cdl_prox1 {           // intermediates of prox_CSR(u, zp, lam, gam)
    float s, ls, a, tg, m, z;
};

__device__ __forceinline__ cdl_prox1 cdl_prox_csr1(float u, float zp, float lam, float gam)
{
#pragma clang fp contract(off)
    cdl_prox1 p;
    p.s = cdl_sgn(zp);
    p.ls = lam * p.s;
    p.a = (u - zp) - p.ls;                                   // u - z_prev - lambd*sign(z_prev)
    p.tg = lam * gam;
    const float inner = cdl_shrink(p.a, p.tg);
    p.m = (inner + zp) + p.ls;
    p.z = cdl_shrink(p.m, lam);
    return p;
}

struct cdl_prox2 {           // intermediates of prox_CSR_f2(u, zp, za, lam, g1, g2)
    float sp, sa_, spa, sap, a, sa, t1, b, t2, m, z;
};

__device__ __forceinline__ cdl_prox2 cdl_prox_csr2(float u, float zp, float za, float lam, float g1, float g2)
{
#pragma clang fp contract(off)
    cdl_prox2 p;
    p.sp = cdl_sgn(zp);
    p.sa_ = cdl_sgn(za);
    p.spa = cdl_sgn(zp - za);
    p.sap = cdl_sgn(za - zp);
    const float l1 = lam * g1, l2 = lam * g2;
    const float ca = (zp + lam * p.sp) + l2 * p.spa;
    const float cb = (za + lam * p.sa_) + l1 * p.sap;
    p.a = u - ca;
    p.sa = cdl_sgn(p.a);
    p.t1 = g1 * lam;
    const float inner = cdl_shrink(p.a, p.t1);
    p.b = (inner - cb) + l1 * p.sa;
    p.t2 = g2 * lam;
    const float mid = cdl_shrink(p.b, p.t2);
    p.m = (mid + cb) - l1 * p.sa;
    p.z = cdl_shrink(p.m, lam);
    return p;
}

// d ST(x,t) / dx as autograd sees sign(x) * relu(|x| - t) (sign has zero gradient): the gate of the reverse pass
// (k_prox_bwd) and of the tangent below.
__device__ __forceinline__ bool cdl_st_dx(float x, float t) { return x != 0.0f && fabsf(x) - t > 0.0f; }

// Tangents of the two maps at the primal's intermediates (the pointwise pass of cdl_prox.hip): the
// maps are piecewise linear in (u, zp, za), so the derivative along (ud, zpd, zad) is a nest of gates.  Selects, not
// products with 0 / 1: a NaN in a dead branch stays there, and (x - zad) + zad is never formed.  No threshold enters a
// value.  The transposes are k_prox_bwd's: gu = Gm Ga g, gzp += Gm (1 - Ga) g; resp. gu = Gm Gb Ga g, gzp -= Gm Gb Ga g, gza += Gm (1 - Gb) g.
__device__ __forceinline__ float cdl_prox_csr1_tangent(const cdl_prox1 &p, float lam, float ud, float zpd)
{
    const bool Ga = cdl_st_dx(p.a, p.tg), Gm = cdl_st_dx(p.m, lam);
    return Gm ? (Ga ? ud : zpd) : 0.0f;
}

__device__ __forceinline__ float cdl_prox_csr2_tangent(const cdl_prox2 &p, float lam, float ud, float zpd, float zad)
{
#pragma clang fp contract(off)
    const bool Ga = cdl_st_dx(p.a, p.t1), Gb = cdl_st_dx(p.b, p.t2), Gm = cdl_st_dx(p.m, lam);
    return Gm ? (Gb ? (Ga ? ud - zpd : 0.0f) : zad) : 0.0f;
}

// Optional CSR epilogue of the analysis kernels: out = prox(u; zp[, za]) and, for training, u itself.
struct cdl_prox_args {
    const float *zp, *za, *lam, *g1, *g2;   // zp == nullptr: epilogue off
    float *u_out;                           // nullable
};

__device__ __forceinline__ float cdl_prox_apply(const cdl_prox_args &px, float u, size_t idx, int row)
{
    if (px.u_out) px.u_out[idx] = u;
    return px.za ? cdl_prox_csr2(u, px.zp[idx], px.za[idx], px.lam[row], px.g1[row], px.g2[row]).z
                 : cdl_prox_csr1(u, px.zp[idx], px.lam[row], px.g1[row]).z;
}

// Optional noise-level map of the shrinkage epilogues: thr = tau[n,m] + cmap[n,pix] * tslope[m],
// tau then holding t[k,0,m].  The product is rounded before the sum (contraction off), as torch's broadcast
// `t0 + c * t1` does (model/net.py:83), so the thresholds are the reference's bit for bit.
struct cdl_map_args {
    const float *cmap;      // (N, code pixels); nullptr: no map
    const float *tslope;    // (M); with the CSR epilogue (3, M): the slopes of lam, gam1, gam2
};

__device__ __forceinline__ float cdl_map_threshold(float t0, float c, float slope)
{
#pragma clang fp contract(off)
    const float prod = c * slope;
    return t0 + prod;
}

// The CSR epilogue under a noise-level map: all three threshold families follow the map, px.lam /
// g1 / g2 holding the constant parts per (sample, channel) row and mp.tslope the 3*M slopes of lam, gam1, gam2 (the third
// plane unread without z_after).  cm: the map at this element's pixel.
__device__ __forceinline__ float cdl_prox_apply_map(const cdl_prox_args &px, const cdl_map_args &mp, float u, size_t idx,
                                                    int row, int m, int M, float cm)
{
    if (px.u_out) px.u_out[idx] = u;
    const float lam = cdl_map_threshold(px.lam[row], cm, mp.tslope[m]);
    const float g1 = cdl_map_threshold(px.g1[row], cm, mp.tslope[M + m]);
    return px.za ? cdl_prox_csr2(u, px.zp[idx], px.za[idx], lam, g1, cdl_map_threshold(px.g2[row], cm, mp.tslope[2 * M + m])).z
                 : cdl_prox_csr1(u, px.zp[idx], lam, g1).z;
}

__host__ __device__ __forceinline__ int cdl_floordiv(int a, int b)
{
    int q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// ---- timing-ablation switches: compiled OUT of the product library ------------------------------------------
// The kernels carry run-time switches that turn parts of them off for timing experiments (results are then wrong).
// They exist only in the probe build (`make libcdlnet_hip_ablate.so`, -DCDL_ABLATE, loaded by the tools through
// CDLNET_HIP_LIB); in libcdlnet_hip.so CDL_DBG() is the constant 0, the kernels' parameter blocks have no debug
// field, and CDL_FUSED_DEBUG / CDL_DENSE_DEBUG are not read.
#ifdef CDL_ABLATE
#define CDL_DBG(flags, bit) (((flags) & (bit)) != 0)
#define CDL_DBG_FIELD(decl) decl
#define CDL_DBG_COMMA(x) , x
#else
#define CDL_DBG(flags, bit) (false)
#define CDL_DBG_FIELD(decl)
#define CDL_DBG_COMMA(x)
#endif

// ---- process-wide switches and per-device bookkeeping (cdl_options.hip) ---------------------------------
struct cdl_options {
    int mfma_analysis, mfma_synthesis, mfma_wgrad, mfma_dense;   // 0: use the fp32 VALU kernels instead (CDL_MFMA_*=0)
    int no_tiled, no_pipelined_synthesis;                        // CDL_NO_TILED, CDL_NO_PIPELINED_SYNTHESIS
    int fused_snake;                                             // CDL_FUSED_SNAKE=0: no alternating tile direction
    int fused_grid;                                              // CDL_FUSED_GRID=n: fewer persistent workgroups (probes)
    int fused_da;                                                // CDL_FUSED_DA=0: dA_k by k_wgrad2d instead of inside the reverse stage
    int fusedg_bwd_prec;                                         // CDL_FUSEDG_PREC=0|2: forces the arithmetic of the tile kernel's sweeps (experiments)
    int fusedg_strip;                                            // CDL_FUSEDG_STRIP=1: cdl_stripg.hip instead of the tile kernel k_stage_g
    int scalar_assemble;                                         // CDL_SCALAR_ASSEMBLE=1: the one-pixel-per-thread patch assemble (tests)
    int fused_debug, dense_debug;                                // -DCDL_ABLATE builds only (always 0 in the product)
    const char *trace_file;                                      // CDL_TRACE_FILE=path: each distinct launch record appended once (nullptr: off)
};
const cdl_options &cdl_opts();                                   // snapshot of the environment, read once
bool cdl_exact_fp32();                                           // this host thread asked for the fp32 VALU tier (cdl_set_exact_fp32)
int cdl_current_device();
int cdl_cu_count();                                              // compute units of the CURRENT device
int cdl_ensure_dynamic_lds(const void *kernel, int bytes);       // per (device, kernel): keep the dynamic-LDS limit >= bytes

// The alignment contract (include/cdlnet_hip.h): a caller's pointer needs only the alignment of its element type, so a
// launcher selects a 16-byte form only after this test of EVERY pointer that form vector-accesses (NULL counts as aligned).
static inline bool cdl_aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr)
{
    return ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b) | reinterpret_cast<size_t>(c) |
             reinterpret_cast<size_t>(d)) & 15) == 0;
}

// May a patch assemble use its 16-byte form (four pixels per thread)?  The row length AND every thin pointer decide;
// CDL_SCALAR_ASSEMBLE=1 forces the one-pixel form (tests).
static inline bool cdl_assemble16(int W, const float *out, const float *mask, const float *sub, const float *acc)
{
    return (W & 3) == 0 && cdl_aligned16(out, mask, sub, acc) && !cdl_opts().scalar_assemble;
}

// Persistent workgroups of the fused stage kernels: one per CU of the current device, striding over the work items;
// CDL_FUSED_GRID=n caps the count (probes).
static inline unsigned cdl_persistent_grid(size_t work_items)
{
    size_t cus = (size_t)cdl_cu_count();
    const int cap = cdl_opts().fused_grid;
    if (cap > 0 && (size_t)cap < cus) cus = (size_t)cap;
    return (unsigned)(work_items < cus ? work_items : cus);
}

// One batch of a sweep's K (first bank, second bank) weight pairs for a k_prep_* launch, pairs k0 .. k0 + nb - 1 (nb is
// returned).  The shifted bank is index shift2 -- forward (1): (w1[k], w2[k+1 mod K]); reverse (0): (w1[k+1 mod K], w2[k]).
template <class Batch>
static inline int cdl_pair_batch(Batch *b, const float *const *w1, const float *const *w2, int K, int shift2, int k0)
{
    constexpr int cap = (int)(sizeof(b->wA) / sizeof(b->wA[0]));
    const int nb = K - k0 < cap ? K - k0 : cap;
    *b = Batch{};
    for (int i = 0; i < nb; ++i) {
        const int k = k0 + i;
        b->wA[i] = shift2 == 0 ? w1[(k + 1) % K] : w1[k];
        b->wB[i] = shift2 == 0 ? w2[k] : w2[(k + 1) % K];
    }
    return nb;
}

static inline bool cdl_geom_ok(const cdl_geom *g)
{
    if (!g) return false;
    if (g->N <= 0 || g->C <= 0 || g->M <= 0) return false;
    if (g->D <= 0 || g->H <= 0 || g->W <= 0) return false;
    if (g->Pd <= 0 || g->Ph <= 0 || g->Pw <= 0) return false;
    if (g->sd <= 0 || g->sh <= 0 || g->sw <= 0) return false;
    if (g->pd < 0 || g->ph < 0 || g->pw < 0) return false;
    if (g->D % g->sd || g->H % g->sh || g->W % g->sw) return false;
    // the transpose must map Z*s back onto X exactly (output_padding = s-1): 2p + s - P >= 0 .. s-1
    return true;
}

// Strides of a broadcast threshold (cdl_bcast): 0 on a broadcast axis, else the dense stride of a contiguous tensor whose
// other axes are full or 1.  The spatial axes are broadcast together (p == 0) or all present (p == 1).
static inline bool cdl_bcast_ok(const cdl_bcast *s, int M, size_t per_m)
{
    if (!s || (s->p != 0 && s->p != 1)) return false;
    const long long dm = s->p ? (long long)per_m : 1;
    if (s->m != 0 && s->m != dm) return false;
    const long long dn = s->m ? dm * M : dm;
    return s->n == 0 || s->n == dn;
}

// ---- the filter planes of the sparse matrix-core tier (cdl_analysis_mfma.hip, cdl_synth_mfma.hip, cdl_wgrad_mfma.hip) ----
// One gate and one ladder for the three files: a new plane is added here, and cdl_mfma_wgrad_takes agrees with the other
// two by construction.  Equal stride 1 or 2 in the plane, odd square planes up to 9 x 9 or the 9 x 5 planes of the shipped
// 9 x 9 x 5 net, "same" padding.
static inline bool cdl_mfma_plane_ok(const cdl_geom *g)
{
    if (g->sw != g->sh || (g->sw != 1 && g->sw != 2)) return false;
    if (g->Pw != 3 && g->Pw != 5 && g->Pw != 7 && g->Pw != 9) return false;
    if (g->Ph != g->Pw && !(g->Ph == 9 && g->Pw == 5)) return false;
    return g->pw == g->Pw / 2 && g->ph == g->Ph / 2;
}

// fn(PH, PW, SW) as integral constants for the ten planes of the gate (the idiom of cdl_fused2d.hip's dispatch_mt_prec);
// CDL_EUNSUPPORTED for any other plane
template <class F>
static inline int cdl_mfma_dispatch_plane(const cdl_geom *g, F &&fn)
{
    using std::integral_constant;
    auto by_stride = [&](auto ph, auto pw) {
        return g->sw == 1   ? fn(ph, pw, integral_constant<int, 1>{})
               : g->sw == 2 ? fn(ph, pw, integral_constant<int, 2>{})
                            : CDL_EUNSUPPORTED;
    };
    if (g->Ph == 9 && g->Pw == 5) return by_stride(integral_constant<int, 9>{}, integral_constant<int, 5>{});
    if (g->Ph != g->Pw) return CDL_EUNSUPPORTED;
    if (g->Pw == 3) return by_stride(integral_constant<int, 3>{}, integral_constant<int, 3>{});
    if (g->Pw == 5) return by_stride(integral_constant<int, 5>{}, integral_constant<int, 5>{});
    if (g->Pw == 7) return by_stride(integral_constant<int, 7>{}, integral_constant<int, 7>{});
    if (g->Pw == 9) return by_stride(integral_constant<int, 9>{}, integral_constant<int, 9>{});
    return CDL_EUNSUPPORTED;
}

// ---- the four tiers behind cdl_analysis*, cdl_synthesis and cdl_wgrad*, in the order cdl_operators.hip walks them -----
// One face per tier and operator: a launcher that returns CDL_EUNSUPPORTED when it does not serve the call, and
// ..._ws_floats(g), the floats that launcher may use (0: none, or no plan; no such function: no workspace).  ..._takes(g):
// the tier's plan serves the geometry -- its launcher can still refuse a short or misaligned workspace.
// 1. dense matrix-core tier (cdl_dense_mfma.hip): many-channel unit-stride convolution (C >= 16 on both sides), analysis
// (transpose = 0) or synthesis role
bool cdl_dense_takes(const cdl_geom *g, int transpose);
size_t cdl_dense_ws_floats(const cdl_geom *g, int transpose);
int cdl_dense_conv(const cdl_geom *g, int transpose, const float *x, const float *in_gate, const float *w,
                   float alpha, const float *add, const float *add_gate, const float *mask, const float *sub,
                   const float *tau, int relu, const float *out_gate, float *out, float *ws, size_t ws_floats,
                   void *stream);
bool cdl_dense_wgrad_takes(const cdl_geom *g);
size_t cdl_dense_wgrad_ws_floats(const cdl_geom *g);
int cdl_dense_wgrad(const cdl_geom *g, const float *F, const float *gate, const float *x, float alpha, float *dw,
                    float *ws, size_t ws_floats, void *stream);
// the VGG16 layers of the perceptual loss (cdl_vgg.hip) on the dense tier: forms of cdl_dense_vgg
enum { CDL_VGG_PLAIN = 0, CDL_VGG_BIAS = 1, CDL_VGG_POOL = 2, CDL_VGG_DIFF = 3, CDL_VGG_UNPOOL = 4 };
size_t cdl_dense_vgg_workgroups(const cdl_geom *g, int transpose);
int cdl_dense_vgg(const cdl_geom *g, int transpose, int form, const float *x, const float *w, const float *bias,
                  const float *out_gate, float *out, unsigned char *pool_arg, const unsigned char *unpool_arg,
                  const float *fy, float *seed_x, float *seed_y, double *partial, float *ws, size_t ws_floats,
                  void *stream);
// the dense switch as cdl_residual.hip reads it (cdl_operators.hip): CDL_MFMA_DENSE and CDL_NO_TILED, NOT the exact-fp32
// request (DESIGN.md section 37 has what follows from that)
bool cdl_dense_switch_on();
// 2. sparse matrix-core tier (cdl_analysis_mfma.hip, cdl_synth_mfma.hip, cdl_wgrad_mfma.hip)
int cdl_mfma_analysis(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                      const float *gate, const float *tau, float *out, const cdl_prox_args &px, float *ws,
                      size_t ws_floats, void *stream, const cdl_map_args &mp = cdl_map_args{nullptr, nullptr});
size_t cdl_mfma_analysis_ws_floats(const cdl_geom *g);
size_t cdl_mfma_analysis_rev_ws_floats(const cdl_geom *g);
int cdl_mfma_analysis_rev(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                          const float *zsup, const float *c, float *dt0, float *dt1, float *out, float *ws,
                          size_t ws_floats, void *stream, float *dtau_n = nullptr, const float *cmap = nullptr);
int cdl_mfma_synthesis(const cdl_geom *g, const float *z, const float *gate, const float *w, float alpha,
                       const float *mask, const float *sub, float *out, float *ws, size_t ws_floats, void *stream);
size_t cdl_mfma_synthesis_ws_floats(const cdl_geom *g);
// dw = alpha * F (x) x for one operand set, or for two ungated ones of the same geometry (dA_k and dB_k of one iteration) in
// ONE launch + ONE fold.  gate: support gate of a single F (nullable).  rsc != 0: the fat operands F are in the strip
// kernel's row-strip channel-major layout (cdl_strip.hip, CDL_LAY_RSC; ungated).  cdl_mfma_wgrad_takes: this kernel (and not
// a VALU fallback, which reads the reference layout only) is what the fused generic sweeps count on; it reads CDL_MFMA_WGRAD
// and its own plan, not CDL_NO_TILED, the exact-fp32 request or the dense tier ahead of it.
struct cdl_wgrad_op {
    const float *F, *x;
    float alpha;
    float *dw;
};
int cdl_mfma_wgrad(const cdl_geom *g, const cdl_wgrad_op *ops, int nops, const float *gate, int rsc, float *ws,
                   size_t ws_floats, void *stream);
size_t cdl_mfma_wgrad_ws_floats(const cdl_geom *g);
bool cdl_mfma_wgrad_takes(const cdl_geom *g);
// 3. register-tiled VALU tier (cdl_generic_tiled.hip)
int cdl_tiled_analysis(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                       const float *gate, const float *tau, float *out, const cdl_prox_args &px, void *stream,
                       const cdl_map_args &mp = cdl_map_args{nullptr, nullptr});
int cdl_tiled_synthesis(const cdl_geom *g, const float *z, const float *gate, const float *w, float alpha,
                        const float *mask, const float *sub, float *out, float *ws, size_t ws_floats,
                        void *stream);
size_t cdl_tiled_synthesis_ws_floats(const cdl_geom *g);
int cdl_tiled_wgrad(const cdl_geom *g, const float *z, const float *gate, const float *x, float alpha,
                    float *dw, float *workspace, size_t workspace_floats, void *stream);
size_t cdl_tiled_wgrad_ws_floats(const cdl_geom *g);
// 4. plain VALU tier (cdl_generic.hip): no workspace
int cdl_plain_analysis(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                       const float *gate, const float *tau, float *out, const cdl_prox_args &px, void *stream,
                       const cdl_map_args &mp);
int cdl_plain_synthesis(const cdl_geom *g, const float *z, const float *gate, const float *w, float alpha,
                        const float *mask, const float *sub, float *out, void *stream);
int cdl_plain_wgrad(const cdl_geom *g, const float *z, const float *gate, const float *x, float alpha, float *dw, void *stream);
// per-sample threshold gradients from a sweep's partial sums (cdl_datagrad.hip):
// dtau_n[n,m] = sum_{j<R} partial[n sN + m sM + j sR], j in order
int cdl_dtau_per_sample(const float *partial, int N, int M, int R, size_t sN, size_t sM, size_t sR, float *dtau_n,
                        void *stream);
