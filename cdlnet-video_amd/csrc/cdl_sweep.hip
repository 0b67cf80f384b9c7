// Whole forward / reverse sweeps of the shape-generic loop from one C call: the same launches that
// cdl_analysis / cdl_synthesis / cdl_wgrad / cdl_tau_grad / cdl_prox_csr* make, enqueued back to back.
// Single-frame inference (the frame-recurrent CSR drivers, reference analyzemri.py:87-182) and crop-sized
// training (traincsr.py) run launches of a few microseconds, where a host round trip per launch
// (interpreter + ctypes, ~30 us) is what bounds the step.
#include "cdl_common.h"

namespace {

struct Scratch {                 // what every operator of a sweep gets behind its own arguments
    float *p;
    size_t floats;
    void *stream;
};

// The forward-order loop of the primal, tangent and CSR-tangent sweeps:
//   z_1 = step_0(thin0),   r_k = mask B_k z_k - thin0,   z_{k+1} = step_k(z_k - A_k r_k),   out = B_0 z_K.
// step(k, x, alpha, zin) -> rc is the analysis-type launch of iteration k: it writes z[k] from zin + alpha A_k x.
// (cdl_forward_order_sweep of cdl_fused_sweep.h walks fragment tables stage-then-assemble: another shape of loop.)
template <class Step>
int forward_order_loop(const cdl_geom *g, int K, const float *thin0, const float *mask, const float *const *wB,
                       float *const *z, float *const *r, float *out, const Scratch &sc, Step step)
{
    for (int k = 0; k < K; ++k) {
        if (k > 0)
            CDL_TRY(cdl_synthesis(g, z[k - 1], nullptr, wB[k], 1.0f, mask, thin0, r[k - 1], sc.p, sc.floats, sc.stream));
        CDL_TRY(step(k, k ? r[k - 1] : thin0, k ? -1.0f : 1.0f, k ? z[k - 1] : nullptr));
    }
    return cdl_synthesis(g, z[K - 1], nullptr, wB[0], 1.0f, nullptr, nullptr, out, sc.p, sc.floats, sc.stream);
}

// Without an image gradient a reverse sweep starts from dL/dz_K alone: dB_0 = 0, gk = g_z.
int seed_from_code_gradient(const cdl_geom *g, const float *g_z, float *dB0, float *gk, void *stream)
{
    const size_t code = (size_t)g->N * g->M * (g->D / g->sd) * (g->H / g->sh) * (g->W / g->sw);
    const size_t flen = (size_t)g->M * g->C * g->Pd * g->Ph * g->Pw;
    hipError_t e = hipMemsetAsync(dB0, 0, flen * sizeof(float), S(stream));
    if (e != hipSuccess) return -(int)e;
    e = hipMemcpyAsync(gk, g_z, code * sizeof(float), hipMemcpyDeviceToDevice, S(stream));
    return e != hipSuccess ? -(int)e : 0;
}

// q_k of iteration k >= 1 from gk = du_k: q = -mask A_k^T du_k.  With data gradients S = A_k^T du_k goes out unmasked,
// dyp (= at k = K-1, +=) S, then q = -mask S in place.
int residual_gradient(const cdl_geom *g, int k, int K, const float *gk, const float *wAk, const float *mask, float *q,
                      float *dyp, const Scratch &sc)
{
    if (!dyp) return cdl_synthesis(g, gk, nullptr, wAk, -1.0f, mask, nullptr, q, sc.p, sc.floats, sc.stream);
    CDL_TRY(cdl_synthesis(g, gk, nullptr, wAk, 1.0f, nullptr, nullptr, q, sc.p, sc.floats, sc.stream));
    return cdl_dyp_split(g, q, mask, dyp, k < K - 1, 1, sc.stream);
}

// Iteration 0, where u_0 = A_0 yp: dA_0 from gk = du_0, and dyp += A_0^T du_0.
int first_iteration_gradients(const cdl_geom *g, int K, const float *gk, const float *yp, const float *wA0, float *dA0,
                              float *q, float *dyp, const Scratch &sc)
{
    CDL_TRY(cdl_wgrad(g, gk, nullptr, yp, 1.0f, dA0, sc.p, sc.floats, sc.stream));
    if (!dyp) return 0;
    CDL_TRY(cdl_synthesis(g, gk, nullptr, wA0, 1.0f, nullptr, nullptr, q, sc.p, sc.floats, sc.stream));
    return cdl_dyp_split(g, q, nullptr, dyp, K > 1, 0, sc.stream);
}

// Reverse sweep of the plain loop (no neighbour codes), primal or tangent.  The analysis that produces dL/dz_k also gates
// it by the support of z_k and reduces the threshold gradients of iteration k (cdl_analysis_rev) -- a separate gate /
// threshold pass re-read and re-wrote the tensor the analysis had just written (3 of the sweep's fat passes per iteration).
//   zgate[k]: the code whose support gates iteration k; z / r / yp: the operands of the filter gradients (the primal's are
//       its own codes: zgate = z; the tangent's are zd / rd / vp under the primal's gates).
//   dt + k * dt_stride: the (2, M) threshold sums of iteration k (stride 0: a scratch nobody reads).
//   c / dtau / dyp / cmap / tslope / dcmap (nullable): the noise levels and the data gradients, as in cdl_ista_backward.
int plain_reverse_sweep(const cdl_geom *g, int K, const float *yp, const float *mask, const float *c,
                        const float *const *wA, const float *const *wB, const float *const *zgate, const float *const *z,
                        const float *const *r, const float *g_xp, const float *g_z, float *const *dA, float *const *dB,
                        float *dt, size_t dt_stride, float *gbuf0, float *gbuf1, float *q, float *dyp, float *dtau,
                        const float *cmap, const float *tslope, float *dcmap, const Scratch &sc)
{
    const size_t NM = (size_t)g->N * g->M, M = g->M;
    float *gk = gbuf0, *other = gbuf1;
    float *dtk = dt + (size_t)(K - 1) * dt_stride, *dtauk = dtau ? dtau + (K - 1) * NM : nullptr;
    if (g_xp) {                  // gk = [z_K != 0] (B_0^T g_xp (+ g_z)), with the threshold sums of iteration K-1
        CDL_TRY(cdl_wgrad(g, z[K - 1], nullptr, g_xp, 1.0f, dB[0], sc.p, sc.floats, sc.stream));
        CDL_TRY(cdl_analysis_rev(g, g_xp, wB[0], 1.0f, g_z, zgate[K - 1], c, dtk, dtk + M, dtauk, gk, sc.p, sc.floats, cmap,
                                 sc.stream));
    } else {                     // the same from g_z: gated in place
        CDL_TRY(seed_from_code_gradient(g, g_z, dB[0], gk, sc.stream));
        CDL_TRY(cdl_tau_grad_gate(g, gk, zgate[K - 1], c, dtk, dtk + M, dtauk, sc.p, cmap, sc.stream));
    }
    for (int k = K - 1; k >= 0; --k) {                          // gk = du_k, gated; dt_k written
        if (dcmap)               // dcmap (= at k = K-1, +=) sum_m t[k,1,m] (-sign(z_{k+1}) du_k)
            CDL_TRY(cdl_sigma_grad(g, gk, zgate[k], tslope + (size_t)k * M, dcmap, k < K - 1, sc.stream));
        if (k == 0) break;
        CDL_TRY(residual_gradient(g, k, K, gk, wA[k], mask, q, dyp, sc));
        CDL_TRY(cdl_wgrad_pair(g, gk, r[k - 1], -1.0f, dA[k], z[k - 1], q, 1.0f, dB[k], sc.p, sc.floats, sc.stream));
        dtk = dt + (size_t)(k - 1) * dt_stride;                  // dL/dz_{k-1}, gated, with iteration k-1's threshold sums
        CDL_TRY(cdl_analysis_rev(g, q, wB[k], 1.0f, gk, zgate[k - 1], c, dtk, dtk + M, dtau ? dtau + (k - 1) * NM : nullptr,
                                 other, sc.p, sc.floats, cmap, sc.stream));
        float *t = gk;
        gk = other;
        other = t;
    }
    return first_iteration_gradients(g, K, gk, yp, wA[0], dA[0], q, dyp, sc);
}

// Reverse sweep of the CSR loop: cdl_prox_csr_bwd turns gk = dL/dz_{k+1} into dL/du_k in place and accumulates the
// neighbour-code and threshold gradients (and, with a map, every iteration's map gradient into dcmap).
int csr_reverse_sweep(const cdl_geom *g, int K, const float *yp, const float *mask, const float *c, const float *z_prev,
                      const float *z_after, const float *lam, const float *gam1, const float *gam2,
                      const float *const *wA, const float *const *wB, const float *const *z, const float *const *r,
                      const float *const *u, const float *g_xp, const float *g_z, float *const *dA, float *const *dB,
                      float *dt, float *dg1, float *dg2, float *gz_prev, float *gz_after, float *gbuf0, float *gbuf1,
                      float *q, float *dyp, float *dtau, const float *cmap, const float *tslope, float *dcmap,
                      const Scratch &sc)
{
    const size_t NM = (size_t)g->N * g->M, M = g->M;
    float *gk = gbuf0, *other = gbuf1;
    if (dcmap) {
        const size_t grid = (size_t)g->N * (g->D / g->sd) * (g->H / g->sh) * (g->W / g->sw);
        const hipError_t e = hipMemsetAsync(dcmap, 0, grid * sizeof(float), S(sc.stream));
        if (e != hipSuccess) return -(int)e;
    }
    if (g_xp) {
        CDL_TRY(cdl_wgrad(g, z[K - 1], nullptr, g_xp, 1.0f, dB[0], sc.p, sc.floats, sc.stream));
        CDL_TRY(cdl_analysis(g, g_xp, wB[0], 1.0f, g_z, nullptr, nullptr, gk, sc.p, sc.floats, nullptr, nullptr,
                             sc.stream));                       // B_0^T g_xp (+ g_z)
    } else
        CDL_TRY(seed_from_code_gradient(g, g_z, dB[0], gk, sc.stream));
    for (int k = K - 1; k >= 0; --k) {
        CDL_TRY(cdl_prox_csr_bwd(g, gk, u[k], z_prev, z_after, lam + k * NM, gam1 + k * NM, gam2 ? gam2 + k * NM : nullptr,
                                 c, gk, gz_prev, gz_after, dt + k * 2 * M, dg1 + k * 2 * M, dg2 ? dg2 + k * 2 * M : nullptr,
                                 sc.p, sc.floats, cmap, cmap ? tslope + (size_t)k * 3 * M : nullptr, dcmap,
                                 dtau ? dtau + (size_t)k * 3 * NM : nullptr, sc.stream));
        if (k == 0) break;
        CDL_TRY(residual_gradient(g, k, K, gk, wA[k], mask, q, dyp, sc));
        CDL_TRY(cdl_wgrad_pair(g, gk, r[k - 1], -1.0f, dA[k], z[k - 1], q, 1.0f, dB[k], sc.p, sc.floats, sc.stream));
        CDL_TRY(cdl_analysis(g, q, wB[k], 1.0f, gk, nullptr, nullptr, other, sc.p, sc.floats, nullptr, nullptr, sc.stream));
        float *t = gk;
        gk = other;
        other = t;
    }
    return first_iteration_gradients(g, K, gk, yp, wA[0], dA[0], q, dyp, sc);
}

}  // namespace

extern "C" {

size_t cdl_ista_scratch_floats(const cdl_geom *g)
{
    if (!cdl_geom_ok(g)) return 0;
    size_t n = (size_t)2 * CDL_TAU_SPLITS * g->N * g->M;         // cdl_tau_grad (with a map: two partials per split)
    n = max_sz(n, cdl_wgrad_workspace_floats(g));
    n = max_sz(n, cdl_synthesis_workspace_floats(g));
    n = max_sz(n, cdl_prox_csr_scratch_floats(g));
    n = max_sz(n, cdl_analysis_workspace_floats(g));
    n = max_sz(n, cdl_analysis_rev_workspace_floats(g));
    return n;
}

int cdl_ista_forward(const cdl_geom *g, int K, const float *yp, const float *mask, const float *tau,
                     const float *z_prev, const float *z_after, const float *gam1, const float *gam2,
                     const float *const *wA, const float *const *wB, float *const *z, float *const *r,
                     float *const *u, float *xp, float *scratch, size_t scratch_floats, const float *cmap,
                     const float *tslope, void *stream)
{
    if (!cdl_geom_ok(g) || K < 1 || !yp || !tau || !wA || !wB || !z || !xp || (K > 1 && !r)) return CDL_EINVAL;
    if (cmap && !tslope) return CDL_EINVAL;                          // with z_prev: the (K, 3, M) slopes of lam, gam1, gam2
    if (z_prev ? (!gam1 || (z_after && !gam2)) : (z_after || u)) return CDL_EINVAL;
    const size_t NM = (size_t)g->N * g->M;
    const Scratch sc{scratch, scratch_floats, stream};
    return forward_order_loop(g, K, yp, mask, wB, z, r, xp, sc, [&](int k, const float *x, float alpha, const float *zin) {
        if (z_prev)
            return cdl_analysis_prox(g, x, wA[k], alpha, zin, z_prev, z_after, tau + k * NM, gam1 + k * NM,
                                     gam2 ? gam2 + k * NM : nullptr, u ? u[k] : nullptr, z[k], scratch, scratch_floats,
                                     cmap, cmap ? tslope + (size_t)k * 3 * g->M : nullptr, stream);
        return cdl_analysis(g, x, wA[k], alpha, zin, nullptr, tau + k * NM, z[k], scratch, scratch_floats, cmap,
                            cmap ? tslope + (size_t)k * g->M : nullptr, stream);
    });
}

int cdl_ista_backward(const cdl_geom *g, int K, const float *yp, const float *mask, const float *c,
                      const float *z_prev, const float *z_after, const float *lam, const float *gam1,
                      const float *gam2, const float *const *wA, const float *const *wB,
                      const float *const *z, const float *const *r, const float *const *u, const float *g_xp,
                      const float *g_z, float *const *dA, float *const *dB, float *dt, float *dg1, float *dg2,
                      float *gz_prev, float *gz_after, float *gbuf0, float *gbuf1, float *q, float *scratch,
                      size_t scratch_floats, float *dyp, float *dtau, const float *cmap, const float *tslope,
                      float *dcmap, void *stream)
{
    if (!cdl_geom_ok(g) || K < 1 || !yp || !wA || !wB || !z || !dA || !dB || !dt || !gbuf0 || !gbuf1 || !q ||
        !scratch || (K > 1 && !r))
        return CDL_EINVAL;
    if (!g_xp && !g_z) return CDL_EINVAL;
    if (z_prev ? (!u || !lam || !gam1 || !dg1 || (z_after && (!gam2 || !dg2))) : (z_after != nullptr)) return CDL_EINVAL;
    if (scratch_floats < cdl_ista_scratch_floats(g)) return CDL_EINVAL;
    if (cmap ? (c || dtau || (dcmap && !tslope)) : (dcmap != nullptr)) return CDL_EINVAL;   // a map replaces c; dcmap where dtau was
    if (z_prev && cmap && !tslope) return CDL_EINVAL;                  // the CSR maps read their thresholds' slopes
    const Scratch sc{scratch, scratch_floats, stream};
    if (!z_prev)
        return plain_reverse_sweep(g, K, yp, mask, c, wA, wB, z, z, r, g_xp, g_z, dA, dB, dt, (size_t)2 * g->M, gbuf0, gbuf1,
                                   q, dyp, dtau, cmap, tslope, dcmap, sc);
    return csr_reverse_sweep(g, K, yp, mask, c, z_prev, z_after, lam, gam1, gam2, wA, wB, z, r, u, g_xp, g_z, dA, dB, dt,
                             dg1, dg2, gz_prev, gz_after, gbuf0, gbuf1, q, dyp, dtau, cmap, tslope, dcmap, sc);
}

/* Forward-mode tangent of the plain loop at fixed supports: with G_k = [z_{k+1} != 0] of the primal,
 *   zd_1 = G_0 (A_0 vp),   rd_k = mask B_k zd_k - vp,   zd_{k+1} = G_k (zd_k - A_k rd_k),   xdp = B_0 zd_K.
 * The launches of cdl_ista_forward with the shrinkage replaced by the gate: cdl_analysis gates its base only, so the
 * gated step is cdl_analysis_rev (out = [zsup != 0] (zin + alpha A x)), whose threshold sums nobody reads (dt_scratch,
 * 2*M floats).  zgate[k] = z_{k+1} of the primal; zd / rd: K / K-1 buffers (ping-pong tables are fine when not kept). */
int cdl_tangent_forward(const cdl_geom *g, int K, const float *vp, const float *mask, const float *const *wA,
                        const float *const *wB, const float *const *zgate, float *const *zd, float *const *rd, float *xdp,
                        float *dt_scratch, float *scratch, size_t scratch_floats, void *stream)
{
    if (!cdl_geom_ok(g) || K < 1 || !vp || !wA || !wB || !zgate || !zd || !xdp || !dt_scratch || !scratch || (K > 1 && !rd))
        return CDL_EINVAL;
    if (scratch_floats < cdl_ista_scratch_floats(g)) return CDL_EINVAL;
    const Scratch sc{scratch, scratch_floats, stream};
    return forward_order_loop(g, K, vp, mask, wB, zd, rd, xdp, sc, [&](int k, const float *x, float alpha, const float *zin) {
        return cdl_analysis_rev(g, x, wA[k], alpha, zin, zgate[k], nullptr, dt_scratch, dt_scratch + g->M, nullptr, zd[k],
                                scratch, scratch_floats, nullptr, stream);
    });
}

/* Reverse sweep of the tangent net (linear in vp with the gates fixed): the plain reverse sweep of cdl_ista_backward with
 * the supports taken from the primal codes zgate and the operands from the tangent sweep (zd, rd, vp); no threshold
 * gradient leaves it (dt_scratch, 2*M floats) and no data gradient is formed.  g_xp = dL/dxdp, g_zd (nullable) = dL/dzd_K. */
int cdl_tangent_backward(const cdl_geom *g, int K, const float *vp, const float *mask, const float *const *wA,
                         const float *const *wB, const float *const *zgate, const float *const *zd,
                         const float *const *rd, const float *g_xp, const float *g_zd, float *const *dA, float *const *dB,
                         float *gbuf0, float *gbuf1, float *q, float *dt_scratch, float *scratch, size_t scratch_floats,
                         void *stream)
{
    if (!cdl_geom_ok(g) || K < 1 || !vp || !wA || !wB || !zgate || !zd || !g_xp || !dA || !dB || !gbuf0 || !gbuf1 || !q ||
        !dt_scratch || !scratch || (K > 1 && !rd))
        return CDL_EINVAL;
    if (scratch_floats < cdl_ista_scratch_floats(g)) return CDL_EINVAL;
    return plain_reverse_sweep(g, K, vp, mask, nullptr, wA, wB, zgate, zd, rd, g_xp, g_zd, dA, dB, dt_scratch, 0, gbuf0,
                               gbuf1, q, nullptr, nullptr, nullptr, nullptr, nullptr, Scratch{scratch, scratch_floats, stream});
}

/* Forward-mode tangent of the CSR loop at the primal's gates: the proximal maps are piecewise linear
 * in (u, z_prev, z_after), so with u[k] = u_k of the primal (what cdl_ista_forward kept) and Jprox_k the gate nest of
 * cdl_prox_csr1_tangent / cdl_prox_csr2_tangent read off (u_k, z_prev, z_after, lam_k, gam*_k),
 *   ud_0 = A_0 vp,   rd_k = mask B_k zd_k - vp,   ud_k = zd_k - A_k rd_k,   zd_{k+1} = Jprox_k(ud_k; zd_prev, zd_after),
 *   xdp = B_0 zd_K.
 * Per iteration cdl_synthesis and cdl_analysis_prox_tangent (the analysis, then the pointwise tangent in place).  zd_prev /
 * zd_after (nullable): the neighbours' tangents, NULL = a constant neighbour.  zd: K code buffers, rd: K-1 thin ones
 * (consecutive entries differ; two each suffice when nothing is kept).  Its reverse sweep is cdl_ista_backward's CSR branch
 * with yp -> vp, z -> zd, r -> rd, the primal's u / lam / gam*, c = NULL and the threshold outputs discarded. */
int cdl_csr_tangent_forward(const cdl_geom *g, int K, const float *vp, const float *mask, const float *z_prev,
                            const float *z_after, const float *lam, const float *gam1, const float *gam2,
                            const float *zd_prev, const float *zd_after, const float *const *wA, const float *const *wB,
                            const float *const *u, float *const *zd, float *const *rd, float *xdp, float *scratch,
                            size_t scratch_floats, const float *cmap, const float *tslope, void *stream)
{
    if (!cdl_geom_ok(g) || K < 1 || !vp || !z_prev || !lam || !gam1 || !wA || !wB || !u || !zd || !xdp || (K > 1 && !rd))
        return CDL_EINVAL;
    if (z_after ? !gam2 : (zd_after != nullptr)) return CDL_EINVAL;
    if ((cmap == nullptr) != (tslope == nullptr)) return CDL_EINVAL;   // the (K, 3, M) slopes of lam, gam1, gam2
    const size_t NM = (size_t)g->N * g->M;
    const Scratch sc{scratch, scratch_floats, stream};
    return forward_order_loop(g, K, vp, mask, wB, zd, rd, xdp, sc, [&](int k, const float *x, float alpha, const float *zin) {
        return cdl_analysis_prox_tangent(g, x, wA[k], alpha, zin, u[k], z_prev, z_after, lam + k * NM, gam1 + k * NM,
                                         gam2 ? gam2 + k * NM : nullptr, zd_prev, zd_after, zd[k], scratch, scratch_floats,
                                         cmap, cmap ? tslope + (size_t)k * 3 * g->M : nullptr, stream);
    });
}

}  // extern "C"
