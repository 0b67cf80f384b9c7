// The generic operators cdl_analysis*, cdl_synthesis and cdl_wgrad*: argument checks, ONE tier ladder and the workspace sizes
// that follow from it.  No kernel lives here: every rung is a launcher of another file with the face
// cdl_common.h describes; the first result that is not CDL_EUNSUPPORTED is the call's.
#include "cdl_common.h"

namespace {

enum Op { ANALYSIS, SYNTHESIS, WGRAD };
enum Tier { DENSE, MFMA, TILED, PLAIN };                   // dense matrix-core, sparse matrix-core, register-tiled VALU, plain VALU
struct Rung {
    Tier tier;
    size_t (*ws_floats)(const cdl_geom *);                 // nullptr: the rung uses no workspace
};
const Rung ANALYSIS_RUNGS[] = {{DENSE, [](const cdl_geom *g) { return cdl_dense_ws_floats(g, 0); }},
                               {MFMA, cdl_mfma_analysis_ws_floats}, {TILED, nullptr}, {PLAIN, nullptr}};
const Rung SYNTHESIS_RUNGS[] = {{DENSE, [](const cdl_geom *g) { return cdl_dense_ws_floats(g, 1); }},
                                {MFMA, cdl_mfma_synthesis_ws_floats}, {TILED, cdl_tiled_synthesis_ws_floats}, {PLAIN, nullptr}};
const Rung WGRAD_RUNGS[] = {{DENSE, cdl_dense_wgrad_ws_floats},
                            {MFMA, [](const cdl_geom *g) { return 2 * cdl_mfma_wgrad_ws_floats(g); }},   // room for a paired launch
                            {TILED, cdl_tiled_wgrad_ws_floats}, {PLAIN, nullptr}};

// A tier's own switch, read per call so that one process can compare tiers: CDL_MFMA_DENSE / _ANALYSIS / _SYNTHESIS / _WGRAD=0
// and cdl_set_exact_fp32 turn the matrix cores off.  tier_on: may the rung run -- CDL_NO_TILED leaves the plain tier only.
// These two and cdl_dense_switch_on are the only readers of the switches among the operators.
bool switch_on(Op op, Tier t)
{
    const cdl_options &o = cdl_opts();
    const int sparse[] = {o.mfma_analysis, o.mfma_synthesis, o.mfma_wgrad};
    return t >= TILED || ((t == DENSE ? o.mfma_dense : sparse[op]) != 0 && !cdl_exact_fp32());
}
bool tier_on(Op op, Tier t) { return t == PLAIN || (!cdl_opts().no_tiled && switch_on(op, t)); }

// The ladder: try_rung(tier) of each rung that is on, in order, until one serves the call.
template <size_t R, class Try>
int walk(Op op, const Rung (&rungs)[R], Try &&try_rung)
{
    for (const Rung &r : rungs) {
        const int rc = tier_on(op, r.tier) ? try_rung(r.tier) : CDL_EUNSUPPORTED;
        if (rc != CDL_EUNSUPPORTED) return rc;
    }
    return CDL_EUNSUPPORTED;
}

// The most that a rung which `on` admits may use.
template <size_t R>
size_t walk_ws(Op op, const Rung (&rungs)[R], const cdl_geom *g, bool (*on)(Op, Tier) = tier_on)
{
    size_t n = 0;
    for (const Rung &r : rungs)
        if (cdl_geom_ok(g) && r.ws_floats && on(op, r.tier)) n = max_sz(n, r.ws_floats(g));
    return n;
}

int analysis_impl(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin, const float *gate,
                  const float *tau, float *out, const cdl_prox_args &px, float *ws, size_t ws_floats, void *stream,
                  const cdl_map_args &mp = cdl_map_args{nullptr, nullptr})
{
    if (!cdl_geom_ok(g) || !x || !w || !out) return CDL_EINVAL;
    if (out == zin || (gate && !zin)) return CDL_EINVAL;
    if (mp.cmap && (!mp.tslope || (!tau && !px.zp))) return CDL_EINVAL;   // the map needs its slopes and constant parts
    return walk(ANALYSIS, ANALYSIS_RUNGS, [&](Tier t) -> int {
        switch (t) {
        case DENSE:                                        // (the dense tier's analyses carry neither the CSR prox nor a map)
            if (px.zp || mp.cmap) return CDL_EUNSUPPORTED;
            return cdl_dense_conv(g, 0, x, nullptr, w, alpha, zin, gate, nullptr, nullptr, tau, 0, nullptr, out, ws, ws_floats, stream);
        case MFMA: return cdl_mfma_analysis(g, x, w, alpha, zin, gate, tau, out, px, ws, ws_floats, stream, mp);
        case TILED: return cdl_tiled_analysis(g, x, w, alpha, zin, gate, tau, out, px, stream, mp);
        default: return cdl_plain_analysis(g, x, w, alpha, zin, gate, tau, out, px, stream, mp);
        }
    });
}

}  // namespace

bool cdl_dense_switch_on() { return cdl_opts().mfma_dense != 0 && !cdl_opts().no_tiled; }

extern "C" {

size_t cdl_analysis_workspace_floats(const cdl_geom *g) { return walk_ws(ANALYSIS, ANALYSIS_RUNGS, g); }

int cdl_analysis(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                 const float *gate, const float *tau, float *out, float *workspace, size_t workspace_floats,
                 const float *cmap, const float *tslope, void *stream)
{
    return analysis_impl(g, x, w, alpha, zin, gate, tau, out, cdl_prox_args{}, workspace, workspace_floats, stream,
                         cdl_map_args{cmap, tslope});
}

/* Reverse-sweep step: out = [zsup != 0] (zin + alpha A x)  and  (dt0, dt1) = cdl_tau_grad(out, zsup, c) -- the gradient
 * with respect to z_k, gated by z_k's support, together with the threshold gradients it yields.  One launch where the sparse
 * matrix-core analysis is the rung cdl_analysis would stop at (the gate and the per-tile threshold partials ride in its
 * epilogue); otherwise cdl_analysis followed by cdl_tau_grad_gate.  workspace: cdl_analysis_rev_workspace_floats(g). */
size_t cdl_analysis_rev_workspace_floats(const cdl_geom *g)
{
    if (!cdl_geom_ok(g)) return 0;
    size_t n = (size_t)2 * CDL_TAU_SPLITS * g->N * g->M;       // (twice: the map-weighted partials of a map call)
    n = max_sz(n, cdl_analysis_workspace_floats(g));
    return tier_on(ANALYSIS, MFMA) ? max_sz(n, cdl_mfma_analysis_rev_ws_floats(g)) : n;
}

int cdl_analysis_rev(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                     const float *zsup, const float *c, float *dt0, float *dt1, float *dtau_n, float *out,
                     float *workspace, size_t workspace_floats, const float *cmap, void *stream)
{
    if (!cdl_geom_ok(g) || !x || !w || !out || !zsup || !dt0 || !dt1 || !workspace) return CDL_EINVAL;
    if (cmap && (c || dtau_n)) return CDL_EINVAL;               // a map replaces the per-sample scale
    if (out == zin || out == zsup) return CDL_EINVAL;
    if (workspace_floats < cdl_analysis_rev_workspace_floats(g)) return CDL_EINVAL;
    if (tier_on(ANALYSIS, MFMA) && !(tier_on(ANALYSIS, DENSE) && cdl_dense_takes(g, 0))) {
        const int rc = cdl_mfma_analysis_rev(g, x, w, alpha, zin, zsup, c, dt0, dt1, out, workspace, workspace_floats, stream,
                                               dtau_n, cmap);
        if (rc != CDL_EUNSUPPORTED) return rc;
    }
    CDL_TRY(cdl_analysis(g, x, w, alpha, zin, nullptr, nullptr, out, workspace, workspace_floats, nullptr, nullptr, stream));
    return cdl_tau_grad_gate(g, out, zsup, c, dt0, dt1, dtau_n, workspace, cmap, stream);
}

int cdl_analysis_prox(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                      const float *z_prev, const float *z_after, const float *lam, const float *gam1,
                      const float *gam2, float *u_out, float *out, float *workspace, size_t workspace_floats,
                      const float *cmap, const float *tslope, void *stream)
{
    if (!z_prev || !lam || !gam1 || (z_after && !gam2)) return CDL_EINVAL;
    if (u_out && (u_out == out || u_out == zin)) return CDL_EINVAL;
    if ((cmap == nullptr) != (tslope == nullptr)) return CDL_EINVAL;
    const cdl_prox_args px{z_prev, z_after, lam, gam1, gam2, u_out};
    return analysis_impl(g, x, w, alpha, zin, nullptr, nullptr, out, px, workspace, workspace_floats, stream,
                         cdl_map_args{cmap, tslope});
}

int cdl_analysis_prox_tangent(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin,
                              const float *u, const float *z_prev, const float *z_after, const float *lam,
                              const float *gam1, const float *gam2, const float *zd_prev, const float *zd_after,
                              float *out, float *workspace, size_t workspace_floats, const float *cmap,
                              const float *tslope, void *stream)
{
    if (!u || !z_prev || !lam || !gam1) return CDL_EINVAL;
    if (z_after ? !gam2 : (zd_after != nullptr)) return CDL_EINVAL;
    if (out == u || out == z_prev || out == z_after || out == zd_prev || out == zd_after) return CDL_EINVAL;
    if ((cmap == nullptr) != (tslope == nullptr)) return CDL_EINVAL;   // (the map only enters the pointwise pass's gates)
    // Two launches: the analysis writes ud into `out`, the pointwise tangent rewrites it in place.  (The tangent as a branch
    // of the kernels' CSR epilogue cost the PRIMAL epilogue scalar-register spills: DESIGN.md section 22.)
    CDL_TRY(analysis_impl(g, x, w, alpha, zin, nullptr, nullptr, out, cdl_prox_args{}, workspace, workspace_floats, stream));
    return cdl_prox_csr_tangent(g, out, u, z_prev, z_after, lam, gam1, gam2, zd_prev, zd_after, out, cmap, tslope, stream);
}

size_t cdl_synthesis_workspace_floats(const cdl_geom *g) { return walk_ws(SYNTHESIS, SYNTHESIS_RUNGS, g); }

int cdl_synthesis(const cdl_geom *g, const float *z, const float *gate, const float *w, float alpha,
                  const float *mask, const float *sub, float *out, float *ws, size_t n, void *stream)
{
    if (!cdl_geom_ok(g) || !z || !w || !out) return CDL_EINVAL;
    return walk(SYNTHESIS, SYNTHESIS_RUNGS, [&](Tier t) -> int {
        switch (t) {
        case DENSE: return cdl_dense_conv(g, 1, z, gate, w, alpha, nullptr, nullptr, mask, sub, nullptr, 0, nullptr, out, ws, n, stream);
        case MFMA: return cdl_mfma_synthesis(g, z, gate, w, alpha, mask, sub, out, ws, n, stream);
        case TILED: return cdl_tiled_synthesis(g, z, gate, w, alpha, mask, sub, out, ws, n, stream);
        default: return cdl_plain_synthesis(g, z, gate, w, alpha, mask, sub, out, stream);
        }
    });
}

// The switches decide which rungs count, CDL_NO_TILED does not (cdl_residual_ and cdl_ista_scratch_floats inherit this size)
size_t cdl_wgrad_workspace_floats(const cdl_geom *g) { return walk_ws(WGRAD, WGRAD_RUNGS, g, switch_on); }

int cdl_wgrad(const cdl_geom *g, const float *z, const float *gate, const float *x, float alpha, float *dw, float *ws,
              size_t n, void *stream)
{
    if (!cdl_geom_ok(g) || !z || !x || !dw) return CDL_EINVAL;
    return walk(WGRAD, WGRAD_RUNGS, [&](Tier t) -> int {
        const cdl_wgrad_op op{z, x, alpha, dw};
        switch (t) {
        case DENSE: return cdl_dense_wgrad(g, z, gate, x, alpha, dw, ws, n, stream);
        case MFMA: return cdl_mfma_wgrad(g, &op, 1, gate, 0, ws, n, stream);
        case TILED: return cdl_tiled_wgrad(g, z, gate, x, alpha, dw, ws, n, stream);
        default: return cdl_plain_wgrad(g, z, gate, x, alpha, dw, stream);
        }
    });
}

/* dw0 = alpha0 * z0 (x) x0 and dw1 = alpha1 * z1 (x) x1 (both ungated, same geometry): one paired matrix-core launch
 * where the sparse matrix-core tier is the rung cdl_wgrad would stop at (cdl_wgrad_mfma.hip), two cdl_wgrad calls
 * otherwise.  Same workspace as cdl_wgrad. */
int cdl_wgrad_pair(const cdl_geom *g, const float *z0, const float *x0, float alpha0, float *dw0, const float *z1,
                   const float *x1, float alpha1, float *dw1, float *workspace, size_t workspace_floats, void *stream)
{
    if (!cdl_geom_ok(g) || !z0 || !x0 || !dw0 || !z1 || !x1 || !dw1) return CDL_EINVAL;
    if (tier_on(WGRAD, MFMA) && !(tier_on(WGRAD, DENSE) && cdl_dense_wgrad_takes(g))) {
        const cdl_wgrad_op ops[2] = {{z0, x0, alpha0, dw0}, {z1, x1, alpha1, dw1}};
        const int rc = cdl_mfma_wgrad(g, ops, 2, nullptr, 0, workspace, workspace_floats, stream);
        if (rc != CDL_EUNSUPPORTED) return rc;
    }
    CDL_TRY(cdl_wgrad(g, z0, nullptr, x0, alpha0, dw0, workspace, workspace_floats, stream));
    return cdl_wgrad(g, z1, nullptr, x1, alpha1, dw1, workspace, workspace_floats, stream);
}

}  // extern "C"
