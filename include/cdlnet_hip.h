/* cdlnet_hip.h -- C ABI of libcdlnet_hip.so: the MI355X (gfx950) kernels behind the
 * unrolled-ISTA hot path of RQLuo/CDLNet-video.
 *
 * The reference has no FFI / plugin layer (it is 100 % Python on ATen); its boundary for
 * this path is the nn.Module surface of `model/net.py`.  The Python host package
 * (`cdlnet-video_amd/`) mirrors that surface and calls the entry points below through
 * ctypes; a maintainer of the reference would bind exactly these (INTEGRATION.md shows
 * the stub).  Each entry point names the reference lines whose ATen calls it replaces.
 *
 * Conventions
 *   - plain pointers and ints only; every pointer is DEVICE memory owned by the caller
 *     (PyTorch's caching allocator in practice), fp32 unless a name says otherwise;
 *   - tensors are contiguous, row-major, in the reference's own layouts:
 *       image-like   (N, C, D, H, W)      "thin"  (C = 1 or 3)
 *       code-like    (N, M, Dz, Hz, Wz)   "fat"   (M = 32..169), Dz = D/sd, ...
 *       filter bank  (M, C, Pd, Ph, Pw)   -- Conv{2,3}d.weight and ConvTranspose{2,3}d.weight
 *                                            share this shape (net.py:32-33, 137-142)
 *     2-D nets are the D = Pd = sd = 1, pd = 0 special case;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*, of the CURRENT device) and do
 *     not synchronise.  The compute entry points keep no state between calls and are re-entrant
 *     across streams, devices and ranks; what is process-wide is lock-protected and off the data
 *     path: a snapshot of the experiment switches read once from the environment
 *     (cdl_options_reload), per-device launch attributes, and the opt-in kernel timing of
 *     cdl_fused2d_timing (bench.py only);
 *   - return 0 on success, a negative value on error: -(hipError_t) for runtime errors,
 *     CDL_EINVAL / CDL_EUNSUPPORTED for argument errors.  Nothing throws.
 *   - in-place is allowed only where a parameter says "inout".
 *   - alignment: a pointer argument needs only the alignment of its element type (4 bytes for float / int / unsigned):
 *     a contiguous view at any element offset of an allocation is a valid tensor argument -- a frame of an unbound
 *     clip, one bank of a stacked filter-gradient tensor, one row of a (K,N,M) threshold table.  A launcher selects a
 *     form of a kernel with 16-byte accesses only after it has tested every pointer that form vector-accesses, and
 *     takes the scalar form of the same kernel otherwise (same terms in the same order: same bits).
 *     The exception is what the LIBRARY sizes and only it reads: the workspaces (`ws`, `workspace`, `scratch`), the
 *     fragment buffers (`frags`), the patch buffers the fused stages write (`patches`) and code buffers in an internal
 *     layout (CDL_LAY_BLOCKED*, CDL_LAY_RSC) need 16 bytes, and the call returns CDL_EUNSUPPORTED (cdl_vgg_*:
 *     CDL_EINVAL) otherwise.  DESIGN.md section 26 lists the launchers that gate on alignment.
 */
#ifndef CDLNET_HIP_H
#define CDLNET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDL_EINVAL        (-10001)
#define CDL_EUNSUPPORTED  (-10002)

/* Geometry of one analysis/synthesis operator pair.  D,H,W are the extents of the
 * (reflect-padded) image, multiples of the stride; the code extents are D/sd, H/sh, W/sw.
 * Zero padding p = (P-1)/2 for CDLNet (net.py:32), P/2 per axis for CDLNetVideo (net.py:138). */
typedef struct cdl_geom {
    int N, C, M;
    int D, H, W;
    int Pd, Ph, Pw;
    int pd, ph, pw;
    int sd, sh, sw;
} cdl_geom;

const char *cdl_version(void);

/* Re-read the CDL_* experiment switches from the environment (they are read once, at first use, into an
 * immutable snapshot; tests and tools that flip a variable mid-process call this afterwards). */
int cdl_options_reload(void);

/* Arithmetic of the shape-generic entry points (cdl_analysis*, cdl_synthesis*, cdl_wgrad*, cdl_ista_* sweeps) called from
 * THIS host thread afterwards: on != 0 keeps them on the fp32 VALU kernels (plain fp32 FMAs: ~3e-6 of an fp64 evaluation even
 * where sums cancel), on == 0 (the default) lets them use the matrix cores (split-bf16 operands: 16-17 significant bits, which
 * a cancelling filter gradient amplifies -- DESIGN.md section 6).  Returns the previous setting.  The fused entry points
 * (cdl_fused2d_*, cdl_fusedg_*) are matrix-core kernels by construction and are not affected: a caller that wants fp32
 * end to end composes the generic ones (the Python host side does: loop.precision_scope("fp32")). */
int cdl_set_exact_fp32(int on);

/* Launch trace (host code, off by default): which kernel of which tier an entry point ran.
 * While on, every kernel launch of the library appends one record to a process-wide log:
 *     <source file>:<line> \t <launcher with the values of its template arguments> \t <note> \n
 * the note holding the run-time variant values of the launcher's plan (and the kernel's name where one launcher
 * has several launches).  cdl_trace(on) returns the previous state and clears the log when switched on.
 * cdl_trace_read copies the log, NUL-terminated and cut to cap, into buf (nullable) and returns its full length in
 * bytes.  CDL_TRACE_FILE=path (read with the other switches) appends each distinct record once to that file as well,
 * from every process that has it set.  Off, a launch pays one relaxed atomic load. */
int cdl_trace(int on);
size_t cdl_trace_read(char *buf, size_t cap);

/* ---- boundary of the loop: model/utils.py:5-22 (pre_process), :70-87 (pre_process_3d) -------
 * mean[n] = sum(y[n]) / (mask ? sum(mask[n]) : numel);  yp = reflect_pad(mask * (y - mean));
 * mask_p = reflect_pad(mask).  pads = {d_lo, d_hi, h_lo, h_hi, w_lo, w_hi} (floor/ceil split,
 * utils.py:35-51).  y: (N,C,D,H,W) unpadded; yp/mask_p: (N,C,D+..,H+..,W+..). */
int cdl_preprocess(const float *y, const float *mask /*nullable*/, float *yp,
                   float *mask_p /*nullable iff mask is*/, float *mean /*N*/,
                   int N, int C, int D, int H, int W, const int pads[6], void *stream);

/* model/utils.py:24-33 (post_process), :89-101: xhat = crop(xp) + mean. D,H,W = unpadded. */
int cdl_postprocess(const float *xp, const float *mean, float *xhat,
                    int N, int C, int D, int H, int W, const int pads[6], void *stream);

/* Adjoint of the crop in cdl_postprocess (autograd of utils.py:26-27): gxp = zero outside the
 * crop window, gxhat inside.  D,H,W = unpadded extents of gxhat; gxp has the padded extents. */
int cdl_postprocess_bwd(const float *gxhat, float *gxp, int N, int C, int D, int H, int W,
                        const int pads[6], void *stream);

/* Adjoint of cdl_preprocess (+ the mean that cdl_postprocess adds back), for gradients with respect to y: with
 * G = the adjoint of the reflect pad applied to dyp (mirrored border values added into their interior sources) and
 * sums over (C,D,H,W) per sample,
 *     no mask: dy = G - mean(G) + sum(g_xhat) / (C D H W)
 *     mask:    dy = mask * G + (sum(g_xhat) - sum(mask * G)) / sum(mask)
 * g_xhat NULL = a loss on the code only (no mean term).  One workgroup per sample, double sums in a fixed order:
 * deterministic.  dyp: (N,C,D+..,H+..,W+..); g_xhat, mask, dy: (N,C,D,H,W) unpadded. */
int cdl_preprocess_bwd(const float *dyp, const float *g_xhat /*nullable*/, const float *mask /*nullable*/, float *dy,
                       int N, int C, int D, int H, int W, const int pads[6], void *stream);

/* tau[k,n,m] = t[k,0,m] + c[n] * t[k,1,m]   (net.py:82,85,87; c = sigma/255 or absent = 0) */
int cdl_thresholds(const float *t /*K,2,M*/, const float *c /*N, nullable*/, float *tau /*K,N,M*/,
                   int K, int N, int M, void *stream);

/* Stand-alone ST(x, t) = sign(x)*relu(|x|-t) (net.py:11-14) over a code-like tensor:
 * out[i] = ST(x[i], tau[i / per_m]) for `rows` = N*M rows of `per_m` elements.  In the nets the
 * shrinkage is fused into cdl_analysis; this exists for callers of the reference's helper.
 * This and the other pointwise passes (cdl_shrink_b*, cdl_prox_csr*) launch one thread per element and return
 * CDL_EUNSUPPORTED for a tensor of 2^39 elements or more (2^31 workgroups). */
int cdl_shrink(const float *x, const float *tau /*rows*/, float *out, int rows, size_t per_m,
               void *stream);

/* ---- thresholds of any broadcast shape --------------------------------------
 * The reference's ST / prox_CSR / prox_CSR_f2 take any threshold that broadcasts to the code shape (N, M, spatial..): a
 * noise-level map enters as t[k,:1] + c * t[k,1:2] with c (N,1,H,W).  cdl_bcast holds the element strides of such a tensor
 * over (sample, channel, code pixel): element (n, m, pix) reads thr[n*s.n + m*s.m + pix*s.p].  A stride is 0 on a
 * broadcast axis and otherwise the dense stride of the contiguous tensor; the spatial axes are broadcast together (p = 0)
 * or all present (p = 1: the caller expands a partly spatial threshold to the full code grid).  {M, 1, 0} is the row form
 * of the entry points without _b, which are its callers.  Anything else is CDL_EINVAL. */
typedef struct cdl_bcast {
    long long n, m, p;
} cdl_bcast;

int cdl_shrink_b(const float *x, const float *tau, const cdl_bcast *s_tau, float *out, int N, int M, size_t per_m,
                 void *stream);
/* Reverse of cdl_shrink_b as autograd differentiates sign(x)*relu(|x|-t): gx = gup where x != 0 and |x| - t > 0, else 0
 * (gx may alias gup), and, when not NULL, dtau_el[i] = -sign(x[i]) * gx[i]: the threshold gradient per code element,
 * which the caller reduces over the threshold's broadcast axes. */
int cdl_shrink_b_bwd(const float *gup, const float *x, const float *tau, const cdl_bcast *s_tau, float *gx,
                     float *dtau_el /*nullable*/, int N, int M, size_t per_m, void *stream);

/* ---- analysis half: F.conv2d / F.conv3d at net.py:85,87,200,205 and gabor.py:55 ------------
 *   acc  = alpha * corr(x ; w)                         x thin, w (M,C,P..), acc fat
 *   base = zin ? (gate ? (gate != 0 ? zin : 0) : zin) : 0
 *   out  = tau ? ST(base + acc, tau[n,m]) : base + acc,  ST(u,t) = sign(u)*max(|u|-t,0) (net.py:11-14)
 * Forward k=0: (alpha=+1, zin=NULL, tau).  Forward k>=1: (alpha=-1, zin=z_k, tau) with
 * x = mask*B_k z_k - yp.  Backward: g_k = [z_{k+1}!=0]*g_{k+1} + corr(q ; B_k) is
 * (alpha=+1, zin=g_{k+1}, gate=z_{k+1}, tau=NULL).  out must not alias zin.
 * Noise-level map (net.py:82-87 with a sigma that varies over the code grid; both NULL: none): cmap (N, code pixels)
 * and tslope (M) turn the threshold of element (n, m, pix) into tau[n,m] + cmap[n,pix] * tslope[m] -- tau then holds
 * t[k,0,m], tslope t[k,1,m], cmap sigma/255; the product is rounded before the sum, as torch's broadcast does.
 * workspace (cdl_analysis_workspace_floats(g) floats, 0 when no kernel wants it) lets the matrix-core kernel of the
 * shape-generic path stage its prepared filter fragments.  workspace == NULL: VALU. */
int cdl_analysis(const cdl_geom *g, const float *x, const float *w, float alpha,
                 const float *zin /*nullable*/, const float *gate /*nullable*/,
                 const float *tau /*N*M, nullable*/, float *out, float *workspace /*nullable*/, size_t workspace_floats,
                 const float *cmap /*nullable*/, const float *tslope /*M, nullable*/, void *stream);
size_t cdl_analysis_workspace_floats(const cdl_geom *g);
/* One step of the reverse sweep (autograd of net.py:87 / 205 through the shrinkage of the previous iteration):
 *   out = [zsup != 0] * (zin + alpha * A x),   (dt0, dt1[, dtau_n]) = cdl_tau_grad(out, zsup, c)
 * i.e. cdl_analysis followed by cdl_tau_grad_gate, as ONE fat launch where the matrix-core analysis covers the
 * geometry (gate and threshold partials in its epilogue).  dtau_n NULL: no per-sample threshold gradients.
 * out must differ from zin and zsup.  cmap (nullable; then c and dtau_n must be NULL): as cdl_tau_grad's.
 * workspace: required, cdl_analysis_rev_workspace_floats(g) floats. */
int cdl_analysis_rev(const cdl_geom *g, const float *x, const float *w, float alpha, const float *zin /*nullable*/,
                     const float *zsup, const float *c /*N, nullable*/, float *dt0 /*M*/, float *dt1 /*M*/,
                     float *dtau_n /*N,M, nullable*/, float *out, float *workspace, size_t workspace_floats,
                     const float *cmap /*N, code pixels; nullable*/, void *stream);
size_t cdl_analysis_rev_workspace_floats(const cdl_geom *g);

/* ---- synthesis half: F.conv_transpose2d/3d at net.py:87,90,205,210 and gabor.py:64 ----------
 *   v   = alpha * corrT( gate ? [gate!=0]*z : z ; w )   z fat, v thin, output_padding = s-1
 *   out = (mask ? mask*v : v) - (sub ? sub : 0)
 * Forward residual r_k = mask*B_k z_k - yp: (alpha=1, mask, sub=yp).  Dictionary synthesis
 * D z_K: (alpha=1, NULL, NULL).  Backward q_k = mask * (-A_k^T du): (z=g, gate=z_{k+1}, alpha=-1, mask).
 * workspace: scratch for launches too small to fill the GPU (single frames, crops): the code channels are then split
 * over extra workgroups whose partial images (cdl_synthesis_workspace_floats(g) floats, 0 when no split is worthwhile)
 * are added in a fixed order.  workspace == NULL: no split. */
int cdl_synthesis(const cdl_geom *g, const float *z, const float *gate /*nullable*/, const float *w, float alpha,
                  const float *mask /*nullable*/, const float *sub /*nullable*/, float *out,
                  float *workspace /*nullable*/, size_t workspace_floats, void *stream);
size_t cdl_synthesis_workspace_floats(const cdl_geom *g);

/* ---- filter gradients (autograd of the two conv calls above; train.py:98) --------------------
 *   dw[m,c,kd,ki,kj] = alpha * sum_{n,zd,zy,zx} zg[n,m,zd,zy,zx] * x[n,c,zd*sd-pd+kd, zy*sh-ph+ki, zx*sw-pw+kj]
 * with zg = gate ? [gate!=0]*z : z.  dA_k: (z=g_{k+1}, gate=z_{k+1}, x=r_k, alpha=-1);
 * dB_k: (z=z_k, x=q_k, alpha=+1).  Deterministic (no atomics).  Pw <= 16. dw is overwritten. */
int cdl_wgrad(const cdl_geom *g, const float *z, const float *gate /*nullable*/, const float *x,
              float alpha, float *dw, float *workspace /*nullable*/, size_t workspace_floats, void *stream);
/* Two UNGATED filter gradients of one geometry -- the dA_k / dB_k pair of an iteration of the reverse sweep
 * (train.py:98 through net.py:87 / 204-207) -- as one launch where the matrix-core kernel covers the shape; otherwise two
 * cdl_wgrad calls.  Same results as two calls, same workspace (cdl_wgrad_workspace_floats). */
int cdl_wgrad_pair(const cdl_geom *g, const float *z0, const float *x0, float alpha0, float *dw0, const float *z1,
                   const float *x1, float alpha1, float *dw1, float *workspace, size_t workspace_floats,
                   void *stream);
/* Scratch (floats) that lets cdl_wgrad split the pixel range over more workgroups (two-stage,
 * fixed-order reduction).  Without a workspace a slower single-stage kernel is used. */
size_t cdl_wgrad_workspace_floats(const cdl_geom *g);

/* Threshold gradients of one iteration: with du = [zout!=0]*g,
 *   dt0[m] = -sum_{n,pix} sign(zout)*du,   dt1[m] = -sum_n c[n] * sum_pix sign(zout)*du
 * (c NULL -> dt1 = 0).  dtau_n (nullable) receives the per-sample threshold gradient dtau_n[n,m] = -sum_pix
 * sign(zout)*du of sample n (dt0 = sum_n dtau_n, dt1 = sum_n c[n] dtau_n): what dL/dc needs; dt0 / dt1 do not depend
 * on whether it is given.  scratch: CDL_TAU_SPLITS*N*M floats (rows are split over workgroups and folded in a fixed
 * order). dt0/dt1 are overwritten.
 * cmap (N, code pixels; nullable): the noise-level map of cdl_analysis in place of c (c and dtau_n must then be NULL):
 *   dt1[m] = -sum_{n,pix} cmap[n,pix] * sign(zout)*du, a second partial per row; scratch: 2*CDL_TAU_SPLITS*N*M floats. */
#define CDL_TAU_SPLITS 16
int cdl_tau_grad(const cdl_geom *g, const float *gup, const float *zout, const float *c /*N, nullable*/,
                 float *dt0 /*M*/, float *dt1 /*M*/, float *dtau_n /*N,M, nullable*/,
                 float *scratch /*CDL_TAU_SPLITS*N*M*/, const float *cmap /*nullable*/, void *stream);
/* Same, and gup is gated IN PLACE (gup[i] = 0 where zout[i] == 0) in the same pass: the reverse sweep's three
 * consumers of the gated gradient then need no gate (one fat read each less). */
int cdl_tau_grad_gate(const cdl_geom *g, float *gup /*inout*/, const float *zout, const float *c /*N, nullable*/,
                      float *dt0 /*M*/, float *dt1 /*M*/, float *dtau_n /*N,M, nullable*/,
                      float *scratch /*CDL_TAU_SPLITS*N*M*/, const float *cmap /*nullable*/, void *stream);
/* Gradient of the noise-level map, one iteration (a reduction over the code channels, fixed order):
 *   dcmap[n,pix] (+)= -sum_m tslope[m] * sign(z[n,m,pix]) * du[n,m,pix]      du = dL/du_k (gated), z = z_{k+1}
 * acc_add 0: dcmap is overwritten. */
int cdl_sigma_grad(const cdl_geom *g, const float *du, const float *z, const float *tslope /*M*/,
                   float *dcmap /*N, code pixels*/, int acc_add, void *stream);
/* Generic reverse sweep, iteration k: q holds S = A_k^T du_k (unmasked, alpha = +1); dyp = S (acc_add 0) or dyp += S,
 * then with make_q: q = -(mask ? mask : 1) * S in place -- the q_k the sweep continues with. */
int cdl_dyp_split(const cdl_geom *g, float *q /*inout, thin*/, const float *mask /*nullable*/, float *dyp,
                  int acc_add, int make_q, void *stream);

/* ---- CSR temporal variants --------------------------------------
 * prox_CSR / prox_CSR_f2 of model/net.py:229-262, the shrinkage that CDLNet_CSR.forward
 * (net.py:438-455) and CDLNet_CSRf2.forward (net.py:545-563) apply instead of ST when a neighbour
 * frame's code is supplied.  u, z_prev, z_after, out are fat (N,M,D/sd,H/sh,W/sw); lam, gam1, gam2 are
 * per (sample, channel) like tau (N*M, from cdl_thresholds).  z_after == NULL selects
 *   out = ST(ST(u - z_prev - lam*sign(z_prev), lam*gam1) + z_prev + lam*sign(z_prev), lam)
 * and z_after != NULL the three-level map with both neighbours.  The reference's evaluation order is
 * kept term by term (no fma): the maps are discontinuous for negative thresholds.  out may alias u. */
int cdl_prox_csr(const cdl_geom *g, const float *u, const float *z_prev, const float *z_after /*nullable*/,
                 const float *lam, const float *gam1, const float *gam2 /*nullable iff z_after is*/,
                 float *out, void *stream);

/* cdl_analysis with the CSR map as its epilogue (one fat write + read per iteration less than
 * cdl_analysis followed by cdl_prox_csr):  u = zin + alpha*corr(x ; w),  out = prox(u; z_prev[, z_after]),
 * and u itself to u_out when it is not NULL (the reverse sweep needs it).  Same bits as the two-call form.
 * Noise-level map (both NULL: none): cmap (N, code pixels) with tslope (3,M), the slopes of lam,
 * gam1, gam2 in this order (the third plane unread without z_after).  lam / gam1 / gam2 then hold the constant parts and
 * element (n, m, pix) takes lam[n,m] + cmap[n,pix]*tslope[0,m] etc., the product rounded before the sum.
 * workspace: as cdl_analysis's (NULL: VALU). */
int cdl_analysis_prox(const cdl_geom *g, const float *x, const float *w, float alpha,
                      const float *zin /*nullable*/, const float *z_prev, const float *z_after /*nullable*/,
                      const float *lam, const float *gam1, const float *gam2 /*nullable*/,
                      float *u_out /*nullable*/, float *out, float *workspace /*nullable*/, size_t workspace_floats,
                      const float *cmap /*nullable*/, const float *tslope /*3*M, nullable*/, void *stream);

/* Tangent of the two maps.  They are piecewise linear in (u, z_prev, z_after); with the intermediates
 * of the PRIMAL (u, z_prev[, z_after], lam, gam*) and st_dx(x,t) = (x != 0 && |x| - t > 0):
 *   prox_CSR:     Ga = st_dx(a, lam*gam1), Gm = st_dx(m, lam):              out = Gm ? (Ga ? ud : zd_prev) : 0
 *   prox_CSR_f2:  Ga = st_dx(a, t1), Gb = st_dx(b, t2), Gm = st_dx(m, lam): out = Gm ? (Gb ? (Ga ? ud - zd_prev : 0) : zd_after) : 0
 * evaluated as selects (a NaN in a dead branch does not leak); no threshold enters a value.  ud: the tangent of u;
 * zd_prev / zd_after (nullable): the neighbours' tangents, NULL = zero (a constant neighbour).  out may alias ud.
 * Noise-level map (both NULL: none, one without the other: CDL_EINVAL): cmap (N, code pixels) with
 * tslope (3,M) as in cdl_analysis_prox, lam / gam1 / gam2 the constant parts -- the gates are read at the thresholds the
 * primal's epilogue formed, lam[n,m] + cmap[n,pix]*tslope[0,m] etc., the product rounded before the sum. */
int cdl_prox_csr_tangent(const cdl_geom *g, const float *ud, const float *u, const float *z_prev,
                         const float *z_after /*nullable*/, const float *lam, const float *gam1,
                         const float *gam2 /*nullable iff z_after is*/, const float *zd_prev /*nullable*/,
                         const float *zd_after /*nullable*/, float *out, const float *cmap /*nullable*/,
                         const float *tslope /*3*M, nullable*/, void *stream);

/* The tangent step of one iteration: ud = zin + alpha*corr(x ; w) (cdl_analysis into out), then
 * out = Jprox(u; z_prev[, z_after])(ud, zd_prev, zd_after) in place (cdl_prox_csr_tangent): two launches, the bits of the
 * two calls.  (As a branch of the kernels' CSR epilogue it slowed the primal epilogue: DESIGN.md section 22.)
 * workspace: as cdl_analysis's (NULL: VALU).  cmap / tslope: as cdl_prox_csr_tangent's (the analysis takes no map). */
int cdl_analysis_prox_tangent(const cdl_geom *g, const float *x, const float *w, float alpha,
                              const float *zin /*nullable*/, const float *u, const float *z_prev,
                              const float *z_after /*nullable*/, const float *lam, const float *gam1,
                              const float *gam2 /*nullable*/, const float *zd_prev /*nullable*/,
                              const float *zd_after /*nullable*/, float *out, float *workspace /*nullable*/,
                              size_t workspace_floats, const float *cmap /*nullable*/,
                              const float *tslope /*3*M, nullable*/, void *stream);

/* Reverse of cdl_prox_csr as autograd differentiates the reference expression (sign() has zero
 * gradient): gu = dL/du (may alias gz); gz_prev / gz_after (nullable) are ACCUMULATED into, because a
 * neighbour code feeds all K iterations; dlam, dgam1, dgam2 are (2,M) and receive
 * [sum_n s, sum_n c[n]*s] of the per-(n,m) threshold sums, i.e. the gradients of t[k], g1[k], g2[k]
 * under lam = t[k,0] + c*t[k,1] (net.py:444).  scratch: cdl_prox_csr_scratch_floats(g) floats.
 * dsum_n (3,N,M; nullable): the per-(n,m) sums s themselves, family by family (lam, gam1, gam2; the third plane is
 * written only with z_after) -- dL/dc[n] is formed from them.
 * Noise-level map: cmap (N, code pixels) with tslope (3,M) as in cdl_analysis_prox, lam / gam1 /
 * gam2 the constant parts; c and dsum_n must then be NULL, dlam / dgam1 / dgam2 receive [sum s, sum cmap*s] over samples
 * and pixels, and dcmap (N, code pixels; nullable) is ACCUMULATED into:
 *     dcmap[n,pix] += sum_m tslope[0,m]*s_lam + tslope[1,m]*s_gam1 + tslope[2,m]*s_gam2
 * Every reduction has a fixed order (no atomics); nothing of the code tensors' size is written beside gu, gz_*. */
int cdl_prox_csr_bwd(const cdl_geom *g, const float *gz, const float *u, const float *z_prev,
                     const float *z_after /*nullable*/, const float *lam, const float *gam1,
                     const float *gam2 /*nullable*/, const float *c /*N, nullable*/, float *gu,
                     float *gz_prev /*nullable*/, float *gz_after /*nullable*/, float *dlam /*2*M*/,
                     float *dgam1 /*2*M*/, float *dgam2 /*2*M, nullable*/, float *scratch,
                     size_t scratch_floats, const float *cmap /*nullable*/, const float *tslope /*3*M, nullable*/,
                     float *dcmap /*nullable*/, float *dsum_n /*3*N*M, nullable*/, void *stream);
/* (covers the map form whether or not a map is passed: N*M*ceil(pixels/1024)*24 wave partials + MS*N*pixels map-gradient
 *  partials, MS <= ceil(M/8) channel ranges -- a few MB at 8 x 256 x 256; cdl_ista_scratch_floats includes it) */
size_t cdl_prox_csr_scratch_floats(const cdl_geom *g);

/* The two maps and their reverse with thresholds of any broadcast shape (cdl_bcast above; s_gam2 is read only with
 * z_after).  The forward bits are those of the reference expression for every threshold shape.  In the reverse pass each
 * of dlam, dgam1, dgam2 (nullable: not wanted) receives the gradient of its threshold before the reduction over its
 * broadcast axes, which is the caller's: N*M row sums (fixed order) for a threshold without spatial extent (p = 0), one
 * value per code element (N*M*code pixels) for one with (p = 1).  gu, gz_prev, gz_after, scratch: as cdl_prox_csr_bwd. */
int cdl_prox_csr_b(const cdl_geom *g, const float *u, const float *z_prev, const float *z_after /*nullable*/,
                   const float *lam, const cdl_bcast *s_lam, const float *gam1, const cdl_bcast *s_gam1,
                   const float *gam2 /*nullable iff z_after is*/, const cdl_bcast *s_gam2, float *out, void *stream);
int cdl_prox_csr_b_bwd(const cdl_geom *g, const float *gz, const float *u, const float *z_prev,
                       const float *z_after /*nullable*/, const float *lam, const cdl_bcast *s_lam, const float *gam1,
                       const cdl_bcast *s_gam1, const float *gam2 /*nullable*/, const cdl_bcast *s_gam2, float *gu,
                       float *gz_prev /*nullable*/, float *gz_after /*nullable*/, float *dlam /*nullable*/,
                       float *dgam1 /*nullable*/, float *dgam2 /*nullable*/, float *scratch, size_t scratch_floats,
                       void *stream);

/* ---- blind noise-level estimate --------------------------------------
 * model/nle.py:17-27 (nle_mad) with the filter of model/wvlt.py:13-41: sigma_hat[n] = median over (C,H',W') of
 * |conv2d(y, flip(outer(dec_hi, dec_hi)) of 'bior4.4', stride 2, groups C)| / 0.6745, the lower median as
 * torch.median returns it (exact selection, no sort).  y (N,C,H,W) in the reference's [0,1] scale, H,W >= 10;
 * callers multiply by 255 (analyze.py:139).  scratch: cdl_nle_mad_scratch_floats(N,C,H,W) floats. */
size_t cdl_nle_mad_scratch_floats(int N, int C, int H, int W);
int cdl_nle_mad(const float *y, float *sigma_hat /*N*/, float *scratch, size_t scratch_floats, int N, int C,
                int H, int W, void *stream);

/* The same estimate over windows of the band: along an axis of band length L = (H-10)/2 + 1
 * there is one cell [0, L) if L <= window, otherwise ceil((L - window) / step) + 1 cells of `window` samples, cell i
 * starting at min(i * step, L - window).  cells[n][iy][ix] = lower median of |HHy| over the cell and all C channels
 * / 0.6745, exact; a window that covers the band gives the bits of cdl_nle_mad.  No atomics on floats: repeated
 * calls are bit-identical.  CDL_EINVAL: null pointers, window < 2, step < 1, H or W < 10.
 * scratch: cdl_nle_mad_cells_scratch_floats(N,C,H,W) floats (the band). */
size_t cdl_nle_mad_cells_scratch_floats(int N, int C, int H, int W);
int cdl_nle_mad_cells(const float *y, float *cells /*N x ny x nx*/, float *scratch, size_t scratch_floats, int N,
                      int C, int H, int W, int window, int step, void *stream);

/* The noise-level function of signal-dependent noise, var(y | x) = a x + b: the same band
 * binned by local intensity instead of position.  Band sample (i, j) carries d = |HHy| and the key m = the mean of
 * the 7 x 7 pixels under the non-zero taps (rows 2i+2 .. 2i+8, columns 2j+2 .. 2j+8; an fp32 sum / 49).  With
 * scale = (float)(bins / (hi - lo)) a sample belongs to bin k = (int)floorf((m - lo) * scale) if lo <= m < hi and
 * k < bins, otherwise to none; all C channels of an image pool.  count_bins[n][k] = members (int32),
 * sigma_bins[n][k] = their lower median of d (rank (count - 1) / 2) / 0.6745, exact; an empty bin gives 0, 0.
 * Integer counting only: repeated calls are bit-identical.  CDL_EINVAL before any launch: null pointers, H or W <
 * 10, bins < 1, hi <= lo, scratch too small.  scratch: cdl_nle_nlf_bins_scratch_floats(N,C,H,W) floats (two bands). */
size_t cdl_nle_nlf_bins_scratch_floats(int N, int C, int H, int W);
int cdl_nle_nlf_bins(const float *y, float *sigma_bins /*N x bins*/, int *count_bins /*N x bins*/, float *scratch,
                     size_t scratch_floats, int N, int C, int H, int W, int bins, float lo, float hi, void *stream);

/* model/nle.py:29-89 (nle_pca), the per-pass work of one channel: over every patchsize x patchsize patch of channel
 * `channel` of y (N,C,H,W), pooled over the batch, its texture strength Xtr (the sums of the squared half-differences
 * ((x[i][j] - x[i][j+2]) / 2)^2 over the patch's p x (p-2) window plus those along rows over its (p-2) x p window),
 * and over the patches with Xtr < tau (tau = +inf keeps every patch) the non-centred second moment
 * gram = sum x x^T (fp64, p^2 x p^2, both triangles) and their number *count (int64).  3 <= patchsize <= 11,
 * H, W >= patchsize.  Deterministic: partials are reduced in a fixed order.  The host divides by count - 1.
 * scratch: cdl_nle_pca_scratch_floats(N,C,H,W,patchsize) floats. */
size_t cdl_nle_pca_scratch_floats(int N, int C, int H, int W, int patchsize);
int cdl_nle_pca_gram(const float *y, int N, int C, int H, int W, int channel, int patchsize, float tau,
                     double *gram /*p^2 x p^2*/, long long *count /*1*/, float *scratch, size_t scratch_floats,
                     void *stream);

/* The same pass over a regular grid of cells, every cell of every sample its own domain:
 * along an axis of L pixels there is one cell [0, L) if L <= window, otherwise ceil((L - window) / step) + 1 cells of
 * `window` pixels, cell i starting at min(i * step, L - window).  Cell (n, iy, ix) takes only the patches that lie
 * wholly inside it ((window - p + 1)^2 origins for a full cell; samples never pool, overlapping cells each form
 * their own Gram) whose Xtr < tau[n][iy][ix] (fp32, device; +inf keeps every patch), and gives
 * gram[n][iy][ix] = sum x x^T (fp64, p^2 x p^2, both triangles) and count[n][iy][ix] (int64).  Same kernels and the
 * same fixed reduction order per cell as cdl_nle_pca_gram, with shorter fp32 chains (8 patches) between the fp64
 * additions, since a cell has few patches to average the rounding over: repeated calls are bit-identical.
 * CDL_EINVAL before any launch: null pointers, patchsize outside 3..11, window < patchsize, step < 1, H or W <
 * patchsize.  scratch: cdl_nle_pca_gram_cells_scratch_floats(N,C,H,W,patchsize,window,step) floats. */
size_t cdl_nle_pca_gram_cells_scratch_floats(int N, int C, int H, int W, int patchsize, int window, int step);
int cdl_nle_pca_gram_cells(const float *y, int N, int C, int H, int W, int channel, int patchsize, int window,
                           int step, const float *tau /*N x ny x nx*/, double *gram /*N x ny x nx x p^2 x p^2*/,
                           long long *count /*N x ny x nx*/, float *scratch, size_t scratch_floats, void *stream);

/* ---- SSIM (the evaluation metric of analyzemri.py and the loss term of loss.py's CombinedLossWithSSIM) ----------
 * P independent contiguous H x W planes of x and y; the window is `taps` host-side 1-D weights `win` (odd, 3..15,
 * H, W >= taps) that sum to 1 (within 1e-5; otherwise CDL_EINVAL: the kernels centre each tile on one pixel, which is
 * exact only for a normalised window), applied along both axes with valid filtering: Ho x Wo = (H - taps + 1) x
 * (W - taps + 1) positions.
 * Per position, with the window moments of x and y, sx = kappa (E[x^2] - E[x]^2) (and sy, sxy alike),
 * C1 = (K1 R)^2, C2 = (K2 R)^2, R = data_range[plane] (device, P floats):
 *     cs = (2 sxy + C2) / (sx + sy + C2),  S = (2 mx my + C1) / (mx^2 + my^2 + C1) * cs.
 * cdl_ssim_fwd writes the per-plane means of S and cs over the positions (cs nullable).  cdl_ssim_bwd takes the
 * per-plane upstream gradients g_ssim of those SSIM means and writes dx, dy (each nullable) and the per-plane
 * dL/dR (nullable); at least one of the three.  Both deterministic: fixed-order fp64 reductions, no atomics.
 * scratch: cdl_ssim_scratch_floats(P,H,W,taps) floats, shared by both (0: shape or taps not supported). */
size_t cdl_ssim_scratch_floats(int P, int H, int W, int taps);
int cdl_ssim_fwd(const float *x, const float *y, int P, int H, int W, const float *win /*host, taps*/, int taps,
                 float K1, float K2, float kappa, const float *data_range /*P*/, float *ssim /*P*/,
                 float *cs /*P, nullable*/, float *scratch, size_t scratch_floats, void *stream);
int cdl_ssim_bwd(const float *x, const float *y, int P, int H, int W, const float *win /*host, taps*/, int taps,
                 float K1, float K2, float kappa, const float *data_range /*P*/, const float *g_ssim /*P*/,
                 float *dx /*nullable*/, float *dy /*nullable*/, float *d_range /*P, nullable*/, float *scratch,
                 size_t scratch_floats, void *stream);

/* ---- MS-SSIM (pytorch_msssim's ms_ssim): the SSIM kernels above over a 2x2 average-pooling pyramid ---------------
 * Level 0 is the caller's P planes of H x W; level i + 1 is torch's avg_pool2d(level i, 2, padding = [H_i % 2, W_i % 2])
 * (count_include_pad: an odd axis gets one zero row / column in FRONT and the divisor stays 4), H_{i+1} = (H_i + 1) / 2.
 * kappa is 1; win, taps, K1, K2, data_range as above, the same at every level.
 * cdl_msssim_pyramid_floats: floats of the levels 1 .. levels-1 of P planes, stored back to back (0: levels outside
 * 1..8, or a level below 3 x 3).  cdl_msssim_scratch_floats: the scratch of both calls (0: taps not supported, levels
 * outside 1..8, or a level smaller than the window).
 * cdl_msssim_fwd: one call for the whole pyramid, two launches per level.  Writes vals[level][plane] = {mean of S, mean
 * of cs} (raw: the relu, the powers and the product of ms_ssim stay with the caller) and, for levels > 1, the pooled
 * planes pyr_x, pyr_y (cdl_msssim_pyramid_floats each; the level's own forward launch writes the next level).
 * cdl_msssim_bwd: g_vals[level][plane] = upstream gradients of {S mean, cs mean}; writes dx, dy (H x W planes) and the
 * per-plane dL/dR summed over the levels, each nullable, at least one given.  Coarsest level first, one launch per level
 * (two when d_range is given); a level's dx, dy land in `work` (2 x cdl_msssim_pyramid_floats floats, x side first;
 * needed when levels > 1 and dx or dy is given) and the next finer level adds a quarter of them to its own pixels.
 * Deterministic like the calls above.  CDL_EINVAL before any launch: a null pointer that is needed, a window that does
 * not sum to 1, a scratch shorter than cdl_msssim_scratch_floats, a shape that function refuses.  pyr_*, vals and work
 * are caller tensors: 4-byte alignment is enough. */
size_t cdl_msssim_pyramid_floats(int P, int H, int W, int levels);
size_t cdl_msssim_scratch_floats(int P, int H, int W, int taps, int levels);
int cdl_msssim_fwd(const float *x, const float *y, int P, int H, int W, const float *win /*host, taps*/, int taps,
                   float K1, float K2, const float *data_range /*P*/, int levels, float *pyr_x, float *pyr_y,
                   float *vals /*levels x P x 2*/, float *scratch, size_t scratch_floats, void *stream);
int cdl_msssim_bwd(const float *x, const float *y, const float *pyr_x, const float *pyr_y, int P, int H, int W,
                   const float *win /*host, taps*/, int taps, float K1, float K2, const float *data_range /*P*/,
                   int levels, const float *g_vals /*levels x P x 2*/, float *dx /*nullable*/, float *dy /*nullable*/,
                   float *d_range /*P, nullable*/, float *work, float *scratch, size_t scratch_floats, void *stream);

/* ---- perceptual term of loss.py's CombinedLossWithSSIM: VGG16 features[:16] (relu3_3) -------------------------
 * P independent contiguous one-channel H x W planes (H, W >= 4) of the output x and the target y; every frame is the
 * reference's three-channel repeat, so conv1_1 runs on the filters summed over their input channels.  The seven
 * convolutions (torchvision's features.{0,2,5,7,10,12,14}) come as device pointer arrays w[7] ((O, I, 3, 3)) and
 * b[7] (O).  With F = relu3_3, (256, H4, W4) per plane, H4 = floor(floor(H/2)/2) (W4 alike):
 *     loss = mean over all P * 256 * H4 * W4 elements of (F(x) - F(y))^2.
 * cdl_vgg_forward runs F(y) first, into feat (P * 256 * H4 * W4, nullable: scratch), then, with x, writes loss (one
 * device float) and the seeds of the backward; x NULL: F(y) into feat only (grads 0).  grads (CDL_VGG_DX |
 * CDL_VGG_DY) asks it to keep what cdl_vgg_backward needs for dx / dy.  cdl_vgg_backward (the same grads, scratch and
 * weights) writes dx = dloss/dx * g_loss[0] and dy (each nullable, at least one; g_loss a device float).  No weight
 * gradients.  Both deterministic (fixed-order fp64 sums, no atomics), no host synchronisation.
 * scratch: cdl_vgg_scratch_floats(P, H, W, grads) floats, 16-byte aligned (0: shape not supported). */
#define CDL_VGG_DX 1
#define CDL_VGG_DY 2
size_t cdl_vgg_scratch_floats(int P, int H, int W, int grads);
int cdl_vgg_forward(const float *x /*nullable*/, const float *y, int P, int H, int W, const float *const *w,
                    const float *const *b, int grads, float *feat /*nullable unless x is NULL*/,
                    float *loss /*1, nullable iff x is NULL*/, float *scratch, size_t scratch_floats, void *stream);
int cdl_vgg_backward(int P, int H, int W, const float *const *w, const float *const *b, int grads,
                     const float *g_loss /*1*/, float *dx /*nullable*/, float *dy /*nullable*/, float *scratch,
                     size_t scratch_floats, void *stream);

/* ---- ResidualBlock of CDLNetVideo(residual=True) -------------------------
 * model/net.py:105-120, applied to the code after every iteration (net.py:199-207):
 *     h = relu(conv1(x)),  out = relu(conv2(h) + x),   conv*: Conv3d(M, M, P, stride 1, padding P/2, bias=False)
 * g: a geometry with C == M (the block's channels), unit strides, (D,H,W) the code extents; w1, w2 (M,M,Pd,Ph,Pw).
 * forward writes h (kept for the reverse pass) and out; backward takes g_out = dL/dout and writes dx, dw1, dw2,
 * using dh (code-sized scratch).  x, h, out, dh, dx are (N,M,D,H,W).  scratch: cdl_residual_scratch_floats(g). */
size_t cdl_residual_scratch_floats(const cdl_geom *g);
int cdl_residual_forward(const cdl_geom *g, const float *x, const float *w1, const float *w2, float *h, float *out,
                         float *scratch, size_t scratch_floats, void *stream);
int cdl_residual_backward(const cdl_geom *g, const float *x, const float *h, const float *out, const float *w1,
                          const float *w2, const float *g_out, float *dx, float *dw1, float *dw2, float *dh,
                          float *scratch, size_t scratch_floats, void *stream);

/* ---- whole sweeps of the shape-generic loop in one call ------------------------------------------
 * The same launches as K x (cdl_synthesis, cdl_analysis | cdl_analysis_prox) + the final synthesis,
 * resp. the reverse sweep (cdl_tau_grad | cdl_prox_csr_bwd, cdl_synthesis, 2 x cdl_wgrad, cdl_analysis
 * per iteration), enqueued from C: single frames and crops are launch-bound, a host round trip per
 * launch would dominate.  Pointer tables are HOST arrays of device pointers.
 * Forward (net.py:76-92 / 192-212 / 426-463 / 525-568): tau (K,N,M) thresholds (CSR: lam); z_prev NULL =
 * plain ST loop, else the CSR map with gam1 (K,N,M) [and z_after, gam2]; z[k] receives z_{k+1}, r[k]
 * receives r_{k+1} (k < K-1), u[k] (CSR, nullable table) receives u_k; entries may alias ping-pong
 * buffers when nothing is kept, as long as z[k] != z[k-1].  xp receives D z_K.  scratch (nullable):
 * cdl_ista_scratch_floats(g) floats.
 * Backward: z, r, u as saved by the forward; g_xp = dL/d(D z_K) and / or g_z = dL/dz_K; writes dA[k],
 * dB[k], dt (K,2,M) [, dg1, dg2 (K,2,M)], accumulates gz_prev / gz_after (nullable); gbuf0, gbuf1 fat
 * scratch, q thin scratch, scratch as above (required).  The gradients of the data (both NULL: neither is computed):
 *     dyp  (thin, as yp; nullable):  dL/dyp = sum_k A_k^T du_k  (u_0 = A_0 yp, u_k = z_k - A_k(mask B_k z_k - yp))
 *     dtau (K,N,M; nullable):        dL/dtau[k,n,m], the per-sample threshold gradients (dL/dc = sum t[k,1,m] dtau);
 *                                    with z_prev (K,3,N,M): those of lam, gam1, gam2 (cdl_prox_csr_bwd's dsum_n)
 * Noise-level map (all NULL: none): cmap (N, code pixels) and tslope (K,M) = t[:,1,:] as in cdl_analysis,
 * tau then holding t[k,0,m] for every sample; in the reverse sweep cmap takes the place of c (c and dtau must be NULL) and
 *     dcmap (N, code pixels; nullable): dL/dcmap = sum_k cdl_sigma_grad(du_k, z_{k+1}, tslope[k])
 * With z_prev tslope holds (K,3,M): the slopes of lam, gam1, gam2 of every iteration in this order
 * (the third plane unread without z_after), tau / gam1 / gam2 (forward) resp. lam / gam1 / gam2 (reverse) the constant
 * parts t[k,0,m], g1[k,0,m], g2[k,0,m] for every sample; dt / dg1 / dg2 receive [sum s, sum cmap*s] and dcmap the sum over
 * the iterations of cdl_prox_csr_bwd's map gradient. */
size_t cdl_ista_scratch_floats(const cdl_geom *g);
int cdl_ista_forward(const cdl_geom *g, int K, const float *yp, const float *mask /*nullable*/,
                     const float *tau, const float *z_prev /*nullable*/, const float *z_after /*nullable*/,
                     const float *gam1 /*nullable*/, const float *gam2 /*nullable*/,
                     const float *const *wA, const float *const *wB, float *const *z, float *const *r,
                     float *const *u /*nullable*/, float *xp, float *scratch, size_t scratch_floats,
                     const float *cmap /*nullable*/, const float *tslope /*K*M or K*3*M, nullable*/, void *stream);
int cdl_ista_backward(const cdl_geom *g, int K, const float *yp, const float *mask /*nullable*/,
                      const float *c /*N, nullable*/, const float *z_prev /*nullable*/,
                      const float *z_after /*nullable*/, const float *lam, const float *gam1, const float *gam2,
                      const float *const *wA, const float *const *wB, const float *const *z,
                      const float *const *r, const float *const *u /*CSR*/, const float *g_xp /*nullable*/,
                      const float *g_z /*nullable*/, float *const *dA, float *const *dB, float *dt,
                      float *dg1 /*CSR*/, float *dg2 /*CSR f2*/, float *gz_prev /*nullable*/,
                      float *gz_after /*nullable*/, float *gbuf0, float *gbuf1, float *q, float *scratch,
                      size_t scratch_floats, float *dyp /*nullable*/, float *dtau /*K*N*M or K*3*N*M, nullable*/,
                      const float *cmap /*nullable*/, const float *tslope /*K*M or K*3*M, nullable*/, float *dcmap /*nullable*/,
                      void *stream);

/* ---- forward-mode tangent of the plain loop at the primal's supports ----
 * With G_k = [zgate[k] != 0] (zgate[k] = z_{k+1} of the primal) and a direction vp in the padded observation:
 *   zd_1 = G_0 (A_0 vp),  rd_k = mask B_k zd_k - vp,  zd_{k+1} = G_k (zd_k - A_k rd_k),  xdp = B_0 zd_K
 * -- no threshold appears.  The launches of cdl_ista_forward with cdl_analysis_rev as the gated step.  zd: K code
 * buffers, rd: K-1 thin ones (consecutive entries must differ; two each suffice when nothing is kept).  dt_scratch: 2*M
 * floats nobody reads; scratch: cdl_ista_scratch_floats(g). */
int cdl_tangent_forward(const cdl_geom *g, int K, const float *vp, const float *mask /*nullable*/,
                        const float *const *wA, const float *const *wB, const float *const *zgate, float *const *zd,
                        float *const *rd, float *xdp, float *dt_scratch, float *scratch, size_t scratch_floats,
                        void *stream);
/* Its reverse sweep (the tangent net is linear in vp with the gates fixed): dA[k], dB[k] of a loss with dL/dxdp = g_xp --
 * cdl_ista_backward's plain branch with the supports taken from zgate and the operands from the tangent sweep; no
 * threshold and no data gradient.  g_zd (nullable) = dL/dzd_K, added before the last gate.  gbuf0, gbuf1: code-sized;
 * q: thin. */
int cdl_tangent_backward(const cdl_geom *g, int K, const float *vp, const float *mask /*nullable*/,
                         const float *const *wA, const float *const *wB, const float *const *zgate,
                         const float *const *zd, const float *const *rd, const float *g_xp,
                         const float *g_zd /*nullable*/, float *const *dA, float *const *dB, float *gbuf0, float *gbuf1,
                         float *q, float *dt_scratch, float *scratch, size_t scratch_floats, void *stream);

/* ---- forward-mode tangent of the CSR loop at the primal's gates ----
 * u[k] = u_k of the primal (cdl_ista_forward's table), lam / gam1 / gam2 (K,N,M) the primal's; zd_prev / zd_after (nullable)
 * the tangents of the neighbour codes:
 *   ud_0 = A_0 vp,  rd_k = mask B_k zd_k - vp,  ud_k = zd_k - A_k rd_k,  zd_{k+1} = Jprox_k(ud_k; zd_prev, zd_after),
 *   xdp = B_0 zd_K.
 * Per iteration cdl_synthesis + cdl_analysis_prox_tangent.  zd: K code buffers,
 * rd: K-1 thin ones (two each suffice when nothing is kept).  The reverse sweep is cdl_ista_backward's CSR branch with
 * yp -> vp, z -> zd, r -> rd, the primal's u / lam / gam*, c = NULL: gz_prev / gz_after then receive dL/dzd_prev, dL/dzd_after
 * and dt / dg1 / dg2 sums nobody reads (the gates are piecewise constant: no threshold gradient through the tangent).
 * Noise-level map (both NULL: none): cmap (N, code pixels) with tslope (K,3,M) as in cdl_ista_forward's
 * CSR branch, lam / gam1 / gam2 the constant parts; the reverse sweep takes the same cmap / tslope, dcmap = NULL. */
int cdl_csr_tangent_forward(const cdl_geom *g, int K, const float *vp, const float *mask /*nullable*/,
                            const float *z_prev, const float *z_after /*nullable*/, const float *lam,
                            const float *gam1, const float *gam2 /*nullable*/, const float *zd_prev /*nullable*/,
                            const float *zd_after /*nullable*/, const float *const *wA, const float *const *wB,
                            const float *const *u, float *const *zd, float *const *rd, float *xdp, float *scratch,
                            size_t scratch_floats, const float *cmap /*nullable*/,
                            const float *tslope /*K*3*M, nullable*/, void *stream);

/* model/solvers.py:24-28 (uball_project) applied by net.py:72-73,189-190: every filter
 * (consecutive `flen` floats) with l2 norm > 1 is scaled onto the unit sphere, in place, for `nbanks` banks of identical
 * shape (w: HOST array of device pointers) in one launch per 64 banks: net.py:72-73 projects A[k] and B[k] for every k. */
int cdl_project_filter_banks(float *const *w, int nbanks, int nfilters, int flen, void *stream);

/* model/gabor.py:7-28,46-51 (gabor_kernel, get_filter): w[m,c,i,j] = sum_o alpha[o,m,c] *
 * exp(-(a0*(i-x0))^2 - (a1*(j-x0))^2) * cos(sgn*(w00*(i-x0) + w01*(j-x0) + psi)),
 * x0=(P-1)/2, sgn=-1 for the analysis ("transpose") filter.  alpha (O,M,C), a,w0 (O,M,C,2), psi (O,M,C), w (M,C,P,P).
 * Every bank of a net in ONE launch (GDLNet.forward re-synthesises its 2K banks per call, net.py:659-675):
 * bank k reads alpha[k], a[k], w0[k], psi[k] (aliased pointers are fine: shared parameters, net.py:607-622), writes
 * w[k]; transpose[k] != 0 selects the analysis filter.  _bwd: grads[k] receives the block
 * [dalpha (order*M*C) | da (2*order*M*C) | dw0 (2*order*M*C) | dpsi (order*M*C)] for upstream dw[k] (zeros when
 * dw[k] is NULL); the caller sums the blocks of aliased parameters. */
int cdl_gabor_filter_banks(int nbanks, const float *const *alpha, const float *const *a, const float *const *w0,
                           const float *const *psi, const int *transpose, float *const *w, int order, int M, int C,
                           int P, void *stream);
int cdl_gabor_filter_banks_bwd(int nbanks, const float *const *alpha, const float *const *a, const float *const *w0,
                               const float *const *psi, const int *transpose, const float *const *dw,
                               float *const *grads, int order, int M, int C, int P, void *stream);

/* OR-ed into the `precision` argument of cdl_fused2d_iter_fwd / _stage_bwd / _wgrad: walk the tiles from
 * the last to the first.  Stage results are identical; the filter gradients' per-workgroup partial sums
 * are grouped differently (still deterministic).  The whole-sweep entry points alternate it per launch. */
#define CDL_TILES_REVERSED 16

/* Layouts of the fat (code-like) operands of the fused path, OR-ed into `precision` as well:
 *   CDL_LAY_NCHW   (N, M, H, W) fp32 -- the reference's layout; what leaves or enters a sweep (z_K, user gradients)
 *   CDL_LAY_BLK    pixel-blocked fp32 [n][y][ceil(W/32)][M/4][32 px][4 ch]: 16 contiguous bytes per lane and
 *                  register quad, 8 KiB contiguous per 32-pixel row block (measured 5.65 vs 5.08 TB/s for a pure
 *                  load -> store stream of the cfg2 code tensor, tools/probes/probe_stream.hip); for tensors that
 *                  stay INSIDE a sweep (z_1..z_{K-1}, du_k).  Bit-identical values to CDL_LAY_NCHW.
 *   CDL_LAY_BLK16  the same blocking with bf16 elements: opt-in reduced-precision STORAGE (half the fat bytes;
 *                  arithmetic and accumulation stay as `precision` says; the 1e-5 parity gate does not apply).
 * cdl_fused2d_iter_fwd / _stage_bwd: CDL_LAYOUT_IN = zin / base, CDL_LAYOUT_OUT = zout / du_out (pairs: equal
 * layouts, or NCHW on exactly one side).  cdl_fused2d_wgrad: CDL_LAYOUT_IN = X0 and X1.  cdl_fused2d_forward /
 * _backward: CDL_LAYOUT_IN = the layout of z[0..K-2] and of the du ping-pong buffers (z[K-1], g_z: NCHW). */
#define CDL_LAY_NCHW  0
#define CDL_LAY_BLK   1
#define CDL_LAY_BLK16 2
/* cdl_fusedg_* on the strip kernel's shapes (one image channel, stride 1 / 2, M <= 192) only: row-strip channel-major
 * fp32 [n][code row][ceil(Wz/32)][M][32 columns] -- what a wave moves per code row is one contiguous run of M * 128
 * bytes.  Same values as CDL_LAY_NCHW; for the codes that stay inside a sweep. */
#define CDL_LAY_RSC   3
#define CDL_LAYOUT_IN(l)  ((l) << 5)
#define CDL_LAYOUT_OUT(l) ((l) << 7)
/* cdl_fusedg_* only, OR-ed into `precision` beside the bits above: one threshold row per (sample, depth) PLANE instead of
 * one per sample -- one noise level per frame of a clip.  Every work item of the tile kernel and of
 * the grouped strip kernel lies in one plane (n, zd) and loads its thresholds once, so the bit only changes which row that
 * load reads: n * D + zd instead of n.  With the bit set
 *   cdl_fusedg_iter_fwd            tau is (N*D, M)
 *   cdl_fusedg_forward             tau is (K, N*D, M)
 *   cdl_fusedg_backward            c is (N*D): dt[k,1,m] = sum_{n,d} c[n,d] * (sum over the tiles of plane (n,d));
 *                                  dtau (nullable) is (K, N*D, M).  Same partial rows in the same order as without the bit.
 *   cdl_fusedg_stage_bwd           unchanged (the reverse stage reads no threshold); cdl_fusedg_tangent does not take it
 * and the strip kernel proper (2-D, D == 1: CDL_PLAN_STRIP geometries) returns CDL_EINVAL.  With the bit clear every call
 * enqueues exactly the launches it enqueued before the bit existed. */
#define CDL_TAU_PER_PLANE 512

/* ==== fused MFMA path (cdl_fused2d.hip): 2-D, C = 1, stride 1, odd P <= 7, M in {32, 64} =========
 * One launch per unrolled iteration replaces the whole body of net.py:87
 *     z = ST(z - A_k(mask*B_k(z) - yp), tau_k)
 * with the fusion boundary moved to the one-channel residual:
 *     cdl_fused2d_iter_fwd :  r_k, z_k  ->  z_{k+1} = ST(z_k + sgn * A_k r_k, tau_k)   (fat, written once)
 *                                           patches = partial B_next z_{k+1}           (thin)
 *     cdl_fused2d_assemble :  patches  ->  r_{k+1} = mask * (B_next z_{k+1}) - yp      (thin)
 * For k = 0 pass r = yp, zin = NULL, sgn = +1 (net.py:85); for k >= 1 sgn = -1.  For the last
 * iteration B_next is D = B_0 and assemble(mask = sub = NULL) yields D z_K (net.py:90).
 * precision: 0 = split-bf16 (hi+lo operands, 3 MFMAs per product, fp32-grade), 1 = plain bf16, 2 = split-bf16 with all
 * four products (exact fp32 products; for objectives that difference two forward passes, e.g. MC-SURE). */
int cdl_fused2d_supported(const cdl_geom *g);              /* 1 if this geometry has a fused kernel */
size_t cdl_fused2d_frag_bytes(int M);                      /* bytes of one prepared (A_k, B_next) pair */
size_t cdl_fused2d_patch_floats(const cdl_geom *g);        /* floats in the patch workspace */
size_t cdl_fused2d_code_bytes(const cdl_geom *g, int layout);   /* bytes of one code tensor in CDL_LAY_* */
/* fp32 filters (M,1,P,P) -> bf16 hi/lo MFMA operand fragments for one launch (A_k with B_next). */
int cdl_fused2d_prep(const float *wA, const float *wB, void *frags, int M, int P, void *stream);
/* map_out (nullable, cdl_fused2d_map_words(g) words): support / sign bit planes of z_{k+1} for the reverse
 * sweep (2 bits per code element, written by the same launch).
 * A noise-level map -- cmap (N,1,H,W) with tslope (M), both or neither (a mix is CDL_EINVAL): the
 * threshold of code element (n, m, y, x) is tau[n,m] + cmap[n,y,x] * tslope[m], product rounded before the sum as on the
 * generic tier (cdl_analysis), tau then holding t[k,0,m] for every sample.  Split-bf16 x3 arithmetic and the layouts
 * CDL_LAY_NCHW / CDL_LAY_BLK only (anything else with a map: CDL_EUNSUPPORTED); cmap needs float alignment only.  With
 * both NULL the call enqueues exactly the launch it enqueued without these arguments. */
int cdl_fused2d_iter_fwd(const cdl_geom *g, const float *r, const float *zin /*nullable*/,
                         const float *tau /*N*M*/, const void *frags, float sgn, float *zout,
                         float *patches, unsigned *map_out /*nullable*/, int precision,
                         const float *cmap /*nullable*/, const float *tslope /*nullable*/, void *stream);
/* The map of a code tensor, (N,4,H,W) 32-bit words: plane 2h holds [z != 0], plane 2h+1 the sign bit, bit
 * 16R + v of a word = channel 32R + 8(v>>2) + 4h + (v&3) of that pixel (the MFMA accumulator layout).  The
 * reverse stage reads it instead of the fat z_{k+1}: 16 B per pixel against 4*M.  cdl_fused2d_support_map
 * builds it from a tensor for callers that did not get it from cdl_fused2d_iter_fwd. */
size_t cdl_fused2d_map_words(const cdl_geom *g);
int cdl_fused2d_support_map(const cdl_geom *g, const float *z, unsigned *map, void *stream);
/* out = (mask ? mask : 1) * alpha * (sum of the overlapping patches) - (sub ? sub : 0), and (acc non-NULL) the plain
 * sum S of the patches, unmasked and unscaled: acc = S (acc_add 0) or acc += S.  S comes from the same summation as
 * `out`, which does not depend on whether acc is given.  out may be NULL only when acc is set (acc only). */
int cdl_fused2d_assemble(const cdl_geom *g, const float *patches, const float *mask /*nullable*/,
                         const float *sub /*nullable*/, float alpha, float *out /*nullable iff acc*/,
                         float *acc /*nullable*/, int acc_add, void *stream);

/* ---- fused reverse sweep (what loss.backward() does through ATen in the reference, train.py:98) ----
 * One stage per iteration k = K-1 .. 0, same kernel skeleton as the forward launch:
 *     g_{k+1} = base + corr(thin ; W1)          base = du_{k+1} (or dL/dz_K, nullable), thin = q_{k+1} (or
 *                                               dL/d(D z_K)), W1 = B_{k+1} (or B_0)
 *     du_k    = [z_{k+1} != 0] * g_{k+1}        support and sign from `map` -> du_out (fat, written once)
 *     dtau    : per-workgroup partials of -sum sign(z_{k+1}) * du_k     -> dtau_partial (tiles x M)
 *     patches : partial W2^T du_k (W2 = A_k)    -> cdl_fused2d_assemble(alpha = -1, mask) gives q_k
 * frags = cdl_fused2d_prep(W1, W2).  do_synth = 0 for k = 0 (no q_0 is needed). */
size_t cdl_fused2d_tiles(const cdl_geom *g);               /* workgroups (= dtau_partial rows) per launch */
/* Floats of the dtau_partial buffer of cdl_fused2d_stage_bwd / _backward: cdl_fused2d_tiles(g) * M, and twice that when the
 * call passes a noise-level map (with_map != 0: the map-weighted partials sit behind the plain ones).  A caller that adds
 * cmap to an existing call MUST resize the buffer with this: the stage writes both arrays. */
size_t cdl_fused2d_dtau_partial_floats(const cdl_geom *g, int with_map);
/* r2, dA, workspace (all three set, or all three NULL; a mix is CDL_EINVAL): the analysis-filter gradient of the
 * iteration rides in the stage (what autograd of net.py:87 computes from du_k and r_k): dA = alpha * sum_px du_out (x)
 * im2col(r2) -- cdl_fused2d_wgrad's product, taken from the stage's registers instead of a second fat read of du_out.
 * du_out / patches / dtau_partial do not depend on whether it rides; workspace: cdl_fused2d_wgrad_workspace_floats(g).
 * The whole-sweep entry point cdl_fused2d_backward uses it (5.1 instead of 6.1 fat passes per iteration;
 * CDL_FUSED_DA=0 restores the two-launch form for A/B runs).
 * A noise-level map -- the forward's cmap and tslope (both or neither), as cdl_fused2d_iter_fwd's: du_out, patches and the
 * partials in dtau_partial are what they are without it (the stage gates on `map`, it reads no threshold); dtau_partial
 * then holds cdl_fused2d_dtau_partial_floats(g, 1) floats, TWO arrays of cdl_fused2d_tiles(g) * M, and the second receives the map-weighted partials
 * -sum cmap * sign(z_{k+1}) * du_k (cdl_fused2d_dtau_reduce's dtau_partial_w).  dcmap (nullable, only with a map; (N,1,H,W),
 * float alignment): dL/dcmap of this iteration, sum_m tslope[m] * (-sign(z_{k+1}) du_k)[m] per pixel -- written
 * (dcmap_add = 0) or added to what dcmap holds (dcmap_add != 0: every reverse iteration after the first). */
int cdl_fused2d_stage_bwd(const cdl_geom *g, const float *thin, const float *base /*nullable*/,
                          const unsigned *map /*of z_{k+1}*/, const void *frags, float *du_out, float *patches,
                          float *dtau_partial, int do_synth, const float *r2 /*(N,1,H,W), nullable*/, float alpha,
                          float *dA /*(M,1,P,P), nullable*/, float *workspace /*nullable*/, int precision,
                          const float *cmap /*nullable*/, const float *tslope /*nullable*/, float *dcmap /*nullable*/,
                          int dcmap_add, void *stream);
/* dt0[m] = sum over workgroups; dt1[m] = sum_n c[n] * (sum over the workgroups of image n); c nullable.
 * dtau_n (nullable) receives the per-image sums dtau_n[n,m] of the partial rows, tiles in order.
 * dtau_partial_w (nullable; together with c: CDL_EINVAL): the map-weighted partials of a reverse stage that ran with a
 * noise-level map; dt1[m] is then their sum over the workgroups, in dt0's order. */
int cdl_fused2d_dtau_reduce(const cdl_geom *g, const float *dtau_partial, const float *c /*N*/, float *dt0 /*M*/,
                            float *dt1 /*M*/, float *dtau_n /*N,M, nullable*/, const float *dtau_partial_w /*nullable*/,
                            void *stream);

/* Filter gradients on the matrix cores: up to two independent reductions per launch
 *     dw_a[m,i,j] = alpha_a * sum_{n,y,x} Xa[n,m,y,x] * Ta[n,y-p+i,x-p+j]     (a = 0, 1; either may be absent)
 * e.g. (Xa,Ta,alpha) = (du_k, r_k, -1) -> dA_k and (z_k, q_k, +1) -> dB_k.  Two-stage and deterministic:
 * per-workgroup partial sums in `workspace`, then a fixed-order reduction.  workspace_floats() floats: two regions of
 * partials, so that cdl_fused2d_backward can hold dA_k's and dB_k's until its one reduction launch per iteration (a
 * stand-alone call uses the first). */
size_t cdl_fused2d_wgrad_workspace_floats(const cdl_geom *g);
int cdl_fused2d_wgrad(const cdl_geom *g, const float *X0, const float *T0, float alpha0, float *dw0,
                      const float *X1, const float *T1, float alpha1, float *dw1,
                      float *workspace, int precision, void *stream);

/* ---- whole sweeps in one call (same launches as above, enqueued from C: no per-launch host cost) ----
 * Pointer tables are HOST arrays of device pointers.  Forward: z[k] receives z_{k+1} (K entries; entries
 * may alias two ping-pong buffers when nothing is kept for training, as long as z[k] != z[k-1]); r[k]
 * receives r_{k+1} for k < K-1 (same aliasing rule); maps (nullable table) receives the bit map of z_{k+1};
 * xp receives D z_K.  frags: K * cdl_fused2d_frag_bytes(M) bytes (every pair is prepared up front, one launch).
 * Backward (net.py forward lines in reverse): z[k] = z_{k+1}, r[k] = r_{k+1}, maps[k] as saved by the forward,
 * g_xp = dL/d(D z_K), g_z = dL/dz_K or NULL; writes dA[k], dB[k] (filter shapes) and dt (K,2,M);
 * du0/du1 fat scratch (contents unspecified on return: when dA_0 rides in the last stage, du_0 is never written),
 * q thin scratch, dtau_partial (tiles x M), wgrad_ws (workspace_floats).
 * Per iteration four launches: stage (with dA_k's partials), assemble, dB_k's partials, and ONE reduction of dA_k, dB_k
 * and dt[k] -- each summed in the order of its stand-alone entry point (bit-identical to them).
 * The gradients of the data, as cdl_ista_backward's (both NULL: neither is computed): dyp (thin, nullable) receives
 * sum_k A_k^T du_k -- the unmasked sum each assemble already forms, plus the k = 0 synthesis half (its stage then runs
 * with do_synth = 1) and one assemble into dyp only; dtau (K,N,M, nullable) the per-image threshold gradients.
 * A noise-level map (both sweeps; cmap (N,1,H,W) with tslope (K,M), both or neither): the stage launches become their map
 * forms (see cdl_fused2d_iter_fwd / _stage_bwd), the launch count stays.  The reverse sweep then takes c = NULL and
 * dtau = NULL (either with a map: CDL_EINVAL), dtau_partial of cdl_fused2d_dtau_partial_floats(g, 1) floats, writes dt[k,1,m] as the sum of the weighted
 * partials, and fills dcmap (nullable) with dL/dcmap.  All three NULL: exactly the launches of the sweep without a map. */
int cdl_fused2d_forward(const cdl_geom *g, int K, const float *yp, const float *mask /*nullable*/,
                        const float *tau /*K,N,M*/, const float *const *wA, const float *const *wB,
                        float *const *z, float *const *r, unsigned *const *maps /*nullable*/, float *xp,
                        void *frags, float *patches, int precision, const float *cmap /*nullable*/,
                        const float *tslope /*K,M, nullable*/, void *stream);
int cdl_fused2d_backward(const cdl_geom *g, int K, const float *yp, const float *mask /*nullable*/,
                         const float *c /*N, nullable*/, const float *const *wA, const float *const *wB,
                         const float *const *z, const float *const *r, const unsigned *const *maps,
                         const float *g_xp, const float *g_z /*nullable*/, float *const *dA, float *const *dB,
                         float *dt, float *du0, float *du1, float *q, void *frags, float *patches,
                         float *dtau_partial, float *wgrad_ws, int precision, float *dyp /*nullable*/,
                         float *dtau /*K*N*M, nullable*/, const float *cmap /*nullable*/,
                         const float *tslope /*K,M, nullable*/, float *dcmap /*nullable*/, void *stream);

/* Tangent sweep on the fused 2-D kernels: per iteration one reverse-stage launch with the FORWARD's
 * prepared pair (A_k, B_{k+1}), base = zd_k, thin = -rd_k and maps[k] = the primal's bit map of z_{k+1}, then one assemble
 * (alpha = -1, sub = nvp = -vp) that writes nrd[k] = -rd_{k+1}.  zd[0..K-2] in CDL_LAYOUT_IN(precision) (NCHW or blocked
 * fp32), zd[K-1] NCHW; nrd: K-1 thin buffers holding the NEGATED residuals.  dtau_partial: cdl_fused2d_tiles(g) * M floats
 * nobody reads.  Buffers as cdl_fused2d_forward's. */
int cdl_fused2d_tangent(const cdl_geom *g, int K, const float *vp, const float *nvp, const float *mask /*nullable*/,
                        const float *const *wA, const float *const *wB, const unsigned *const *maps, float *const *zd,
                        float *const *nrd, float *xdp, void *frags, float *patches, float *dtau_partial, int precision,
                        void *stream);

/* ==== fused MFMA path for the other shapes (cdl_fusedg.hip): any C, 2-D / 3-D, unit stride, square planes ====
 * P in {3,5,7}, odd Pd with C*Pd in {1,3,5,7}, M <= 64 -- CDLNetVideo.forward's loop body (net.py:204-207) and
 * CDLNet.forward's (net.py:86-87) with C = 3 + mask (JDD).  Same fusion boundary and call structure as the
 * cdl_fused2d_* family above: one launch per iteration takes (r_k thin, z_k fat) to (z_{k+1} fat, patches of
 * B_next z_{k+1}); cdl_fusedg_assemble sums the patches over tiles and depth taps and applies alpha, mask, -sub.
 * Codes in the reference's (N,M,D,H,W) layout; map = (N,4,D,H,W) words as cdl_fused2d_support_map describes.
 * precision: 0 (split-bf16 x3), or 2 (split-bf16 x4: all four products) on the tile kernel; CDL_TILES_REVERSED may be
 * OR-ed in. */
int cdl_fusedg_supported(const cdl_geom *g);
/* Profiling hook (not part of the reference surface): while buf != NULL every cdl_fusedg stage launch records
 * s_memtime stamps of its workgroup 0 into buf[8 waves][256] (16 KB of device memory).  NULL switches it off. */
int cdl_fusedg_set_timeline(void *buf);
size_t cdl_fusedg_frag_bytes(const cdl_geom *g);           /* bytes of one prepared (A_k, B_next) pair */
size_t cdl_fusedg_patch_floats(const cdl_geom *g);
size_t cdl_fusedg_tiles(const cdl_geom *g);                /* workgroup tiles (= dtau_partial rows) per launch */
size_t cdl_fusedg_map_words(const cdl_geom *g);
/* Layout for the codes that stay inside a sweep (z[0..K-2], the du buffers): CDL_LAY_RSC where a strip kernel takes the
 * geometry and -- when a reverse sweep will follow (training != 0) -- the matrix-core filter-gradient kernel does too,
 * CDL_LAY_NCHW otherwise; floats of one code tensor in a
 * layout.  cdl_fusedg_forward / _backward take it as CDL_LAYOUT_IN(layout) in `precision`; the single-stage entry points
 * take CDL_LAYOUT_IN (zin / base) and CDL_LAYOUT_OUT (zout / du_out). */
int cdl_fusedg_code_layout(const cdl_geom *g, int training);
size_t cdl_fusedg_code_floats(const cdl_geom *g, int layout);
int cdl_fusedg_prep(const cdl_geom *g, const float *wA, const float *wB, void *frags, void *stream);
int cdl_fusedg_iter_fwd(const cdl_geom *g, const float *r, const float *zin /*nullable*/, const float *tau /*N,M*/,
                        const void *frags, float sgn, float *zout, float *patches, unsigned *map_out /*nullable*/,
                        int precision, void *stream);
int cdl_fusedg_stage_bwd(const cdl_geom *g, const float *thin, const float *base /*nullable*/, const unsigned *map,
                         const void *frags, float *du_out, float *patches /*nullable iff !do_synth*/,
                         float *dtau_partial /*tiles,M*/, int do_synth, int precision, void *stream);
/* As cdl_fused2d_assemble / cdl_fused2d_dtau_reduce, optional outputs included (every route: tile, strip and grouped
 * strip kernels) */
int cdl_fusedg_assemble(const cdl_geom *g, const float *patches, const float *mask /*nullable*/,
                        const float *sub /*nullable*/, float alpha, float *out /*nullable iff acc*/,
                        float *acc /*nullable*/, int acc_add, void *stream);
int cdl_fusedg_dtau_reduce(const cdl_geom *g, const float *dtau_partial, const float *c /*N, nullable*/, float *dt0,
                           float *dt1, float *dtau_n /*N,M, nullable*/, void *stream);
/* The same reduction with the (sample, depth) plane as the "sample" (CDL_TAU_PER_PLANE): c is (N*D), dt1[m] =
 * sum_{n,d} c[n,d] * (sum over the tiles of plane (n,d)), dtau_nd (nullable) the per-plane sums (N*D, M).  dt0 is
 * cdl_fusedg_dtau_reduce's bit for bit; CDL_EINVAL where the strip kernel proper takes the geometry. */
int cdl_fusedg_dtau_reduce_planes(const cdl_geom *g, const float *dtau_partial, const float *c /*N*D, nullable*/,
                                  float *dt0, float *dt1, float *dtau_nd /*N*D,M, nullable*/, void *stream);
/* Whole sweeps (arguments as cdl_fused2d_forward / _backward, the data gradients dyp / dtau included).  The reverse sweep takes the filter gradients
 * dA_k = -du_k (x) r_k, dB_k = z_k (x) q_k from cdl_wgrad: wgrad_ws = cdl_wgrad_workspace_floats(g) floats. */
int cdl_fusedg_forward(const cdl_geom *g, int K, const float *yp, const float *mask /*nullable*/, const float *tau,
                       const float *const *wA, const float *const *wB, float *const *z, float *const *r,
                       unsigned *const *maps /*nullable*/, float *xp, void *frags, float *patches, int precision,
                       void *stream);
int cdl_fusedg_backward(const cdl_geom *g, int K, const float *yp, const float *mask /*nullable*/,
                        const float *c /*nullable*/, const float *const *wA, const float *const *wB,
                        const float *const *z, const float *const *r, const unsigned *const *maps, const float *g_xp,
                        const float *g_z /*nullable*/, float *const *dA, float *const *dB, float *dt, float *du0,
                        float *du1, float *q, void *frags, float *patches, float *dtau_partial, float *wgrad_ws,
                        size_t wgrad_ws_floats, int precision, float *dyp /*nullable*/,
                        float *dtau /*K*N*M, nullable*/, void *stream);

/* cdl_fused2d_tangent for the shapes of this family (tile and strip kernels); codes in the reference's layout only
 * (precision carries no layout bits). */
int cdl_fusedg_tangent(const cdl_geom *g, int K, const float *vp, const float *nvp, const float *mask /*nullable*/,
                       const float *const *wA, const float *const *wB, const unsigned *const *maps, float *const *zd,
                       float *const *nrd, float *xdp, void *frags, float *patches, float *dtau_partial, int precision,
                       void *stream);

/* Per-kernel timing inside the fused sweeps: cdl_fused2d_timing(1) starts collecting HIP-event pairs around
 * every forward stage (class 0; the k = 0 launch, which reads no code, is class 3), reverse stage (1) and
 * filter-gradient (2) launch of the sweeps on their own stream, cdl_fused2d_timing(0) stops; _read synchronises and returns the summed milliseconds and launch counts
 * per class.  For measurement (bench.py); off by default, no events are recorded then. */
int cdl_fused2d_timing(int enable);
int cdl_fused2d_timing_read(double *ms_sum /*4*/, int *count /*4*/);

#ifdef __cplusplus
}
#endif
#endif /* CDLNET_HIP_H */
