// The host loop of the fused forward and tangent sweeps (cdl_fused2d.hip, cdl_fusedg.hip): K stages in forward order, each
// followed by one assemble -- into r[k], the next stage's thin operand, or after the last stage into the image output.  No
// launch lives here: a launch is traced under the file it is written in.  (The reverse sweeps reduce differently: apart.)
//   stage(k, fk, thin, reversed, lay_in, lay_out) -> rc: iteration k on its fragments fk; `reversed`: snake order, every
//       second stage walks the tiles backwards.  The code it reads / writes is in `lay`, the first and last in `lay_edge`.
//   assemble(mask, sub, alpha, out) -> rc: out = mask * alpha * (overlap-sum of the stage's patches) - sub.
#pragma once
#include <cstddef>

template <class Stage, class Assemble>
int cdl_forward_order_sweep(int K, const void *frags, size_t frag_bytes, const float *thin0, const float *mask,
                            const float *sub, float alpha, float *const *r, float *out, bool snake, int lay, int lay_edge,
                            Stage stage, Assemble assemble)
{
    const float *thin = thin0;
    for (int k = 0; k < K; ++k) {
        const void *fk = static_cast<const char *>(frags) + (size_t)k * frag_bytes;
        int rc = stage(k, fk, thin, (k & 1) && snake, k ? lay : lay_edge, k < K - 1 ? lay : lay_edge);
        if (rc) return rc;
        if (k < K - 1) {
            rc = assemble(mask, sub, alpha, r[k]);
            thin = r[k];
        } else {
            rc = assemble(nullptr, nullptr, 1.0f, out);
        }
        if (rc) return rc;
    }
    return 0;
}
