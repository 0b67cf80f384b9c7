"""cva.functional.analysis_prox: the analysis with the CSR map in its epilogue as a differentiable
block, against the same computation composed from functional.analysis and functional.prox_csr / prox_csr_f2 with the
thresholds formed by torch.  Values bit for bit (the fused epilogue evaluates the composed expression); gradients at the
issue's tolerances: 1e-5 for tensors of the codes' or the image's size, 2e-5 for the reduced sums (thresholds, the map)."""
import pytest
import torch

from gpu_util import check

pytestmark = pytest.mark.gpu

KEYS = [((20, 22), 7, 2), ((20, 24), 5, 1)]         # the stride-padded 19 x 21 case (code grid 10 x 11), and unit stride


def inputs(sp, P, s, both, seed):
    gen = torch.Generator().manual_seed(seed)
    N, M = 2, 5
    zsp = tuple(d // s for d in sp)
    r = lambda shape, sc=1.0: (sc * torch.randn(shape, generator=gen)).cuda()
    code = lambda: (0.3 * torch.randn((N, M) + zsp, generator=gen) * (torch.rand((N, M) + zsp, generator=gen) > 0.5)).cuda()
    d = dict(x=r((N, 1) + sp), w=r((M, 1, P, P), 0.2), add=code(), zp=code(), wz=r((N, M) + zsp))
    if both:
        d["za"] = code()
    return d, gen, N, M, zsp


def run(fn, tensors):
    leaves = {k: v.clone().requires_grad_(True) for k, v in tensors.items()}
    z = fn(leaves)
    (z * leaves["wz"].detach()).sum().backward()
    return z.detach(), {k: v.grad for k, v in leaves.items() if k != "wz"}


def compare(tag, fused, composed, tensors, reduced):
    z, gf = run(fused, tensors)
    zr, gc = run(composed, tensors)
    assert torch.equal(z, zr), tag
    for k, ref in gc.items():
        assert gf[k] is not None and gf[k].shape == tensors[k].shape, (tag, k)      # in the shape given
        check(f"{tag} d{k}", gf[k], ref, 2e-5 if k in reduced else 1e-5)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("sp,P,s", KEYS)
@pytest.mark.parametrize("cshape", ["N", "1"])
def test_map_form(sp, P, s, both, cshape):
    """Every threshold a triple (t0, c, t1): the (cmap, slopes) form of the fused kernels."""
    import cdlnet_video_amd as cva
    F = cva.functional
    d, gen, N, M, zsp = inputs(sp, P, s, both, 70 + both + s)
    u = lambda shape, lo, hi: (lo + (hi - lo) * torch.rand(shape, generator=gen)).cuda()
    d["c"] = u(((N if cshape == "N" else 1), 1) + zsp, 10 / 255, 40 / 255)
    fams = ["l", "a"] + (["b"] if both else [])
    for f, hi in zip(fams, (0.1, 1.0, 1.0)):
        d[f + "0"] = u((1, M, 1, 1), 0.01, hi)                 # the constant part, (1,M,1,1)
        d[f + "1"] = u((M, 1, 1), 0.0, 2 * hi)                  # the slope, (M,1,1)
    za = lambda t: t["za"] if both else None

    def fused(t):
        trip = [(t[f + "0"], t["c"], t[f + "1"]) for f in fams]
        return F.analysis_prox(t["x"], t["w"], t["zp"], trip[0], trip[1], za(t), trip[2] if both else None, s, -1.0, t["add"])

    def composed(t):
        thr = [t[f + "0"] + t["c"] * t[f + "1"] for f in fams]
        uu = F.analysis(t["x"], t["w"], s, -1.0, t["add"])
        return F.prox_csr_f2(uu, t["zp"], t["za"], *thr) if both else F.prox_csr(uu, t["zp"], *thr)

    reduced = {"c"} | {f + i for f in fams for i in "01"}
    compare(f"analysis_prox map[{'f2' if both else 'f1'} c{cshape}] {sp}s{s}", fused, composed, d, reduced)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("sp,P,s", KEYS)
def test_row_form_and_broadcast_form(sp, P, s, both):
    """One threshold per (sample, channel) in mixed shapes and a number: the fused row form.  A threshold with spatial
    extent that is not a triple: the two-launch form."""
    import cdlnet_video_amd as cva
    F = cva.functional
    d, gen, N, M, zsp = inputs(sp, P, s, both, 80 + both + s)
    u = lambda shape, lo, hi: (lo + (hi - lo) * torch.rand(shape, generator=gen)).cuda()
    d["lam"], d["g1"] = u((N, M, 1, 1), 0.01, 0.2), u((M, 1, 1), 0.2, 1.2)
    za = lambda t: t["za"] if both else None
    g2 = 0.7 if both else None

    def fused(t):
        return F.analysis_prox(t["x"], t["w"], t["zp"], t["lam"], t["g1"], za(t), g2, s, 1.0, t["add"])

    def composed(t):
        uu = F.analysis(t["x"], t["w"], s, 1.0, t["add"])
        return F.prox_csr_f2(uu, t["zp"], t["za"], t["lam"], t["g1"], g2) if both else F.prox_csr(uu, t["zp"], t["lam"], t["g1"])

    tag = f"analysis_prox rows[{'f2' if both else 'f1'}] {sp}s{s}"
    compare(tag, fused, composed, d, {"lam", "g1"})
    no_add = lambda t: F.analysis_prox(t["x"], t["w"], t["zp"], t["lam"], t["g1"], za(t), g2, s)
    no_add_ref = lambda t: (F.prox_csr_f2(F.analysis(t["x"], t["w"], s), t["zp"], t["za"], t["lam"], t["g1"], g2) if both
                            else F.prox_csr(F.analysis(t["x"], t["w"], s), t["zp"], t["lam"], t["g1"]))
    compare(tag + " no add", no_add, no_add_ref, {k: v for k, v in d.items() if k != "add"}, {"lam", "g1"})
    d["lam"] = u((N, 1) + zsp, 0.01, 0.2)                       # spatial extent, no triple
    compare(tag + " spatial", fused, composed, d, {"lam", "g1"})


def test_refusals():
    import cdlnet_video_amd as cva
    F = cva.functional
    x, w = torch.randn(2, 1, 20, 24).cuda(), torch.randn(5, 1, 5, 5).cuda()
    z, c = torch.zeros(2, 5, 20, 24).cuda(), torch.rand(2, 1, 20, 24).cuda()
    t = torch.rand(5, 1, 1).cuda()
    with pytest.raises(ValueError):                  # a triple beside a plain threshold
        F.analysis_prox(x, w, z, (t, c, t), 0.5)
    with pytest.raises(ValueError):                  # two different maps
        F.analysis_prox(x, w, z, (t, c, t), (t, c.clone(), t))
    with pytest.raises(ValueError):                  # a constant part per sample: not t0[m] + c * t1[m]
        F.analysis_prox(x, w, z, (torch.rand(2, 5, 1, 1).cuda(), c, t), (t, c, t))
    with pytest.raises(ValueError):                  # a map that does not broadcast to the code grid
        F.analysis_prox(x, w, z, (t, c[:, :, :7], t), (t, c[:, :, :7], t))
    with pytest.raises(ValueError):
        F.analysis_prox(x, w, z, 0.1, 0.5, z)        # z_after without gamma2
    with torch.no_grad():                            # and nothing is kept without a gradient to form
        assert F.analysis_prox(x, w, z, (t, c, t), (t, c, t)).shape == z.shape
