"""cva.functional on the device: the building blocks of the nets as differentiable functions.  The
reference in every case is torch autograd through the oracle's functions, which broadcast a threshold or a sigma map as
the reference's own torch expressions do.

Tolerances (max-norm relative, gpu_util.check) are those of tests/test_gpu_sigmamap.py and tests/test_gpu_csr.py for the
same quantities: outputs 1e-5; gradients through the matrix-core kernels 5e-5 on the default tier and 1e-5 under
precision_scope("fp32"); the pointwise maps' gu and per-element threshold gradients 1e-6, their neighbour-code gradients
1e-5, their reduced threshold gradients 2e-5."""
import pytest
import torch

from gpu_util import check, load_golden, log
from oracle import cdl_oracle as O

pytestmark = pytest.mark.gpu

XTOL = 1e-5
TIER_TOL = {"default": 5e-5, "fp32": 1e-5}
GU_TOL = 1e-6
EL_TOL = 1e-6
NB_TOL = 1e-5
RED_TOL = 2e-5
CSR_GTOL = 2e-4          # tests/test_gpu_csr.py GTOL: the CSR nets' gradients against another evaluation of the same net


class _tier:
    """precision_scope("fp32") or nothing."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from cdlnet_video_amd import loop
        self.scope = loop.precision_scope("fp32") if self.name == "fp32" else None
        if self.scope:
            self.scope.__enter__()

    def __exit__(self, *exc):
        if self.scope:
            self.scope.__exit__(*exc)
        return False


def _leaf(t):
    return t.detach().cpu().clone().requires_grad_(True)


def _dev_leaf(t):
    return t.detach().cuda().requires_grad_(True)


def _pad(P):
    return tuple(p // 2 for p in P)


# ------------------------------------------------------------------------------------------ 1. linear operators
#        x shape             M   P          s  mask
LINEAR = [((4, 1, 200, 64), 16, (7, 7), 1, None),          # matrix-core analysis
          ((4, 1, 200, 64), 40, (5, 5), 1, None),          # two channel tiles
          ((2, 1, 33, 31), 16, (7, 7), 1, None),           # tiled fp32
          ((2, 1, 34, 32), 16, (7, 7), 2, None),
          ((2, 3, 24, 28), 32, (7, 7), 1, "bayer"),        # Bayer mask in `synthesis`
          ((1, 1, 6, 24, 40), 16, (3, 5, 5), 1, None),
          ((2, 1, 8, 20, 12), 5, (9, 9, 5), 2, None)]
LINEAR_IDS = [f"{'x'.join(map(str, c[0]))}-M{c[1]}-P{'x'.join(map(str, c[2]))}-s{c[3]}" for c in LINEAR]


def _linear_case(idx):
    shape, M, P, s, masked = LINEAR[idx]
    gen = torch.Generator().manual_seed(100 + idx)
    x = torch.randn(shape, generator=gen)
    w = 0.1 * torch.randn((M, shape[1]) + P, generator=gen)
    code = (shape[0], M) + tuple(d // s for d in shape[2:])
    z = torch.randn(code, generator=gen) * (torch.rand(code, generator=gen) > 0.5)
    return shape, code, P, s, masked, gen, x, w, z


@pytest.mark.parametrize("tier", ["default", "fp32"])
@pytest.mark.parametrize("idx", range(len(LINEAR)), ids=LINEAR_IDS)
def test_analysis_and_its_gradients(idx, tier):
    import cdlnet_video_amd as cva
    shape, code, P, s, _, gen, x, w, _ = _linear_case(idx)
    with_add = idx % 2 == 1
    alpha = -1.0 if with_add else 1.0
    add = torch.randn(code, generator=gen) if with_add else None
    G = torch.randn(code, generator=gen)

    lx, lw = _leaf(x), _leaf(w)
    ladd = _leaf(add) if with_add else None
    ref = alpha * O.analysis(lx, lw, s, _pad(P))
    if with_add:
        ref = ladd + ref
    (ref * G).sum().backward()

    dx, dw = _dev_leaf(x), _dev_leaf(w)
    dadd = _dev_leaf(add) if with_add else None
    with _tier(tier):
        out = cva.functional.analysis(dx, dw, s, alpha, dadd)
    (out * G.cuda()).sum().backward()                     # outside the scope: the node remembers its tier
    tag, tol = f"functional.analysis[{LINEAR_IDS[idx]} {tier}]", TIER_TOL[tier]
    check(f"{tag} out", out, ref, XTOL)
    check(f"{tag} dx", dx.grad, lx.grad, tol)
    check(f"{tag} dw", dw.grad, lw.grad, tol)
    if with_add:
        check(f"{tag} dadd", dadd.grad, ladd.grad, GU_TOL)


@pytest.mark.parametrize("tier", ["default", "fp32"])
@pytest.mark.parametrize("idx", range(len(LINEAR)), ids=LINEAR_IDS)
def test_synthesis_and_its_gradients(idx, tier):
    import cdlnet_video_amd as cva
    shape, code, P, s, masked, gen, x, w, z = _linear_case(idx)
    with_sub = idx % 2 == 0
    alpha = -1.0 if with_sub else 1.0
    sub = torch.randn(shape, generator=gen) if with_sub else None
    mask = O.bayer_mask(x) if masked else None
    G = torch.randn(shape, generator=gen)

    lz, lw = _leaf(z), _leaf(w)
    lsub = _leaf(sub) if with_sub else None
    ref = alpha * O.synthesis(lz, lw, s, _pad(P))
    if mask is not None:
        ref = mask * ref
    if with_sub:
        ref = ref - lsub
    (ref * G).sum().backward()

    dz, dw = _dev_leaf(z), _dev_leaf(w)
    dsub = _dev_leaf(sub) if with_sub else None
    with _tier(tier):
        out = cva.functional.synthesis(dz, dw, s, alpha, mask.cuda() if mask is not None else None, dsub)
    (out * G.cuda()).sum().backward()
    tag, tol = f"functional.synthesis[{LINEAR_IDS[idx]} {tier}]", TIER_TOL[tier]
    check(f"{tag} out", out, ref, XTOL)
    check(f"{tag} dz", dz.grad, lz.grad, tol)
    check(f"{tag} dw", dw.grad, lw.grad, tol)
    if with_sub:
        check(f"{tag} dsub", dsub.grad, lsub.grad, GU_TOL)


# ------------------------------------------------------------------------------------------ 2. pointwise maps
CODES = [(2, 5, 9, 13), (1, 3, 4, 20, 24), (3, 64, 40, 40)]


def _forms(shape):
    N, M = shape[:2]
    sp = tuple(shape[2:])
    one = (1,) * len(sp)
    forms = ["number", (1, M) + one, (N, M) + one, (N, 1) + sp, (1, 1) + sp, (N, M) + sp]
    if len(sp) == 3:
        forms.append((N, 1, sp[0], 1, 1))
    return forms


def _threshold(form, scale, gen):
    """A threshold of the given form in [0, scale), a sixth of its values negated (the maps are discontinuous there)."""
    if form == "number":
        return 0.37 * scale
    t = scale * torch.rand(form, generator=gen)
    return torch.where(torch.rand(form, generator=gen) < 1 / 6, -t, t)


def _codes(shape, gen):
    """As test_prox_forward_and_reverse_vs_oracle: sparse neighbours; and exact zeros in u."""
    u = 0.05 * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) > 0.1)
    zp = 0.05 * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) > 0.4)
    za = 0.05 * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) > 0.4)
    return u, zp, za, torch.randn(shape, generator=gen)


def _run_map(fn, codes, thr, gz, device):
    """fn(*codes, *thr) with every tensor a leaf on `device`; returns (out, code grads, threshold grads or None)."""
    mk = _dev_leaf if device == "cuda" else _leaf
    lc = [mk(c) for c in codes]
    lt = [mk(t) if torch.is_tensor(t) else t for t in thr]
    out = fn(*lc, *lt)
    (out * gz.to(out.device)).sum().backward()
    return out.detach(), [c.grad for c in lc], [t.grad if torch.is_tensor(t) else None for t in lt]


def _dense(t, shape):
    return t.expand(shape).contiguous() if torch.is_tensor(t) else t


@pytest.mark.parametrize("which", ["shrink", "prox_csr", "prox_csr_f2"])
@pytest.mark.parametrize("shape", CODES, ids=lambda s: "x".join(map(str, s)))
def test_pointwise_maps_with_thresholds_of_every_broadcast_form(shape, which):
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import ops
    F = cva.functional
    gen = torch.Generator().manual_seed(sum(shape) + len(which))
    u, zp, za, gz = _codes(shape, gen)
    N, M = shape[:2]
    sp = tuple(shape[2:])
    forms = _forms(shape)
    if which == "shrink":
        codes, ours, ref_fn, scales = [u], F.shrink, O.soft_threshold, (0.02,)
    elif which == "prox_csr":
        codes, ours, ref_fn, scales = [u, zp], F.prox_csr, O.prox_csr, (0.02, 1.2)
    else:
        codes, ours, ref_fn, scales = [u, zp, za], F.prox_csr_f2, O.prox_csr_f2, (0.02, 1.2, 1.2)
    code_tols = (GU_TOL, NB_TOL, NB_TOL)
    for i, form in enumerate(forms):
        # the j-th threshold takes the (i + j)-th form: every form in every slot, and mixed forms in one call
        mine = [forms[(i + j) % len(forms)] for j in range(len(scales))]
        thr = [_threshold(f, sc, gen) for f, sc in zip(mine, scales)]
        tag = f"functional.{which}[{'x'.join(map(str, shape))} {mine}]"
        ref, ref_gc, ref_gt = _run_map(ref_fn, codes, thr, gz, "cpu")
        out, gc, gt = _run_map(ours, codes, thr, gz, "cuda")
        assert torch.equal(out.cpu(), ref), f"{tag}: the forward map differs from the oracle"
        for name, a, b, tol in zip(("gu", "gz_prev", "gz_after"), gc, ref_gc, code_tols):
            check(f"{tag} {name}", a, b, tol)
        _, _, gt_dense = _run_map(ours, codes, [_dense(t, shape) for t in thr], gz, "cuda")
        for j, (t, a, b, d) in enumerate(zip(thr, gt, ref_gt, gt_dense)):
            if not torch.is_tensor(t):
                assert a is None
                continue
            assert a.shape == t.shape, f"{tag}: threshold {j} gradient of shape {tuple(a.shape)}"
            check(f"{tag} dthreshold{j}", a, b, EL_TOL if tuple(t.shape) == tuple(shape) else RED_TOL)
            check(f"{tag} dthreshold{j} against the dense expansion's", a, d.sum_to_size(t.shape), 1e-6)

    # the row form is the nets' own path, bit for bit
    rows = [_threshold((N, M) + (1,) * len(sp), sc, gen).cuda() for sc in scales]
    flat = [r.reshape(N, M).contiguous() for r in rows]
    dev = [c.cuda() for c in codes]
    with torch.no_grad():
        got = ours(*dev, *rows)
    if which == "shrink":
        want = ops.shrink(dev[0], flat[0])
    else:
        geom = ops.Geometry.make(N, 1, M, sp, (1,) * len(sp), (0,) * len(sp), 1)
        want = ops.prox_csr(geom, dev[0], dev[1], flat[0], flat[1], *((dev[2], flat[2]) if which == "prox_csr_f2" else ()))
    assert torch.equal(got, want)
    assert got.grad_fn is None and not got.requires_grad


def test_thresholds_given_as_a_list_or_on_the_cpu():
    """cva.ST / cva.prox_CSR convert a threshold as torch.as_tensor(t, device=x.device) always did."""
    import cdlnet_video_amd as cva
    gen = torch.Generator().manual_seed(9)
    u, zp, _, _ = _codes((2, 3, 5, 7), gen)
    t = torch.tensor([0.01, 0.02, -0.005]).reshape(3, 1, 1)
    want = O.soft_threshold(u, t)
    assert torch.equal(cva.ST(u.cuda(), t).cpu(), want)
    assert torch.equal(cva.ST(u.cuda(), t.tolist()).cpu(), want)
    assert torch.equal(cva.prox_CSR(u.cuda(), zp.cuda(), t, [[[0.5]], [[0.7]], [[1.1]]]).cpu(),
                       O.prox_csr(u, zp, t, torch.tensor([0.5, 0.7, 1.1]).reshape(3, 1, 1)))


# ------------------------------------------------------------------------------------------ 3. analysis_shrink
@pytest.mark.parametrize("tier", ["default", "fp32"])
@pytest.mark.parametrize("idx", [0, 3, 5], ids=[LINEAR_IDS[i] for i in (0, 3, 5)])
def test_analysis_shrink_on_the_support_of_its_output(idx, tier):
    import cdlnet_video_amd as cva
    F = cva.functional
    shape, code, P, s, _, gen, x, w, zin = _linear_case(idx)
    N, M = code[:2]
    one = (1,) * (len(code) - 2)
    with_add = idx != 0
    alpha = -1.0 if with_add else 1.0
    add = 0.5 * zin if with_add else None
    t = 0.3 + 0.6 * torch.rand((N, M) + one, generator=gen)
    G = torch.randn(code, generator=gen)

    dx, dw, dt = _dev_leaf(x), _dev_leaf(w), _dev_leaf(t)
    dadd = _dev_leaf(add) if with_add else None
    with _tier(tier):
        z = F.analysis_shrink(dx, dw, dt, s, alpha, dadd)
        if tier == "fp32":
            with torch.no_grad():
                assert torch.equal(z, F.shrink(F.analysis(dx, dw, s, alpha, dadd), dt))
    (z * G.cuda()).sum().backward()

    lx, lw, lt = _leaf(x), _leaf(w), _leaf(t)
    ladd = _leaf(add) if with_add else None
    u = alpha * O.analysis(lx, lw, s, _pad(P))
    if with_add:
        u = ladd + u
    ref = O.shrink_on_support(u, lt, z.detach().cpu())
    (ref * G).sum().backward()
    tag, tol = f"functional.analysis_shrink[{LINEAR_IDS[idx]} {tier}]", TIER_TOL[tier]
    nnz = float((z != 0).float().mean())
    log(f"{tag} nonzeros {nnz:.3f}")
    assert 0.02 < nnz < 0.98
    check(f"{tag} z", z, ref, XTOL)
    check(f"{tag} dx", dx.grad, lx.grad, tol)
    check(f"{tag} dw", dw.grad, lw.grad, tol)
    assert dt.grad.shape == t.shape
    check(f"{tag} dt", dt.grad, lt.grad, RED_TOL)
    if with_add:
        check(f"{tag} dadd", dadd.grad, ladd.grad, GU_TOL)


# ------------------------------------------------------------------------------------------ 4. modules
def _small(net, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
            elif name.endswith(".a"):
                p.copy_(0.3 + 0.3 * torch.rand(p.shape, generator=gen))
            elif name.endswith("alpha"):
                p.copy_(0.2 * torch.randn(p.shape, generator=gen))
    return net


@pytest.mark.parametrize("kind", ["CDLNet", "CDLNetVideo", "GDLNet"])
def test_module_operators_are_differentiable(kind):
    """net.A[k](x), net.B[k](z), net.D(z): the gradient reaches the filters (the four Gabor parameters) and the input, and
    D and B[0] accumulate on one Parameter.  (Before functional, `out.grad_fn` was None.)"""
    import cdlnet_video_amd as cva
    torch.manual_seed(7)
    if kind == "CDLNet":
        net, s, P, xs = cva.CDLNet(K=2, M=8, P=5, s=2, C=1, init=False), 2, (5, 5), (2, 1, 18, 22)
    elif kind == "CDLNetVideo":
        net, s, P, xs = cva.CDLNetVideo(K=2, M=6, P=(3, 5, 5), s=1, C=1, init=False), 1, (3, 5, 5), (1, 1, 4, 14, 18)
    else:
        net, s, P, xs = (cva.GDLNet(K=3, M=8, P=7, s=1, C=1, order=2, shared="a_psi_w0_alpha", init=False), 1, (7, 7),
                         (2, 1, 17, 19))
    net = _small(net, 11)
    M = net.M
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(xs, generator=gen)
    code = (xs[0], M) + tuple(d // s for d in xs[2:])
    z = torch.randn(code, generator=gen) * (torch.rand(code, generator=gen) > 0.5)
    Gz, Gx1, Gx2 = torch.randn(code, generator=gen), torch.randn(xs, generator=gen), torch.randn(xs, generator=gen)

    # the oracle on leaves, one per distinct Parameter (aliased Gabor parameters share theirs)
    leaves = {id(p): _leaf(p) for p in net.parameters()}

    def filt(mod, transpose):
        if kind == "GDLNet":
            return O.gabor_bank(*(leaves[id(p)] for p in (mod.alpha, mod.a, mod.w0, mod.psi)), P[0], transpose)
        return leaves[id(mod.weight)]

    lx, lz = _leaf(x), _leaf(z)
    ra = O.analysis(lx, filt(net.A[1], True), s, _pad(P))
    rb = O.synthesis(lz, filt(net.B[0], False), s, _pad(P))
    rd = O.synthesis(lz * 0.5, filt(net.D, False), s, _pad(P))
    ((ra * Gz).sum() + (rb * Gx1).sum() + (rd * Gx2).sum()).backward()

    net = net.cuda()
    dx, dz = _dev_leaf(x), _dev_leaf(z)
    analyse = net.A[1].T if kind == "GDLNet" else net.A[1]
    a, b, d = analyse(dx), net.B[0](dz), net.D(dz * 0.5)
    for out in (a, b, d):
        assert out.grad_fn is not None and out.requires_grad
    ((a * Gz.cuda()).sum() + (b * Gx1.cuda()).sum() + (d * Gx2.cuda()).sum()).backward()
    tag, tol = f"modules[{kind}]", TIER_TOL["default"]
    check(f"{tag} A[1](x)", a, ra, XTOL)
    check(f"{tag} B[0](z)", b, rb, XTOL)
    check(f"{tag} D(z)", d, rd, XTOL)
    check(f"{tag} dx", dx.grad, lx.grad, tol)
    check(f"{tag} dz", dz.grad, lz.grad, tol)
    seen = 0
    for name, p in net.named_parameters():
        ref = leaves_by_name(net, leaves, name)
        if ref.grad is None:
            assert p.grad is None, name
            continue
        check(f"{tag} grad {name}", p.grad, ref.grad, tol)
        seen += 1
    assert seen >= (8 if kind == "GDLNet" else 2)
    assert net.D is net.B[0]


def leaves_by_name(net, leaves, name):
    """The oracle leaf of the Parameter `name`: `leaves` was keyed by id() before net.cuda(), which keeps the Parameter
    objects (nn.Module.to swaps their .data)."""
    return leaves[id(dict(net.named_parameters())[name])]


# ------------------------------------------------------------------------------------------ 5. composition
def _plain_loop(F, y, mask, t, A, B, s):
    """CDLNet.forward (sigma None) from the blocks."""
    yp, params, mask_p = F.pre_process(y, s, mask if mask is not None else 1)
    mp = mask_p if torch.is_tensor(mask_p) else None
    z = F.analysis_shrink(yp, A[0], t[0, :1], s)
    for k in range(1, len(A)):
        r = F.synthesis(z, B[k], s, mask=mp, sub=yp)
        z = F.analysis_shrink(r, A[k], t[k, :1], s, alpha=-1.0, add=z)
    return F.post_process(F.synthesis(z, B[0], s), params), z


@pytest.mark.parametrize("shape,s,masked", [((2, 1, 33, 31), 2, False), ((2, 3, 24, 28), 1, True)])
def test_plain_loop_from_blocks_equals_the_net(shape, s, masked):
    import cdlnet_video_amd as cva
    from cdlnet_video_amd import loop
    torch.manual_seed(21)
    net = cva.CDLNet(K=3, M=16, P=7, s=s, C=shape[1], t0=5e-3, adaptive=False, init=True)
    with torch.no_grad():
        net.t.uniform_(2e-3, 2e-2)
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    net = net.cuda()
    gen = torch.Generator().manual_seed(22)
    x = cva.utils.synthetic_clip(shape, seed=23)
    mask = O.bayer_mask(x) if masked else None
    y = x + torch.randn(shape, generator=gen) * 25 / 255
    if masked:
        y = mask * y
    Gx = torch.randn(shape, generator=gen).cuda()
    dmask = mask.cuda() if masked else None
    names = [n for n, _ in net.named_parameters() if n != "g"]

    def grads(run):
        for p in net.parameters():
            p.grad = None
        yl = _dev_leaf(y)
        xhat, z = run(yl)
        ((xhat * Gx).sum() + 0.05 * z.abs().sum()).backward()
        return xhat.detach(), z.detach(), {n: dict(net.named_parameters())[n].grad.clone() for n in names}, yl.grad

    loop.set_backend("generic")
    try:
        ref = grads(lambda yl: net(yl, mask=dmask if masked else 1))
        A, B = [m.weight for m in net.A], [m.weight for m in net.B]
        got = grads(lambda yl: _plain_loop(cva.functional, yl, dmask, net.t, A, B, s))
    finally:
        loop.set_backend("auto")
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    tag = f"blocks == CDLNet[{'x'.join(map(str, shape))} s{s}]"
    for n in names:
        check(f"{tag} grad {n}", got[2][n], ref[2][n], 1e-6)
    check(f"{tag} dL/dy", got[3], ref[3], 1e-6)


def _csr_loop(F, variant, y, zp, za, c, sd, K, s):
    """CDLNet_CSR (variant "csr", neighbour branch) / CDLNet_CSRf2 (both neighbours) from the blocks; c = sigma / 255 of any
    shape that broadcasts against (N, M, *code grid) -- the thresholds are formed by torch, as the reference forms them."""
    thr = lambda p, k: p[k, :1] + c * p[k, 1:2]
    yp, params, _ = F.pre_process(y, s)
    z = None
    for k in range(K):
        if k == 0:
            u = F.analysis(yp, sd["A.0.weight"], s)
        else:
            r = F.synthesis(z, sd[f"B.{k}.weight"], s, sub=yp)
            u = F.analysis(r, sd[f"A.{k}.weight"], s, alpha=-1.0, add=z)
        if variant == "csr":
            z = F.prox_csr(u, zp, thr(sd["t"], k), thr(sd["g"], k))
        else:
            z = F.prox_csr_f2(u, zp, za, thr(sd["t"], k), thr(sd["g1"], k), thr(sd["g2"], k))
    return F.post_process(F.synthesis(z, sd["B.0.weight"], s), params), z


def _csr_case(seed, N=2, M=8, K=3, P=5, s=1, H=26, W=22):
    """The construction whose float32 oracle has no support difference against float64 in any of the six cases."""
    g = torch.Generator().manual_seed(seed)
    W0 = torch.randn(M, 1, P, P, generator=g)
    W0 = W0 / W0.flatten(1).norm(dim=1).reshape(M, 1, 1, 1) / 3.0
    sd = {}
    for k in range(K):
        sd[f"A.{k}.weight"] = W0 + 0.05 * W0.abs().mean() * torch.randn(W0.shape, generator=g)
        sd[f"B.{k}.weight"] = W0 + 0.05 * W0.abs().mean() * torch.randn(W0.shape, generator=g)
    sd["t"] = 2e-3 + 1.8e-2 * torch.rand(K, 2, M, 1, 1, generator=g)
    sd["g1"] = 0.2 + torch.rand(K, 2, M, 1, 1, generator=g)
    sd["g2"] = 0.2 + torch.rand(K, 2, M, 1, 1, generator=g)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    x = (0.5 + 0.25 * torch.sin(7 * xx + 3 * yy) + 0.2 * torch.cos(11 * yy * xx)).expand(N, 1, H, W).clone()
    Hc, Wc = -(-H // s), -(-W // s)
    cy, cx = torch.meshgrid(torch.linspace(0, 1, Hc), torch.linspace(0, 1, Wc), indexing="ij")
    sigma = (15 + 20 * cy * cx).expand(N, 1, Hc, Wc).clone() + 5 * torch.arange(N).reshape(N, 1, 1, 1)
    lvl = sigma.repeat_interleave(s, -1).repeat_interleave(s, -2)[..., :H, :W]
    ys = [x + torch.randn(x.shape, generator=g) * lvl / 255 for _ in range(3)]
    return sd, x, ys, sigma, dict(K=K, P=P, s=s)


def test_csrf2_loop_from_blocks_with_per_sample_sigma_equals_the_net():
    import cdlnet_video_amd as cva
    sd, x, ys, _, kw = _csr_case(41)
    K, P, s = kw["K"], kw["P"], kw["s"]
    sigma = torch.tensor([15.0, 30.0]).reshape(2, 1, 1, 1)
    with torch.no_grad():
        _, zp = O.ista_csr(sd, ys[0], None, None, sigma=sigma, adaptive=True, variant="f2", **kw)
        _, za = O.ista_csr(sd, ys[2], None, None, sigma=sigma, adaptive=True, variant="f2", **kw)
    net = cva.CDLNet_CSRf2(K=K, M=8, P=P, s=s, C=1, t0=0.0, adaptive=True, init=False)
    net.load_state_dict({**sd, "D.weight": sd["B.0.weight"]})
    net = net.cuda()
    xd = x.cuda()
    loss_of = lambda xhat, z: torch.mean((xd - xhat) ** 2) + 0.05 * z.abs().mean()

    lzp, lza = _dev_leaf(zp), _dev_leaf(za)
    xr, zr = net(ys[1].cuda(), lzp, lza, sigma.cuda())
    loss_of(xr, zr).backward()
    ref = {n: p.grad.clone() for n, p in net.named_parameters()}
    ref.update(z_prev=lzp.grad, z_after=lza.grad)

    for p in net.parameters():
        p.grad = None
    params = dict(net.named_parameters())
    mzp, mza = _dev_leaf(zp), _dev_leaf(za)
    xh, z = _csr_loop(cva.functional, "f2", ys[1].cuda(), mzp, mza, sigma.cuda() / 255.0, params, K, s)
    loss_of(xh, z).backward()
    got = {n: p.grad for n, p in net.named_parameters()}
    got.update(z_prev=mzp.grad, z_after=mza.grad)
    check("blocks == CDLNet_CSRf2 xhat", xh, xr, XTOL)
    check("blocks == CDLNet_CSRf2 z", z, zr, XTOL)
    assert sorted(got) == sorted(ref)
    for n in ref:
        check(f"blocks == CDLNet_CSRf2 grad {n}", got[n], ref[n], CSR_GTOL)


def _map_run(F, variant, sd, y, zp, za, sigma, x, K, s):
    leaves = {k: _dev_leaf(v) for k, v in sd.items()}
    ly, lzp, ls = _dev_leaf(y), _dev_leaf(zp), _dev_leaf(sigma)
    lza = _dev_leaf(za) if variant == "f2" else None
    xh, z = _csr_loop(F, variant, ly, lzp, lza, ls / 255.0, leaves, K, s)
    (torch.mean((x.cuda() - xh) ** 2) + 0.05 * z.abs().mean()).backward()
    grads = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    grads.update({"y": ly.grad, "sigma": ls.grad, "z_prev": lzp.grad})
    if lza is not None:
        grads["z_after"] = lza.grad
    return xh.detach(), z.detach(), grads


@pytest.mark.parametrize("seed", [41, 42, 43])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("variant", ["f2", "csr"])
def test_csr_loops_with_a_sigma_map_vs_oracle(variant, s, seed):
    """What the CSR nets refuse and the blocks make possible: a noise-level map in all three threshold families.  Near-ties
    as in test_fixture_matches_reference: at most 4 support differences against the oracle's code on the default tier, and
    then the comparison is made under precision_scope("fp32"), where there must be none."""
    import cdlnet_video_amd as cva
    sd, x, ys, sigma, kw = _csr_case(seed, s=s)
    K = kw["K"]
    with torch.no_grad():
        _, zp = O.ista_csr(sd, ys[0], None, None, sigma=sigma, adaptive=True, variant="f2", **kw)
        _, za = O.ista_csr(sd, ys[2], None, None, sigma=sigma, adaptive=True, variant="f2", **kw)
    if variant == "csr":
        sd = {k: v for k, v in sd.items() if k not in ("g1", "g2")}
        sd["g"] = _csr_case(seed, s=s)[0]["g1"]
        za = None
    leaves = {k: _leaf(v) for k, v in sd.items()}
    ly, lzp, ls = _leaf(ys[1]), _leaf(zp), _leaf(sigma)
    lza = _leaf(za) if za is not None else None
    xr, zr = O.ista_csr(leaves, ly, lzp, lza, sigma=ls, adaptive=True, variant=variant, **kw)
    (torch.mean((x - xr) ** 2) + 0.05 * zr.abs().mean()).backward()
    ref = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    ref.update({"y": ly.grad, "sigma": ls.grad, "z_prev": lzp.grad})
    if lza is not None:
        ref["z_after"] = lza.grad

    tag = f"blocks, sigma map[{variant} s{s} seed{seed}]"
    tier = "default"
    xh, z, got = _map_run(cva.functional, variant, sd, ys[1], zp, za, sigma, x, K, s)
    flips = int(((z.cpu() != 0) != (zr != 0)).sum())
    log(f"{tag} support differences against the oracle: {flips}")
    if flips:
        assert flips <= 4, f"{tag}: {flips} support differences is more than near-ties"
        tier = "fp32"
        with _tier("fp32"):
            xh, z, got = _map_run(cva.functional, variant, sd, ys[1], zp, za, sigma, x, K, s)
        assert int(((z.cpu() != 0) != (zr != 0)).sum()) == 0
    # every gradient of this test, the neighbour codes' included, has passed through the K operator iterations of the sweep:
    # the tolerance of the matrix-core kernels on the tier in use (the 1e-5 of the pointwise maps' neighbour-code gradients
    # is the stand-alone pass's, checked in test_pointwise_maps_with_thresholds_of_every_broadcast_form)
    tol = TIER_TOL[tier]
    check(f"{tag} xhat", xh, xr, XTOL)
    check(f"{tag} z", z, zr, XTOL)
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    assert got["sigma"].shape == sigma.shape
    for n in sorted(ref):
        assert got[n].shape == ref[n].shape, n
        check(f"{tag} grad {n}", got[n], ref[n], tol)


# ------------------------------------------------------------------------------------------ the reference's record
FIX_TOL = 2e-4           # tests/test_gpu_sigmamap.py FIX_TOL / FIX_GTOL: gradients against the reference's recorded ones


@pytest.mark.parametrize("name", ["csr", "f2"])
def test_prox_fixture_with_map_shaped_thresholds(name):
    """tests/golden/p0 (tools/make_golden_functional.py): the unmodified reference's prox_CSR / prox_CSR_f2 with thresholds
    t0[m] + c[n,pix] * t1[m]; the gradient reaches c and the (2,1,M,1,1) families through torch's broadcast."""
    import cdlnet_video_amd as cva
    g = load_golden("p0_prox_map_thresholds")
    v = {k: _dev_leaf(g[k]) for k in ("u", "zp", "za", "c", "t", "g1", "g2")}
    thr = lambda p: p[0] + v["c"] * p[1]
    if name == "csr":
        out = cva.prox_CSR(v["u"], v["zp"], thr(v["t"]), thr(v["g1"]))
    else:
        out = cva.prox_CSR_f2(v["u"], v["zp"], v["za"], thr(v["t"]), thr(v["g1"]), thr(v["g2"]))
    assert torch.equal(out.detach().cpu(), g[f"{name}_out"])
    (out * g["G"].cuda()).sum().backward()
    tols = {"u": GU_TOL, "zp": NB_TOL, "za": NB_TOL}
    seen = 0
    for key, leaf in v.items():
        ref = g.get(f"{name}_d{key}")
        if ref is None:
            assert leaf.grad is None, key
            continue
        assert leaf.grad.shape == ref.shape
        check(f"p0 {name} d{key}", leaf.grad, ref, tols.get(key, RED_TOL))
        seen += 1
    assert seen == (5 if name == "csr" else 7)


def test_csrf2_fixture_with_a_sigma_map():
    """tests/golden/p1: one CDLNet_CSRf2 call of the unmodified reference with both neighbours and `sigma` a map, replayed
    from the blocks.  Near-ties as in test_fixture_matches_reference."""
    import cdlnet_video_amd as cva
    g = load_golden("p1_csrf2_sigma_map")
    K, M, P, s, C = g["hyper"]
    sd = {k: v for k, v in g["sd"].items() if k != "D.weight"}
    flips = lambda z: int(((z.cpu() != 0) != (g["z"] != 0)).sum())
    xh, z, got = _map_run(cva.functional, "f2", sd, g["y"], g["zp"], g["za"], g["sigma"], g["x"], K, s)
    n = flips(z)
    log(f"p1 support differences against the reference: {n}")
    if n:
        assert n <= 4
        with _tier("fp32"):
            xh, z, got = _map_run(cva.functional, "f2", sd, g["y"], g["zp"], g["za"], g["sigma"], g["x"], K, s)
        assert flips(z) == 0
    check("p1 xhat", xh, g["xhat"], XTOL)
    check("p1 z", z, g["z"], XTOL)
    for key, name in (("dy", "y"), ("dsigma", "sigma"), ("dzp", "z_prev"), ("dza", "z_after")):
        assert got[name].shape == g[key].shape
        check(f"p1 {key}", got[name], g[key], FIX_TOL)
    seen = 0
    for key, ref in g["grad"].items():
        check(f"p1 grad {key}", got[key], ref, FIX_TOL)
        seen += 1
    assert seen == 2 * K + 3


# ------------------------------------------------------------------------------------------ 6. loud failures
def test_what_is_not_produced_raises():
    import cdlnet_video_amd as cva
    F = cva.functional
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(2, 4, 8, 8, generator=gen).cuda()
    w = (0.1 * torch.randn(4, 1, 3, 3, generator=gen)).cuda()
    with pytest.raises(NotImplementedError, match="mask"):
        F.synthesis(z, w, mask=torch.ones(2, 1, 8, 8, device="cuda", requires_grad=True))

    # a double backward (the upstream gradient must itself depend on the input for a second derivative to exist)
    zl = z.clone().requires_grad_(True)
    t = torch.full((1, 4, 1, 1), 0.3, device="cuda", requires_grad=True)
    (gz,) = torch.autograd.grad(F.shrink(zl, t).square().sum(), zl, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        gz.sum().backward()
    wl = w.clone().requires_grad_(True)
    (gw,) = torch.autograd.grad(F.synthesis(z, wl).square().sum(), wl, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice|once_differentiable"):
        gw.sum().backward()

    # the nets' own refusals stay
    net = cva.CDLNet_CSR(K=2, M=4, P=3, s=1, C=1, t0=1e-2, adaptive=True, init=False).cuda()
    y = torch.rand(2, 1, 8, 8, device="cuda")
    with pytest.raises(NotImplementedError, match="map"):
        net(y, z, sigma=torch.full((2, 1, 8, 8), 25.0, device="cuda"))
