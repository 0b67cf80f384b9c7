"""Every HIP operator on guard-banded, misaligned buffers (tests/arena_util.py; DESIGN.md "Alignment contract").

Each case carves EVERY tensor argument of an operator out of a poisoned arena at an element offset: all arguments at
offset 0, 1, 2 (a 16-, 4- and 8-byte aligned base) and, in the `out1` mode, the outputs at offset 1 with aligned inputs
(a launcher that tests one pointer and vector-accesses another).  Library-sized workspaces (analysis / filter-gradient
scratch, patch buffers, fragment buffers) are guard-banded too but stay at offset 0: the contract asks 16 bytes of them.

Every case asserts
  1. no guard or pad word changed, and every output element was written;
  2. parity with the float64 (for the discontinuous pointwise maps: the bit-exact fp32) reference of the operator, at
     the tolerance its existing test uses (named next to each case);
  3. the launch trace shows the kernel the case is about, in its 16-byte form when every pointer is aligned and in
     its scalar form otherwise, where the launcher selects on alignment;
  4. where the trace equals the offset-0 run's, the result equals it bit for bit.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import csr_tangent_restate as R
import nle_pca_cells_restate as NC
import nle_pca_restate as NR
import perceptual_restate as PR
import ssim_restate as SR
from arena_util import Arena
from gpu_util import check, launch_sites
from oracle import cdl_oracle as O

pytestmark = pytest.mark.gpu

MODES = {"off0": (0, 0), "off1": (1, 1), "off2": (2, 2), "off3": (3, 3), "out1": (0, 1)}
DEFAULT_MODES = ("off0", "off1", "off2", "out1")
MFMA_TOL, FP32_TOL, FP32_WTOL = 2e-5, 2e-6, 1e-5            # test_gpu_dispatch.py / test_gpu_ops.py
ENV_VALU = {"CDL_MFMA_ANALYSIS": "0", "CDL_MFMA_SYNTHESIS": "0", "CDL_MFMA_WGRAD": "0", "CDL_MFMA_DENSE": "0"}
ENV_MFMA = {"CDL_MFMA_ANALYSIS": "1", "CDL_MFMA_SYNTHESIS": "1", "CDL_MFMA_WGRAD": "1", "CDL_MFMA_DENSE": "1"}


def ops():
    import cdlnet_video_amd as cva
    return cva.ops


class Carve:
    """The arena of one run: inputs at `ioff`, outputs at `ooff`, workspaces at 0."""

    def __init__(self, mode):
        self.arena = Arena("cuda")
        self.ioff, self.ooff = MODES[mode]
        self.outs, self.posts = {}, {}

    def i(self, t, name=None):
        return None if t is None else self.arena.put(t, self.ioff, name)

    def o(self, name, shape, dtype=torch.float32):
        self.outs[name] = self.arena.out(shape, self.ooff, dtype, name)
        return self.outs[name]

    def lay(self, name, n, post):
        """A library-sized code buffer in an internal layout (blocked / rsc: sized by the library, 16-byte accesses, so
        offset 0 by the contract; its padding pixels are never written): guard-banded, and compared as `post(buffer)`."""
        v = self.arena.out((int(n),), 0, torch.float32, name)
        self.posts[name] = (v, post)
        return v

    def io(self, name, t):
        """A buffer the kernel reads and writes (accumulated into, or updated in place): an output that starts as `t`."""
        v = self.o(name, t.shape, t.dtype)
        v.copy_(t)
        return v

    def ws(self, name, n, dtype=torch.float32):
        return self.arena.out((max(int(n), 1),), 0, dtype, name)


class Case:
    """`make()` builds the seeded inputs and returns (run(A), ref(got)): called at the first run, never at collection."""

    def __init__(self, name, make, pin=None, env=None, modes=DEFAULT_MODES):
        self.name, self.make, self.pin, self.env, self.modes = name, make, pin, env or {}, modes
        self._built = None

    def _build(self):
        if self._built is None:
            self._built = self.make()
        return self._built

    def run(self, A):
        return self._build()[0](A)

    def ref(self, got):
        return self._build()[1](got)

    def __repr__(self):
        return self.name


_BASE = {}
PIN_MODE = [None]           # the mode of the run a pin is looking at (for gates on one pointer's alignment)


def execute(case, mode):
    """({output: cpu tensor}, trace signature, launch sites) of one run; guards and definedness asserted."""
    A = Carve(mode)
    with ops().trace() as t:
        case.run(A)
        torch.cuda.synchronize()
    A.arena.check()
    for v in A.outs.values():
        A.arena.assert_defined(v)
    sig = tuple((r.file, r.line, r.func, r.note) for r in t)
    got = {k: v.detach().cpu().clone() for k, v in A.outs.items()}
    got.update({k: post(v).detach().cpu().clone() for k, (v, post) in A.posts.items()})
    return got, sig, launch_sites(t)


def run_case(case, mode, hip_env):
    for k, v in case.env.items():
        hip_env(k, v)
    if case.name not in _BASE:
        _BASE[case.name] = execute(case, "off0")
    base, base_sig, _ = _BASE[case.name]
    got, sig, sites = _BASE[case.name] if mode == "off0" else execute(case, mode)
    for name, (ref, tol) in case.ref(got).items():
        if tol == 0:
            assert torch.equal(got[name], ref.to(got[name].dtype)), f"{case.name}[{mode}] {name}: not the reference's bits"
        elif isinstance(tol, tuple) and tol[0] == "f64":          # max|got - ref| / max|ref| without a pass through float32
            err = float((got[name].double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))
            assert err < tol[1], f"{case.name}[{mode}] {name}: rel_err {err:.3e} >= {tol[1]:.1e}"
        elif isinstance(tol, tuple):                             # ("l2", bound): relative l2 error
            l2 = float((got[name].double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))
            assert tol[0] == "l2" and l2 < tol[1], f"{case.name}[{mode}] {name}: l2 error {l2:.3e} >= {tol[1]:.1e}"
        else:
            check(f"arena {case.name}[{mode}] {name}", got[name], ref, tol)
    assert case.pin is not None, f"{case.name}: no kernel pinned"
    PIN_MODE[0] = mode
    case.pin(sites, mode == "off0", MODES[mode][0] == 0)
    if sig == base_sig:
        for name in got:
            assert torch.equal(got[name], base[name]), f"{case.name}[{mode}] {name}: same launches, other bits than at offset 0"
    return sites


def need(sites, *ids):
    for s in ids:
        assert s in sites, f"{s} did not run: {sorted(sites)}"


def forbid(sites, *ids):
    for s in ids:
        assert s not in sites, f"{s} ran: {sorted(sites)}"


def vec_or_scalar(vec, scalar, always=()):
    """pin(sites, aligned, aligned_in): `vec` when every pointer is aligned, `scalar` otherwise (never both), `always`
    in every mode.  aligned_in: the inputs are aligned (the outputs may not be)."""
    def pin(sites, aligned, aligned_in):
        need(sites, *always)
        need(sites, vec if aligned else scalar)
        forbid(sites, scalar if aligned else vec)
    return pin


def exactly(want, also=()):
    """pin(): launch site -> number of records, exactly; `also` sites at least once."""
    def pin(sites, aligned, aligned_in):
        need(sites, *also)
        for site, n in want.items():
            assert len(sites.get(site, [])) == n, f"{site}: {len(sites.get(site, []))} launches, expected {n}: {sorted(sites)}"
    return pin


def only(*ids):
    def pin(sites, aligned, aligned_in):
        need(sites, *ids)
    return pin


CASES = []


def case(name, **kw):
    def deco(make):
        CASES.append(Case(name, make, **kw))
        return make
    return deco


def sparse(shape, gen, keep=0.3, scale=1.0):
    return scale * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) < keep)


def support_map_ref(z, planes):
    """The support / sign bit planes of a code tensor (ops.fusedg_support_map's layout, which is the fused 2-D kernels'
    for M <= 64), on the CPU."""
    N, M = z.shape[:2]
    out = torch.zeros((N, planes) + tuple(z.shape[2:]), dtype=torch.int64)
    for ch in range(M):
        R, rem = divmod(ch, 32)
        q, rem = divmod(rem, 8)
        h, e = divmod(rem, 4)
        bit, pl = 16 * (R & 1) + 4 * q + e, 4 * (R >> 1) + 2 * h
        nz = z[:, ch] != 0
        out[:, pl] |= nz.to(torch.int64) << bit
        out[:, pl + 1] |= (torch.signbit(z[:, ch]) & nz).to(torch.int64) << bit
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


# ------------------------------------------------------------------------------------------------ pointwise
CODE_SHAPES = [(2, 5, 8, 12), (2, 5, 9, 13), (1, 3, 4, 20, 24)]


def _pointwise(shape):
    tag = "x".join(str(d) for d in shape)
    N, M = shape[:2]
    per = 1
    for d in shape[2:]:
        per *= d
    bsh = (N, M) + (1,) * (len(shape) - 2)

    @case(f"shrink thresholds {tag}", pin=only("cdl_generic.hip:k_shrink", "cdl_generic.hip:k_thresholds"))
    def _():
        gen = torch.Generator().manual_seed(4 + per)
        x = torch.randn(shape, generator=gen) * 0.1
        x.view(-1)[:3] = torch.tensor([0.0, -0.0, 1e-30])
        tau = torch.rand(N, M, generator=gen) * 0.2 - 0.05

        t = torch.rand(3, 2, M, 1, 1, generator=gen) * 0.1
        c = torch.rand(N, generator=gen)

        def run(A):
            ops()._call("cdl_shrink", A.i(x, "x"), A.i(tau, "tau"), A.o("out", shape), N * M, per)
            ops()._call("cdl_thresholds", A.i(t, "t"), A.i(c, "c"), A.o("tau_knm", (3, N, M)), 3, N, M)

        def ref(got):                                                                     # both bit-exact: test_gpu_ops.py
            return {"out": (O.soft_threshold(x, tau.reshape(bsh)), 0),
                    "tau_knm": (t[:, 0].reshape(3, 1, M) + c.reshape(1, N, 1) * t[:, 1].reshape(3, 1, M), 0)}
        return run, ref

    @case(f"shrink_b fwd+bwd {tag}", pin=exactly({"cdl_generic.hip:k_shrink": 2}))
    def _():
        o = ops()
        gen = torch.Generator().manual_seed(5 + per)
        x = torch.randn(shape, generator=gen) * 0.1
        tau = torch.rand(bsh, generator=gen) * 0.2 - 0.05
        gup = torch.randn(shape, generator=gen)
        st = o.bcast_strides(bsh, shape)

        def run(A):
            xd, td = A.i(x, "x"), A.i(tau, "tau")
            o._call("cdl_shrink_b", xd, td, st, A.o("out", shape), N, M, per)
            o._call("cdl_shrink_b_bwd", A.i(gup, "gup"), xd, td, st, A.o("gx", shape), A.o("dtau_el", shape), N, M, per)

        def ref(got):
            xr = x.clone().requires_grad_(True)
            tr = tau.expand(shape).clone().requires_grad_(True)
            out = O.soft_threshold(xr, tr)
            (out * gup).sum().backward()
            # the forward is the reference's expression bit for bit; the reverse is a select of gup / -sign * gup
            return {"out": (out.detach(), 0), "gx": (xr.grad, 0), "dtau_el": (tr.grad, 0)}
        return run, ref

    for both in (False, True):
        @case(f"prox_csr{'_f2' if both else ''} fwd+bwd+tangent {tag}",
              pin=only("cdl_prox.hip:k_prox_fwd", "cdl_prox.hip:k_prox_bwd"))
        def _(both=both):
            o = ops()
            gen = torch.Generator().manual_seed(sum(shape) + both)
            u = 0.05 * torch.randn(shape, generator=gen)
            zp = 0.05 * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) > 0.4)
            za = 0.05 * torch.randn(shape, generator=gen) * (torch.rand(shape, generator=gen) > 0.4)
            gz = torch.randn(shape, generator=gen)
            c = torch.rand(N, generator=gen)
            t, g1, g2 = (torch.rand(1, 2, M, generator=gen) * s for s in (0.02, 1.2, 1.2))
            seed = torch.randn(shape, generator=gen)
            ud, zpd, zad = (torch.randn(shape, generator=gen) for _ in range(3))
            sp = shape[2:]
            geom = o.Geometry.make(N, 1, M, sp, (1,) * len(sp), (0,) * len(sp), 1)
            cb = c.reshape((N,) + (1,) * (len(sp) + 1))
            th = lambda p: (p[0, 0].reshape((1, M) + (1,) * len(sp)) + cb * p[0, 1].reshape((1, M) + (1,) * len(sp)))
            rows = lambda p: th(p).reshape(N, M).contiguous()                  # what cdl_thresholds computes, same expression

            def run(A):
                ud_, zpd_ = A.i(u, "u"), A.i(zp, "z_prev")
                zad_ = A.i(za, "z_after") if both else None
                lam, gam1 = A.i(rows(t), "lam"), A.i(rows(g1), "gam1")
                gam2 = A.i(rows(g2), "gam2") if both else None
                o.prox_csr(geom, ud_, zpd_, lam, gam1, zad_, gam2, out=A.o("z", shape))
                o.prox_csr_bwd(geom, A.i(gz, "gz"), ud_, zpd_, lam, gam1, A.i(c, "c"), A.o("dlam", (2, M)),
                               A.o("dgam1", (2, M)), zad_, gam2, A.o("dgam2", (2, M)) if both else None,
                               A.io("gz_prev", seed), A.io("gz_after", seed) if both else None, out=A.o("gu", shape))
                o.prox_csr_tangent(geom, A.i(ud, "ud"), ud_, zpd_, lam, gam1, zad_, gam2, A.i(zpd, "zd_prev"),
                                   A.i(zad, "zd_after") if both else None, out=A.o("zd", shape))

            def ref(got):
                # tests/test_gpu_csr.py::test_prox_forward_and_reverse_vs_oracle: forward bit-exact, reverse 1e-6 / 1e-5 / 2e-5
                leaves = [v.clone().requires_grad_(True) for v in (u, zp, za, t, g1, g2)]
                lu, lzp, lza, lt, lg1, lg2 = leaves
                fwd = lambda a, b, c_: (O.prox_csr_f2(a, b, c_, th(lt), th(lg1), th(lg2)) if both
                                        else O.prox_csr(a, b, th(lt), th(lg1)))
                z = fwd(lu, lzp, lza)
                (z * gz).sum().backward()
                out = {"z": (z.detach(), 0), "gu": (lu.grad, 1e-6), "gz_prev": (seed + lzp.grad, 1e-5),
                       "dlam": (lt.grad[0], 2e-5), "dgam1": (lg1.grad[0], 2e-5)}
                if both:
                    out.update({"gz_after": (seed + lza.grad, 1e-5), "dgam2": (lg2.grad[0], 2e-5)})
                # the tangent: a select of the tangents' bits on the piece the fp32 gates choose (tests/csr_tangent_restate.py;
                # tests/test_gpu_csr_tangent.py compares with torch.equal)
                G = R.gates(u, zp, za if both else None, th(t), th(g1), th(g2) if both else None)
                out["zd"] = (R.prox_tangent(G, ud, zpd, zad if both else None), 0)
                return out
            return run, ref

    @case(f"tau_grad sigma_grad dyp_split {tag}",
          pin=exactly({"cdl_generic.hip:k_sigma_grad<false>": 1, "cdl_generic.hip:k_sigma_grad<true>": 1,
                       "cdl_datagrad.hip:k_dyp_split": 1, "cdl_generic.hip:k_tau_partial<false,false>": 1},
                      also=("cdl_generic.hip:k_tau_final<false>",)))
    def _():
        o = ops()
        gen = torch.Generator().manual_seed(6 + per)
        sp = shape[2:]
        geom = o.Geometry.make(N, 1, M, sp, (1,) * len(sp), (0,) * len(sp), 1)
        z = sparse(shape, gen)
        gup = torch.randn(shape, generator=gen)
        c = torch.rand(N, generator=gen)
        tslope = torch.rand(M, generator=gen)
        dc0 = torch.randn((N, 1) + sp, generator=gen)
        q = torch.randn(geom.image_shape(), generator=gen)
        mask = (torch.rand(geom.image_shape(), generator=gen) < 0.5).float()
        dyp0 = torch.randn(geom.image_shape(), generator=gen)

        def run(A):
            gd, zd = A.i(gup, "gup"), A.i(z, "zout")
            o.tau_grad(geom, gd, zd, A.i(c, "c"), A.o("dt_k", (2, M)), A.o("dtau_n", (N, M)))
            o.sigma_grad(geom, gd, zd, A.i(tslope, "tslope"), A.o("dcmap", (N, 1) + sp), False)
            o.sigma_grad(geom, gd, zd, A.i(tslope, "tslope2"), A.io("dcmap_acc", dc0), True)
            o.dyp_split(geom, A.io("q", q), A.i(mask, "mask"), A.io("dyp", dyp0), True)

        def ref(got):
            red = tuple(range(2, len(shape)))
            s_nm = -(torch.sign(z).double() * gup.double()).sum(dim=red)
            dc = -(tslope.double().reshape((1, M) + (1,) * len(sp)) * torch.sign(z).double() * gup.double()).sum(1, keepdim=True)
            return {"dt_k": (torch.stack([s_nm.sum(0), (c.double()[:, None] * s_nm).sum(0)]), 1e-5),   # test_gpu_ops.py
                    "dtau_n": (s_nm, 1e-5),
                    "dcmap": (dc, 1e-5), "dcmap_acc": (dc0.double() + dc, 1e-5),                       # test_gpu_sigmamap.py
                    "q": (-mask * q, 0), "dyp": (dyp0 + q, 0)}
        return run, ref


for _shape in CODE_SHAPES:
    _pointwise(_shape)


# ------------------------------------------------------------------------------- preprocess / postprocess
def _prepost(shape, s, masked):
    per_n = 1
    for d_ in shape[1:]:
        per_n *= d_

    def pin(sites, aligned, aligned_in):
        need(sites, "cdl_generic.hip:k_pad_center", "cdl_generic.hip:k_crop_add", "cdl_generic.hip:k_embed",
             "cdl_datagrad.hip:k_preprocess_bwd")
        # from 32768 elements a sample the mean's partial sums are parked as doubles in yp: only when yp is 8-byte aligned
        split = per_n >= 32768 and MODES[PIN_MODE[0]][1] % 2 == 0
        need(sites, *(("cdl_generic.hip:k_sample_sums_split", "cdl_generic.hip:k_sample_sums_final") if split
                      else ("cdl_generic.hip:k_sample_sums",)))
        forbid(sites, "cdl_generic.hip:k_sample_sums" if split else "cdl_generic.hip:k_sample_sums_split")

    @case(f"pre/postprocess {'x'.join(map(str, shape))} s{s} mask{int(masked)}", pin=pin)
    def _():
        o = ops()
        gen = torch.Generator().manual_seed(3 + sum(shape) + s)
        y = torch.rand(shape, generator=gen)
        mask = (torch.rand(shape, generator=gen) < 0.5).float() if masked else None
        if masked:
            y = y * mask
        nd = len(shape) - 2
        N, C = shape[:2]
        sp = o._three(shape[2:], 1)
        pads = o.stride_pads(shape[2:], s)
        p6 = o._pads6(pads, nd)
        spp = [sp[i] + p6[2 * i] + p6[2 * i + 1] for i in range(3)]
        pshape = (N, C) + tuple(spp[3 - nd:])
        xp = torch.randn(pshape, generator=gen)
        gx = torch.randn(shape, generator=gen)
        dyp = torch.randn(pshape, generator=gen)

        def run(A):
            md = A.i(mask, "mask")
            mean = A.o("mean", (N,))
            o._call("cdl_preprocess", A.i(y, "y"), md, A.o("yp", pshape), A.o("mask_p", pshape) if masked else None, mean,
                    N, C, *sp, p6)
            o._call("cdl_postprocess", A.i(xp, "xp"), mean, A.o("xhat", shape), N, C, *sp, p6)
            gxd = A.i(gx, "gxhat")
            o._call("cdl_postprocess_bwd", gxd, A.o("gxp", pshape), N, C, *sp, p6)
            o._call("cdl_preprocess_bwd", A.i(dyp, "dyp"), gxd, md, A.o("dy", shape), N, C, *sp, p6)

        def ref(got):
            y64 = y.double().requires_grad_(True)
            m64 = None if mask is None else mask.double()
            yp, mean, rpads, mask_p = O.preprocess(y64, s, m64)
            assert tuple(rpads) == tuple(pads)
            xhat = O.postprocess(xp.double(), mean, pads)
            # dL/dy of <yp, dyp> + <xhat, gx> (the mean enters both): what cdl_preprocess_bwd computes
            ((yp * dyp.double()).sum() + (xhat * gx.double()).sum()).backward()
            full = torch.zeros(pshape, dtype=torch.float64)
            O.crop(full, pads).copy_(gx.double())
            out = {"yp": (yp.detach(), 2e-6), "mean": (mean.detach().reshape(-1), 2e-6), "xhat": (xhat.detach(), 2e-6),
                   "gxp": (full, 0), "dy": (y64.grad, 1e-5)}           # test_gpu_ops.py 2e-6 / exact; test_gpu_datagrad.py 1e-5
            if masked:
                out["mask_p"] = (mask_p, 0)
            return out
        return run, ref


for _shape, _s, _masked in (((2, 1, 24, 40), 1, False), ((2, 1, 24, 40), 2, True), ((2, 3, 23, 37), 2, True),
                            ((2, 3, 23, 37), 2, False), ((1, 1, 7, 13, 11), 2, False), ((1, 2, 5, 6, 8), 1, True),
                            ((2, 1, 192, 192), 1, False)):
    _prepost(_shape, _s, _masked)


# ------------------------------------------------------------------- analysis / synthesis / filter gradients
TIL, GEN = "cdl_generic_tiled.hip:", "cdl_generic.hip:"
K_ANA = "cdl_analysis_mfma.hip:k_ana_m<PH,PW,SW,MT,PROX,REV,MAP>"
K_WGM = "cdl_wgrad_mfma.hip:k_wgm<PH,PW,SW,NG,CT>"
K_ASM4, K_ASM1 = "cdl_synth_mfma.hip:k_synth_assemble4<PH,PW,SW>", "cdl_synth_mfma.hip:k_synth_assemble<PH,PW,SW>"


@functools.lru_cache(maxsize=None)
def _generic_data(N, C, M, sp, P, s):
    gen = torch.Generator().manual_seed(20)
    zsp = tuple(d // s for d in sp)
    d = {"x": torch.randn((N, C) + sp, generator=gen), "z": sparse((N, M) + zsp, gen),
         "w": torch.randn((M, C) + P, generator=gen) * 0.2, "u": torch.randn((N, M) + zsp, generator=gen),
         "tau": torch.rand(N, M, generator=gen) * 0.5 + 0.01, "c": torch.rand(N, generator=gen)}
    d["mask"] = (torch.rand(d["x"].shape, generator=gen) < 0.4).float()
    return d


def _ladder(key, tier, masked=True):
    N, C, M, sp, P, s = key
    pad = tuple(p // 2 for p in P)
    tol, wtol = (MFMA_TOL, MFMA_TOL) if tier == "mfma" else (FP32_TOL, FP32_WTOL)
    env = ENV_MFMA if tier == "mfma" else ENV_VALU
    tag = f"[{tier}] N{N}C{C}M{M}{sp}P{P}s{s}"
    bsh = (N, M) + (1,) * len(sp)

    def mfma_only(*ids):
        def pin(sites, aligned, aligned_in):
            if tier == "mfma":
                need(sites, *ids)
            else:
                assert not any(k.split(":")[0] in ("cdl_analysis_mfma.hip", "cdl_synth_mfma.hip", "cdl_wgrad_mfma.hip")
                               for k in sites), sorted(sites)
        return pin

    def pin_analysis(sites, aligned, aligned_in):
        """Five calls (iter, gated, reverse step, CSR epilogue, noise-level map): on the matrix-core tier each one a k_ana_m
        launch, one of them with REV, one with PROX, one with MAP; on the VALU tier none."""
        mfma_only(K_ANA)(sites, aligned, aligned_in)
        if tier == "mfma":
            t = [r.template() for r in sites[K_ANA]]
            assert len(t) == 5 and [sum(bool(x[k]) for x in t) for k in ("PROX", "REV", "MAP")] == [1, 1, 1], t
            forbid(sites, *[k for k in sites if k.startswith((TIL, GEN + "k_analysis"))])

    @case(f"analysis {tag}", env=env, pin=pin_analysis)
    def _():
        o = ops()
        geom = o.Geometry.make(N, C, M, sp, P, pad, s)
        d = _generic_data(*key)
        gen = torch.Generator().manual_seed(21)
        code = lambda: 0.3 * torch.randn(d["z"].shape, generator=gen) * (torch.rand(d["z"].shape, generator=gen) > 0.5)
        px = {"zp": code(), "za": code()}
        px.update({k: torch.rand(N, M, generator=gen) * sc + 0.01 for k, sc in (("lam", 0.2), ("g1", 1.2), ("g2", 1.2))})
        px["cmap"] = torch.rand((N, 1) + tuple(d["z"].shape[2:]), generator=gen)
        px["tslope"] = torch.rand(M, generator=gen) * 0.3

        def run(A):
            xd, wd, zd = A.i(d["x"], "x"), A.i(d["w"], "w"), A.i(d["z"], "z")
            o.analysis(geom, xd, wd, -1.0, zd, None, A.i(d["tau"], "tau"), out=A.o("iter", geom.code_shape()))
            o.analysis(geom, xd, wd, 1.0, A.i(d["u"], "gup"), zd, None, out=A.o("gated", geom.code_shape()))
            o.analysis_rev(geom, xd, wd, 0.5, A.i(d["u"], "zin"), zd, A.i(d["c"], "c"), A.o("dt_k", (2, M)),
                           out=A.o("rev", geom.code_shape()))
            o.analysis_prox(geom, xd, wd, -1.0, zd, A.i(px["zp"], "z_prev"), A.i(px["lam"], "lam"), A.i(px["g1"], "gam1"),
                            A.i(px["za"], "z_after"), A.i(px["g2"], "gam2"), u_out=A.o("prox_u", geom.code_shape()),
                            out=A.o("prox_z", geom.code_shape()))
            o.analysis(geom, xd, wd, -1.0, zd, None, A.i(d["tau"], "tau0"), out=A.o("mapped", geom.code_shape()),
                       cmap=A.i(px["cmap"], "cmap"), tslope=A.i(px["tslope"], "tslope"))

        @functools.lru_cache(maxsize=None)
        def refs():
            conv = O.analysis(d["x"].double(), d["w"].double(), s, pad)
            z64, u64 = d["z"].double(), d["u"].double()
            rev = (u64 + 0.5 * conv) * (z64 != 0)
            s_nm = -(torch.sign(z64) * rev).sum(dim=tuple(range(2, z64.dim())))
            thr = d["tau"].double().reshape(bsh) + px["cmap"].double() * px["tslope"].double().reshape((1, M) + (1,) * len(sp))
            return {"iter": (O.soft_threshold(z64 - conv, d["tau"].double().reshape(bsh)), 2 * tol),
                    "gated": (u64 * (z64 != 0) + conv, tol), "rev": (rev, tol),
                    "dt_k": (torch.stack([s_nm.sum(0), (d["c"].double()[:, None] * s_nm).sum(0)]), 2e-5),
                    "prox_u": (z64 - conv, tol), "mapped": (O.soft_threshold(z64 - conv, thr), 2 * tol)}

        def ref(got):
            # the CSR epilogue is the element-wise map of the u the kernel wrote, bit for bit (test_gpu_dispatch.py; the map
            # itself is pinned to the oracle's expression by test_gpu_csr.py)
            b = lambda v: v.reshape(bsh)
            z = O.prox_csr_f2(got["prox_u"], px["zp"], px["za"], b(px["lam"]), b(px["g1"]), b(px["g2"]))
            return dict(refs(), prox_z=(z, 0))
        return run, ref

    def pin_synthesis(sites, aligned, aligned_in):
        """Two calls: on the matrix-core tier two k_synth_m launches and two assembles, 16-byte form on aligned pointers."""
        (vec_or_scalar(K_ASM4, K_ASM1) if tier == "mfma" and sp[-1] % 4 == 0 else mfma_only(K_ASM1))(sites, aligned, aligned_in)
        if tier == "mfma":
            syn = [r for k, v in sites.items() if k.startswith("cdl_synth_mfma.hip:k_synth_m<") for r in v]
            asm = sites.get(K_ASM4, []) + sites.get(K_ASM1, [])
            assert len(syn) == 2 and len(asm) == 2, sorted(sites)

    @case(f"synthesis {tag}", env=env, pin=pin_synthesis)
    def _():
        o = ops()
        geom = o.Geometry.make(N, C, M, sp, P, pad, s)
        d = _generic_data(*key)
        mask = d["mask"] if masked else None

        def run(A):
            zd, wd, md = A.i(d["z"], "z"), A.i(d["w"], "w"), A.i(mask, "mask")
            o.synthesis(geom, zd, wd, 1.0, None, md, A.i(d["x"], "sub"), out=A.o("resid", geom.image_shape()))
            o.synthesis(geom, A.i(d["u"], "gup"), wd, -1.0, zd, md, None, out=A.o("gated", geom.image_shape()))

        @functools.lru_cache(maxsize=None)
        def refs():
            m64 = 1.0 if mask is None else mask.double()
            z64, w64 = d["z"].double(), d["w"].double()
            return {"resid": (m64 * O.synthesis(z64, w64, s, pad) - d["x"].double(), tol),
                    "gated": (-m64 * O.synthesis(d["u"].double() * (z64 != 0), w64, s, pad), tol)}
        return run, lambda got: refs()

    def pin_wgrad(sites, aligned, aligned_in):
        if tier != "mfma":
            assert not any(k.startswith("cdl_wgrad_mfma.hip") for k in sites), sorted(sites)
            return
        need(sites, K_WGM, "cdl_wgrad_mfma.hip:k_wgm_fold")
        wz = sp[-1] // s
        assert len(sites[K_WGM]) == 3 and len(sites["cdl_wgrad_mfma.hip:k_wgm_fold"]) >= 3, sorted(sites)
        assert [r.values()["pair"] for r in sites[K_WGM]] == [0, 0, 1]
        want = 1 if aligned_in and wz % 4 == 0 else 0            # the launcher's prediction of the kernel's own test of F / gate
        for r in sites[K_WGM]:
            v = r.values()
            assert v["vec4"] == want and v["vec4b"] == (want if v["pair"] else -1), (aligned_in, r.note)

    @case(f"wgrad {tag}", env=env, pin=pin_wgrad)
    def _():
        o = ops()
        geom = o.Geometry.make(N, C, M, sp, P, pad, s)
        d = _generic_data(*key)
        n = o._size("cdl_wgrad_workspace_floats", geom)
        fsh = geom.filter_shape()

        def run(A):
            zd, xd, ud = A.i(d["z"], "z"), A.i(d["x"], "x"), A.i(d["u"], "u")
            ws = A.ws("workspace", n)
            o._call("cdl_wgrad", geom, ud, zd, xd, 1.0, A.o("gated", fsh), ws, n)
            o._call("cdl_wgrad", geom, zd, None, xd, -2.0, A.o("plain", fsh), ws, n)
            o._call("cdl_wgrad_pair", geom, ud, xd, 1.0, A.o("pair0", fsh), zd, xd, -2.0, A.o("pair1", fsh), ws, n)

        @functools.lru_cache(maxsize=None)
        def refs():
            def grad(Fc):
                w = d["w"].double().requires_grad_(True)
                (O.analysis(d["x"].double(), w, s, pad) * Fc).sum().backward()
                return w.grad
            z64, u64 = d["z"].double(), d["u"].double()
            return {"gated": (grad(u64 * (z64 != 0)), wtol), "plain": (-2.0 * grad(z64), wtol),
                    "pair0": (grad(u64), wtol), "pair1": (-2.0 * grad(z64), wtol)}
        return run, lambda got: refs()


_ladder((2, 1, 11, (24, 40), (5, 5), 1), "valu", masked=False)
_ladder((2, 3, 9, (20, 24), (7, 7), 2), "valu")
_ladder((1, 1, 6, (6, 12, 16), (3, 5, 5), 1), "valu")
# the matrix-core tier at 256 compute units (test_gpu_dispatch.py's smallest shapes, W made a multiple of 8 so that the
# 16-byte assemble and k_wgm's fast path would be chosen but for the pointer); 9 x 9, M = 169, stride 2: fragments stream
_ladder((16, 1, 8, (60, 120), (5, 5), 1), "mfma")
_ladder((4, 1, 169, (72, 144), (9, 9), 2), "mfma")


# -------------------------------------------------------------------------------------- the fused iterations
def _stage_refs(d, s, pad, mask, got, tol):
    """Forward stage: z' against ST(z - A r) in float64; the assembled residual against the float64 synthesis of the
    kernel's own z' (isolates the second GEMM, as the existing stage tests do); the map is z' 's, exactly."""
    conv = O.analysis(d["r"].double(), d["wA"].double(), s, pad)
    u64 = conv if d["z"] is None else d["z"].double() - conv            # the first iteration: ST(A r)
    z64 = O.soft_threshold(u64, d["tau"].double().reshape(d["tau"].shape + (1,) * (conv.dim() - 2)))
    S = O.synthesis(got["z"].double(), d["wB"].double(), s, pad)
    m64 = 1.0 if mask is None else mask.double()
    return {"z": (z64, tol), "r_next": (m64 * S - d["yp"].double(), tol), "acc": (S, tol),
            "map": (support_map_ref(got["z"], got["map"].shape[1]).reshape(got["map"].shape), 0)}


def _next_ref(d, s, pad, z_got, tol):
    """The following stage fed the kernel's own z' (in an internal layout) and yp as its thin input."""
    u = z_got.double() - O.analysis(d["yp"].double(), d["wA"].double(), s, pad)
    return O.soft_threshold(u, d["tau"].double().reshape(d["tau"].shape + (1,) * (u.dim() - 2))), tol


def cdlnet_lib():
    import cdlnet_video_amd as cva
    return cva._lib.lib()


def _bwd_refs(d, s, pad, mask, got, tol):
    gate = d["z"].double() != 0
    du = (d["base"].double() + O.analysis(d["r"].double(), d["wA"].double(), s, pad)) * gate
    Sq = O.synthesis(got["du"].double(), d["wB"].double(), s, pad)
    m64 = 1.0 if mask is None else mask.double()
    s_nm = -(torch.sign(d["z"].double()) * du).sum(dim=tuple(range(2, du.dim())))
    return {"du": (du, tol), "q": (-m64 * Sq, 4 * tol), "acc": (d["dyp0"].double() + Sq, 4 * tol),
            "dt_k": (torch.stack([s_nm.sum(0), (d["c"].double()[:, None] * s_nm).sum(0)]), 4 * tol)}


def _stage_data(geom, masked, seed, fat=True):
    """fat=False: no code-shaped inputs (a first-iteration stage reads none)."""
    gen = torch.Generator().manual_seed(seed)
    ish, csh, fsh = geom.image_shape(), geom.code_shape(), geom.filter_shape()
    d = {"r": torch.randn(ish, generator=gen), "z": sparse(csh, gen) if fat else None,
         "wA": torch.randn(fsh, generator=gen) * 0.1,
         "wB": torch.randn(fsh, generator=gen) * 0.1, "tau": torch.rand(geom.N, geom.M, generator=gen) * 0.6 + 0.01,
         "yp": torch.randn(ish, generator=gen), "base": torch.randn(csh, generator=gen) if fat else None,
         "c": torch.rand(geom.N, generator=gen), "dyp0": torch.randn(ish, generator=gen)}
    d["mask"] = (torch.rand(ish, generator=gen) < 0.5).float() if masked else None
    return d


F2D = "cdl_fused2d.hip:"
K_STAGE2D = F2D + "k_stage<MT,PREC,MODE,LIN,LOUT,false,WY>"


def _fused2d(N, M, P, H, W, masked, modes=DEFAULT_MODES, big=False):
    tag = f"N{N}M{M}P{P} {H}x{W}"
    pad = (P // 2, P // 2)
    asm = (vec_or_scalar(F2D + "k_assemble_v4<WY>", F2D + "k_assemble<4,WY>", always=(K_STAGE2D,)) if big
           else only(K_STAGE2D, F2D + "k_assemble<1,WY>"))

    def setup():
        o = ops()
        geom = o.Geometry.make(N, 1, M, (H, W), (P, P), pad, 1)
        return o, geom, _stage_data(geom, masked, H * W + M, fat=not big)

    @case(f"fused_iter+assemble+support_map {tag}", pin=asm, modes=modes)
    def _():
        o, geom, d = setup()

        def run(A):
            frags = o.fused_prep(d["wA"].cuda(), d["wB"].cuda())
            patches = A.ws("patches", o._size("cdl_fused2d_patch_floats", geom))
            zout = A.o("z", geom.code_shape())
            o.fused_iter(geom, A.i(d["r"], "r"), None if big else A.i(d["z"], "zin"), A.i(d["tau"], "tau"), frags,
                         1.0 if big else -1.0, patches, out=zout, map_out=A.o("map", (N, 4, H, W), torch.int32))
            o.fused_assemble(geom, patches, A.i(d["mask"], "mask"), A.i(d["yp"], "sub"), 1.0,
                             out=A.o("r_next", geom.image_shape()), acc=A.o("acc", geom.image_shape()))
            if not big:
                o.fused_support_map(geom, zout, out=A.o("map2", (N, 4, H, W), torch.int32))
                # the pixel-blocked layout of the sweeps' internal codes: written, then read by the next stage
                nb = int(cdlnet_lib().cdl_fused2d_code_bytes(geom._c_ref(), o.LAYOUT["blocked"]))
                zb = A.lay("z_blocked", nb // 4, lambda t: o.fused_to_nchw(geom, t, "blocked"))
                o.fused_iter(geom, A.i(d["r"], "r2"), None, A.i(d["tau"], "tau2"), frags, 1.0, patches,
                             out=zb, lay_out="blocked")                                  # (a first stage: as the sweeps write it)
                o.fused_iter(geom, A.i(d["yp"], "r3"), zb, A.i(d["tau"], "tau3"), frags, -1.0, patches,
                             out=A.o("z_next", geom.code_shape()), lay_in="blocked")

        memo = {}

        def ref(got):
            key = torch.cat([got["z"].reshape(-1)] + ([] if big else [got["z_blocked"].reshape(-1)]))
            if "key" not in memo or not torch.equal(memo["key"], key):
                memo["key"], memo["ref"] = key, _stage_refs(d, 1, pad, d["mask"], got, MFMA_TOL)
                if not big:
                    memo["ref"]["map2"] = memo["ref"]["map"]
                    first = _stage_refs(dict(d, z=None), 1, pad, d["mask"], got, MFMA_TOL)["z"]      # ST(A r)
                    memo["ref"]["z_blocked"] = first
                    memo["ref"]["z_next"] = _next_ref(d, 1, pad, got["z_blocked"], MFMA_TOL)
            return memo["ref"]
        return run, ref

    if big:
        return

    @case(f"fused_stage_bwd+assemble+dtau_reduce+wgrad {tag}",
          pin=exactly({K_STAGE2D: 2, F2D + "k_assemble<1,WY>": 2, F2D + "k_dtau_reduce": 1, F2D + "k_wgrad2d<MT,PREC,LAY>": 2}),
          modes=modes)
    def _():
        o, geom, d = setup()
        tiles = o.fused_tiles(geom)

        def run(A):
            frags = o.fused_prep(d["wA"].cuda(), d["wB"].cuda())
            patches = A.ws("patches", o._size("cdl_fused2d_patch_floats", geom))
            gate = A.i(support_map_ref(d["z"], 4), "gate")
            dtp = A.ws("dtau_partial", tiles * M).reshape(tiles, M)
            du = A.o("du", geom.code_shape())
            o.fused_stage_bwd(geom, A.i(d["r"], "thin"), A.i(d["base"], "base"), gate, frags, patches, dtp, True, out=du)
            o.fused_assemble(geom, patches, A.i(d["mask"], "mask"), None, -1.0, out=A.o("q", geom.image_shape()),
                             acc=A.io("acc", d["dyp0"]), acc_add=True)
            o.fused_dtau_reduce(geom, dtp, A.i(d["c"], "c"), A.o("dt_k", (2, M)), A.o("dtau_n", (N, M)))
            ws = A.ws("wgrad_ws", o._size("cdl_fused2d_wgrad_workspace_floats", geom))
            fsh = geom.filter_shape()
            o._call("cdl_fused2d_wgrad", geom, du, A.i(d["yp"], "T0"), -1.0, A.o("dw0", fsh), A.i(d["z"], "X1"),
                    A.i(d["r"], "T1"), 1.0, A.o("dw1", fsh), ws, o.PRECISION["split3"] | o._lay_in("nchw"))
            # the same stage and filter gradients on codes in the pixel-blocked layout (what the sweeps keep between
            # launches): library-sized buffers at offset 0, their guards checked like any other
            nb = int(cdlnet_lib().cdl_fused2d_code_bytes(geom._c_ref(), o.LAYOUT["blocked"])) // 4
            to_nchw = lambda t: o.fused_to_nchw(geom, t, "blocked")
            base_b, z_b = A.lay("base_blocked", nb, to_nchw), A.lay("z_blocked", nb, to_nchw)
            base_b.copy_(o.fused_from_nchw(geom, d["base"].cuda(), "blocked"))
            z_b.copy_(o.fused_from_nchw(geom, d["z"].cuda(), "blocked"))
            du_b = A.lay("du_blocked", nb, to_nchw)
            o.fused_stage_bwd(geom, A.i(d["r"], "thin_b"), base_b, gate, frags, patches, dtp, True, out=du_b,
                              lay_in="blocked", lay_out="blocked")
            o.fused_assemble(geom, patches, None, None, -1.0, out=A.o("q_blocked", geom.image_shape()))
            o._call("cdl_fused2d_wgrad", geom, du_b, A.i(d["yp"], "T0b"), -1.0, A.o("dw0_blocked", fsh), z_b,
                    A.i(d["r"], "T1b"), 1.0, A.o("dw1_blocked", fsh), ws, o.PRECISION["split3"] | o._lay_in("blocked"))

        def ref(got):
            out = _bwd_refs(d, 1, pad, d["mask"], got, MFMA_TOL)
            du64 = out["du"][0]
            s_nm = -(torch.sign(d["z"].double()) * du64).sum(dim=(2, 3))
            out["dtau_n"] = (s_nm, 4 * MFMA_TOL)

            def grad(Fc, x):
                w = d["wA"].double().requires_grad_(True)
                (O.analysis(x.double(), w, 1, pad) * Fc.double()).sum().backward()
                return w.grad
            out["dw0"] = (-grad(got["du"], d["yp"]), MFMA_TOL)          # test_gpu_fused.py: 2e-5 against the generic wgrad
            out["dw1"] = (grad(d["z"], d["r"]), MFMA_TOL)
            # blocked: the inputs arrive as they were put, du has the NCHW run's bits, its patches and gradients hold the
            # same float64 bounds
            out["base_blocked"], out["z_blocked"] = (d["base"], 0), (d["z"], 0)
            out["du_blocked"] = (got["du"], 0)
            out["q_blocked"] = (-O.synthesis(got["du_blocked"].double(), d["wB"].double(), 1, pad), 4 * MFMA_TOL)
            out["dw0_blocked"], out["dw1_blocked"] = out["dw0"], out["dw1"]
            return out
        return run, ref


_fused2d(2, 32, 5, 48, 80, False)
_fused2d(2, 32, 7, 48, 80, True)
_fused2d(2, 64, 5, 48, 80, False)
_fused2d(2, 64, 7, 48, 80, True, modes=DEFAULT_MODES + ("off3",))
# the batch assemble (k_assemble_v4) engages from N H W >= 2^20: one first-iteration stage, M = 32, P = 5
_fused2d(16, 32, 5, 256, 256, False, big=True)


FG, SG, ST = "cdl_fusedg.hip:", "cdl_stripg.hip:", "cdl_strip.hip:"


def _fusedg(N, C, M, sp, P, s, masked, kernel, modes=DEFAULT_MODES):
    """The cdl_fusedg_* entry points: kernel "tile" (k_stage_g), "stripg" (cdl_stripg.hip, CDL_FUSEDG_STRIP=1) or
    "strip" (cdl_strip.hip: C = 1, 2-D, stride 1 or 2, M up to 192)."""
    tag = f"[{kernel}] N{N}C{C}M{M}{sp}P{P}s{s}"
    pad = tuple(p // 2 for p in P)
    env = {"CDL_FUSEDG_STRIP": "1"} if kernel == "stripg" else {}
    v4 = sp[-1] % 4 == 0
    Pn = P[-1]
    if kernel == "tile":
        stage = FG + "k_stage_g<P,G,MT,MODE,FOUR>"
        asm = (vec_or_scalar(FG + "k_assemble_g4<P_>", FG + "k_assemble_g<P_>", always=(stage,)) if v4
               else only(stage, FG + "k_assemble_g<P_>"))
    elif kernel == "stripg":
        asm = only(SG + "k_stripg<P,G,MT,MODE,MAPPED>", SG + "k_assemble_sg<P_>")
    else:
        stage = ST + "k_strip<P,S,MTP,MODE,MAPPED>"
        asm = (vec_or_scalar(ST + "k_assemble_s<P_,S_,4>", ST + "k_assemble_s<P_,S_,1>", always=(stage,)) if v4
               else only(stage, ST + "k_assemble_s<P_,S_,1>"))

    def setup():
        o = ops()
        geom = o.Geometry.make(N, C, M, sp, P, pad, s)
        return o, geom, _stage_data(geom, masked, sum(sp) + M)

    @case(f"fusedg_iter+assemble {tag}", pin=asm, env=env, modes=modes)
    def _():
        o, geom, d = setup()
        mshape = None

        def run(A):
            frags = o.fusedg_prep(geom, d["wA"].cuda(), d["wB"].cuda())
            patches = A.ws("patches", o._fusedg_sizes(geom)[1])
            o.fusedg_iter(geom, A.i(d["r"], "r"), A.i(d["z"], "zin"), A.i(d["tau"], "tau"), frags, -1.0, patches,
                          out=A.o("z", geom.code_shape()), map_out=A.o("map", o._fusedg_map_shape(geom), torch.int32))
            o.fusedg_assemble(geom, patches, A.i(d["mask"], "mask"), A.i(d["yp"], "sub"), 1.0,
                              out=A.o("r_next", geom.image_shape()), acc=A.o("acc", geom.image_shape()))
            if kernel == "strip":        # the row-strip channel-major layout of the sweeps' codes: written, then read
                zr = A.lay("z_rsc", o.fusedg_rsc_buffer(geom, "cpu").numel(), lambda t: o.fusedg_from_rsc(geom, t))
                o.fusedg_iter(geom, A.i(d["r"], "r2"), A.i(d["z"], "zin2"), A.i(d["tau"], "tau2"), frags, -1.0, patches,
                              out=zr, lay_out="rsc")
                o.fusedg_iter(geom, A.i(d["yp"], "r3"), zr, A.i(d["tau"], "tau3"), frags, -1.0, patches,
                              out=A.o("z_next", geom.code_shape()), lay_in="rsc")

        memo = {}

        def ref(got):
            if "z" not in memo or not torch.equal(memo["z"], got["z"]):
                memo["z"], memo["ref"] = got["z"], _stage_refs(d, s, pad, d["mask"], got, MFMA_TOL)
                if kernel == "strip":
                    memo["ref"]["z_rsc"] = (got["z"], 0)                      # the same values in another layout
                    memo["ref"]["z_next"] = _next_ref(d, s, pad, got["z"], MFMA_TOL)
            return memo["ref"]
        return run, ref

    @case(f"fusedg_stage_bwd+assemble+dtau_reduce {tag}", pin=asm, env=env, modes=modes)
    def _():
        o, geom, d = setup()
        items = o._fusedg_sizes(geom)[2]

        def run(A):
            frags = o.fusedg_prep(geom, d["wA"].cuda(), d["wB"].cuda())
            patches = A.ws("patches", o._fusedg_sizes(geom)[1])
            planes = o._fusedg_map_shape(geom)[1]
            gate = A.i(support_map_ref(d["z"], planes).reshape(o._fusedg_map_shape(geom)), "gate_map")
            dtp = A.ws("dtau_partial", items * M).reshape(items, M)
            o.fusedg_stage_bwd(geom, A.i(d["r"], "thin"), A.i(d["base"], "base"), gate, frags, patches, dtp, True,
                               out=A.o("du", geom.code_shape()))
            o.fusedg_assemble(geom, patches, A.i(d["mask"], "mask"), None, -1.0, out=A.o("q", geom.image_shape()),
                              acc=A.io("acc", d["dyp0"]), acc_add=True)
            o.fusedg_dtau_reduce(geom, dtp, A.i(d["c"], "c"), A.o("dt_k", (2, M)))

        return run, lambda got: _bwd_refs(d, s, pad, d["mask"], got, MFMA_TOL)


for _kernel in ("tile", "stripg"):
    _fusedg(2, 1, 48, (6, 20, 40), (5, 5, 5), 1, False, _kernel)
    _fusedg(1, 3, 64, (32, 72), (7, 7), 1, True, _kernel)
_fusedg(2, 1, 169, (64, 128), (7, 7), 2, False, "strip")
_fusedg(1, 1, 169, (150, 154), (7, 7), 2, True, "strip")


# ----------------------------------------------------------------------------------------- ResidualBlock tier
DEN = "cdl_dense_mfma.hip:"


def _residual(N, M, shape, dense=True):
    vec = shape[-1] % 4 == 0

    def pin(sites, aligned, aligned_in):
        if not dense:
            # CDL_MFMA_DENSE=0: the sparse ladder's analysis with the ReLU as a pass of its own over h and out (carved at the
            # output offset): four elements per thread on a 16-byte aligned buffer, one otherwise
            assert not any(k.startswith(DEN) for k in sites), sorted(sites)
            need(sites, "cdl_residual.hip:k_relu", "cdl_residual.hip:k_add_gated")
            relu = sites["cdl_residual.hip:k_relu"]
            assert len(relu) == 2 and all(r.values()["vec4"] == (1 if aligned else 0) for r in relu), [r.note for r in relu]
            return
        need(sites, DEN + "k_dense<MT>", "cdl_residual.hip:k_gate", DEN + "k_dense_wfold")
        want = "true" if vec and aligned else "false"
        need(sites, DEN + f"k_dense_wgrad<{want}>")
        forbid(sites, DEN + f"k_dense_wgrad<{'false' if want == 'true' else 'true'}>")

    @case(f"residual forward+backward{'' if dense else ' [sparse ladder]'} M{M} {shape}", pin=pin,
          env={} if dense else {"CDL_MFMA_DENSE": "0"})
    def _():
        o = ops()
        gen = torch.Generator().manual_seed(100 + M)
        x = torch.randn((N, M) + shape, generator=gen) * 0.5
        w1 = torch.randn((M, M, 3, 3, 3), generator=gen) / (27 * M) ** 0.5
        w2 = torch.randn((M, M, 3, 3, 3), generator=gen) / (27 * M) ** 0.5
        wgt = torch.randn((N, M) + shape, generator=gen)
        geom = o.residual_geometry(x, w1)
        n = o._size("cdl_residual_scratch_floats", geom)

        def run(A):
            xd, w1d, w2d = A.i(x, "x"), A.i(w1, "w1"), A.i(w2, "w2")
            scratch = A.ws("scratch", n)
            h, out = A.o("h", x.shape), A.o("out", x.shape)
            o._call("cdl_residual_forward", geom, xd, w1d, w2d, h, out, scratch if n else None, n)
            o._call("cdl_residual_backward", geom, xd, h, out, w1d, w2d, A.i(wgt, "g_out"), A.o("dx", x.shape),
                    A.o("dw1", w1.shape), A.o("dw2", w2.shape), A.o("dh", x.shape), scratch if n else None, n)

        def ref(got):
            # tests/test_gpu_residual.py: 1e-5 forward; the backward against autograd on float64 convolutions with the
            # PRODUCT's two gates (the block is linear given them), 2e-5
            x64, w164, w264 = (t.double().requires_grad_(True) for t in (x, w1, w2))
            ref_h = torch.relu(F.conv3d(x.double(), w1.double(), padding=1))
            ref_out = torch.relu(F.conv3d(ref_h, w2.double(), padding=1) + x.double())
            G1, G2 = got["h"] != 0, got["out"] != 0
            pre = F.conv3d(x64, w164, padding=1) * G1
            lin = (F.conv3d(pre, w264, padding=1) + x64) * G2
            pre.retain_grad()
            (lin * wgt.double()).sum().backward()
            if not dense:           # tests/test_gpu_residual.py, the r0 block below the dense tier: 1e-5 forward, 1e-4 gradients;
                gt = 1e-4           # dh is dL/d(conv1 x . [h > 0]) before the gate of h
                return {"h": (ref_h, 1e-5), "out": (ref_out, 1e-5), "dx": (x64.grad, gt), "dw1": (w164.grad, gt),
                        "dw2": (w264.grad, gt), "dh": (pre.grad, gt)}
            return {"h": (ref_h, 1e-5), "out": (ref_out, 1e-5), "dx": (x64.grad, 2e-5), "dw1": (w164.grad, 2e-5),
                    "dw2": (w264.grad, 2e-5), "dh": (pre.grad * G1, 2e-5)}
        return run, ref


_residual(1, 16, (4, 8, 8))
_residual(2, 32, (3, 17, 33))
_residual(1, 48, (5, 24, 36))
_residual(1, 16, (4, 8, 8), dense=False)


# ------------------------------------------------------------------------------------------------------ SSIM
def _ssim(shape, win_size):
    N, C, H, W = shape
    P = N * C

    @case(f"ssim fwd+bwd {shape} win {win_size}", pin=only("cdl_ssim.hip:k_ssim_fwd", "cdl_ssim.hip:k_ssim_bwd"))
    def _():
        import ctypes
        import cdlnet_video_amd as cva
        o = cva.ops
        # the inputs of tests/test_gpu_ssim.py::test_ssim_gradients: seed 11 + win, a weight per image on the channel mean
        x = cva.utils.synthetic_clip(shape, seed=11 + win_size)
        y = x + 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(11 + win_size + 100))
        w = torch.rand(N, generator=torch.Generator().manual_seed(5)) + 0.5
        g = (w / C).repeat_interleave(C).contiguous()            # upstream per plane
        rng = torch.full((P,), 1.2)
        win = cva.metrics._gaussian_window(win_size, 1.5)
        warg = (ctypes.c_float * len(win))(*win)

        def run(A):
            n = int(cva._lib.lib().cdl_ssim_scratch_floats(P, H, W, len(win)))
            scratch = A.ws("scratch", n)
            xd, yd, rd = A.i(x.reshape(P, H, W), "x"), A.i(y.reshape(P, H, W), "y"), A.i(rng, "R")
            o._call("cdl_ssim_fwd", xd, yd, P, H, W, warg, len(win), 0.01, 0.03, 1.0, rd, A.o("ssim", (P,)), None, scratch, n)
            o._call("cdl_ssim_bwd", xd, yd, P, H, W, warg, len(win), 0.01, 0.03, 1.0, rd, A.i(g, "g"), A.o("dx", (P, H, W)),
                    A.o("dy", (P, H, W)), A.o("dr", (P,)), scratch, n)

        @functools.lru_cache(maxsize=None)
        def refs():
            # tests/test_gpu_ssim.py: the bound is the restatement's own fp32 error against float64, doubled (at least 1e-6)
            def run_ref(dtype):
                a, b, r = (t.detach().to(dtype).requires_grad_() for t in (x, y, rng))
                pc = SR.ssim_per_channel(a, b, r.reshape(N, C, 1, 1), win_size).reshape(P)
                (pc * g.to(dtype)).sum().backward()
                return {"ssim": pc.detach(), "dx": a.grad.reshape(P, H, W), "dy": b.grad.reshape(P, H, W), "dr": r.grad}
            r64, r32 = run_ref(torch.float64), run_ref(torch.float32)
            err = lambda a, b: float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))
            return {k: (r64[k], max(1e-6, 2 * err(r32[k], r64[k]))) for k in r64}
        return run, lambda got: refs()


_ssim((2, 3, 37, 53), 11)
_ssim((1, 1, 11, 11), 11)


# --------------------------------------------------------------------------------------------------- nle_mad
def _nle_mad(shape):
    N, C, H, W = shape

    @case(f"nle_mad {shape}", pin=only("cdl_nle.hip:k_hh_abs", "cdl_nle.hip:k_select"))
    def _():
        import cdlnet_video_amd as cva
        gen = torch.Generator().manual_seed(sum(shape))
        y = torch.rand(shape, generator=gen) + torch.randn(shape, generator=gen) * 0.1

        def run(A):
            n = int(cva._lib.lib().cdl_nle_mad_scratch_floats(N, C, H, W))
            cva.ops._call("cdl_nle_mad", A.i(y, "y"), A.o("sigma", (N,)), A.ws("scratch", n), n, N, C, H, W)
        # tests/test_nle.py::test_hip_estimate_equals_oracle: 1e-5 against the oracle (a median: a selection, not a sum)
        def ref(got):                                            # the oracle's O.nle_mad in float64
            hh = torch.cat([O.hh_filter().double()] * C)
            band = F.conv2d(y.double(), hh, stride=2, groups=C)
            return {"sigma": (torch.median(band.abs().reshape(N, -1), dim=1)[0] / 0.6745, 1e-5)}
        return run, ref


_nle_mad((1, 1, 10, 10))
_nle_mad((2, 3, 37, 53))


# ------------------------------------------------------------------------------------- the VGG perceptual term
def _vgg(shape):
    B, _, T, H, W = shape
    P = B * T

    @case(f"vgg perceptual fwd+bwd {shape}",
          pin=only("cdl_dense_mfma.hip:k_dense_vgg<MODE>", "cdl_vgg.hip:k_vgg_conv11", "cdl_vgg.hip:k_vgg_fold"))
    def _():
        import cdlnet_video_amd as cva
        # the inputs of tests/test_gpu_perceptual.py::test_value_and_gradients
        sd = PR.random_weights(shape[-2])
        x = cva.utils.synthetic_clip(shape, seed=sum(shape) + 7)
        out = (x + 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(sum(shape) + 8))).clamp(0, 1)
        g = torch.tensor(0.7)

        def run(A):
            ws = [A.i(sd[f"{i}.weight"], f"w{i}") for i in PR.CONVS]
            bs = [A.i(sd[f"{i}.bias"], f"b{i}") for i in PR.CONVS]
            n = int(cva._lib.lib().cdl_vgg_scratch_floats(P, H, W, 3))
            scratch = A.ws("scratch", n)                         # the library's own: 16 bytes, kept between the two calls
            cva.ops._call("cdl_vgg_forward", A.i(out.reshape(P, H, W), "x"), A.i(x.reshape(P, H, W), "y"), P, H, W, ws, bs, 3,
                          None, A.o("loss", ()), scratch, n)
            cva.ops._call("cdl_vgg_backward", P, H, W, ws, bs, 3, A.i(g, "g"), A.o("dx", (P, H, W)), A.o("dy", (P, H, W)),
                          scratch, n)

        @functools.lru_cache(maxsize=None)
        def refs():
            def run_ref(dtype):
                o_, t_ = out.to(dtype).requires_grad_(), x.to(dtype).requires_grad_()
                v = PR.perceptual(o_, t_, {k: w.to(dtype) for k, w in sd.items()})
                (0.7 * v).backward()
                return v.detach().reshape(()), o_.grad.reshape(P, H, W), t_.grad.reshape(P, H, W)
            (v64, dx64, dy64), (v32, _, _) = run_ref(torch.float64), run_ref(torch.float32)
            err = float((v32.double() - v64).abs() / v64.abs())
            # the value: the restatement's own fp32 error doubled, floor 5e-5; the gradients against the free restatement: a
            # ReLU gate or near-tied pool window that rounds the other way moves whole contributions, so the l2 error is gated
            return {"loss": (v64, max(5e-5, 2 * err)), "dx": (dx64, ("l2", 5e-2)), "dy": (dy64, ("l2", 5e-2))}
        return run, lambda got: refs()


_vgg((1, 1, 3, 37, 50))


# --------------------------------------------------------------------------------------------------- nle_pca
PCA = "cdl_nle_pca.hip:"


def _pin_pca(sites, aligned, aligned_in):
    need(sites, PCA + "k_pca_reduce1", PCA + "k_pca_reduce2")
    assert any(k.startswith(PCA + "k_pca_gram<") for k in sites) and all(k.startswith(PCA) for k in sites), sorted(sites)


@case("nle_pca_gram n1 finite tau", pin=_pin_pca)
def _():
    import cdlnet_video_amd as cva
    f = NR.load("n1")
    y, p = torch.from_numpy(f["y"]).float().contiguous(), int(f["patchsize"])
    N, C, H, W = y.shape
    tau, _ = NR.gap_threshold(NR.texture(y[:, 0], p), 0.5)       # tests/test_gpu_nle_pca.py, finite = True

    def run(A):
        n = int(cva._lib.lib().cdl_nle_pca_scratch_floats(N, C, H, W, p))
        cva.ops._call("cdl_nle_pca_gram", A.i(y, "y"), N, C, H, W, 0, p, tau, A.o("gram", (p * p, p * p), torch.float64),
                      A.o("count", (1,), torch.int64), A.ws("scratch", n), n)

    @functools.lru_cache(maxsize=None)
    def refs():
        ref, nref = NR.gram(y[:, 0], p, tau)
        return {"gram": (ref, ("f64", 1e-6)), "count": (torch.tensor([nref]), 0)}        # 1e-6 and the exact count

    def ref(got):
        assert torch.equal(got["gram"], got["gram"].T)
        return refs()
    return run, ref


@case("nle_pca_gram_cells p7 finite tau", pin=_pin_pca)
def _():
    import cdlnet_video_amd as cva
    (H, W), N, w, q, p, itr, seed = NC.PARITY_CASES["p7"]       # tests/test_gpu_nle_pca_cells.py, finite = True
    y = NC.noisy(N, H, W, seed)
    ys, xs = NC.cell_ranges(H, w, q), NC.cell_ranges(W, w, q)
    crops = [((n, iy, ix), y[n:n + 1, :, y0:y1, x0:x1]) for n in range(N) for iy, (y0, y1) in enumerate(ys)
             for ix, (x0, x1) in enumerate(xs)]
    tau = torch.full((N, len(ys), len(xs)), float("inf"), dtype=torch.float32)
    for idx, crop in crops:
        tau[idx] = NR.gap_threshold(NR.texture(crop[:, 0], p), 0.5)[0]

    def run(A):
        n = int(cva._lib.lib().cdl_nle_pca_gram_cells_scratch_floats(N, 1, H, W, p, w, q))
        cva.ops._call("cdl_nle_pca_gram_cells", A.i(y, "y"), N, 1, H, W, 0, p, w, q, A.i(tau, "tau"),
                      A.o("gram", tuple(tau.shape) + (p * p, p * p), torch.float64), A.o("count", tuple(tau.shape), torch.int64),
                      A.ws("scratch", n), n)

    @functools.lru_cache(maxsize=None)
    def refs():
        gram = torch.zeros(tuple(tau.shape) + (p * p, p * p), dtype=torch.float64)
        count = torch.zeros(tuple(tau.shape), dtype=torch.int64)
        for idx, crop in crops:
            gram[idx], count[idx] = NR.gram(crop[:, 0], p, float(tau[idx]))
        return gram, count

    def ref(got):
        gram, count = refs()
        # GRAM_TOL = 1e-6 per cell (each cell against its own maximum), exact counts, exactly symmetric
        worst = max(float((got["gram"][idx] - gram[idx]).abs().max() / gram[idx].abs().max()) for idx, _ in crops)
        assert worst < 1e-6, f"nle_pca_gram_cells: worst relative deviation of a cell {worst:.3e} >= 1e-6"
        assert torch.equal(got["gram"], got["gram"].transpose(-1, -2))
        return {"count": (count, 0)}
    return run, ref


# ------------------------------------------------------------------ refusals: library-sized buffers need 16 bytes
def _refusals():
    """name -> fn(A, bad): a call with ONE library-sized buffer (fragments, patches, a blocked or rsc code buffer) 4-byte
    aligned and everything else aligned.  bad(n): such a float32 buffer; bad(n, torch.uint8): fragment bytes."""
    o = ops()
    P32 = o.PRECISION["split3"]
    g2 = o.Geometry.make(2, 1, 32, (48, 80), (5, 5), (2, 2), 1)                       # fused 2-D
    gt = o.Geometry.make(1, 3, 64, (32, 72), (7, 7), (3, 3), 1)                       # tile kernel
    gs = o.Geometry.make(2, 1, 169, (64, 128), (7, 7), (3, 3), 2)                     # strip kernel

    def common(A, g):
        z = lambda shape: torch.zeros(shape)
        return dict(r=A.i(z(g.image_shape()), "r"), code=A.i(z(g.code_shape()), "code"), tau=A.i(torch.ones(g.N, g.M), "tau"),
                    out=A.o("out", g.code_shape()), wA=A.i(z(g.filter_shape()), "wA"), wB=A.i(z(g.filter_shape()), "wB"))

    def fused(what):
        def fn(A, bad):
            c = common(A, g2)
            nfr, npt = int(cdlnet_lib().cdl_fused2d_frag_bytes(32)), o._size("cdl_fused2d_patch_floats", g2)
            nb = int(cdlnet_lib().cdl_fused2d_code_bytes(g2._c_ref(), o.LAYOUT["blocked"])) // 4
            frags = bad(nfr, torch.uint8) if "frags" in what else torch.zeros(nfr, dtype=torch.uint8, device="cuda")
            patches = bad(npt) if "patches" in what else A.ws("patches", npt)
            gate = A.i(torch.zeros((2, 4, 48, 80), dtype=torch.int32), "gate")
            dtp = A.ws("dtp", o.fused_tiles(g2) * 32)
            blk = lambda hit: bad(nb) if hit else A.ws("blk", nb)
            if what == "prep frags":
                o._call("cdl_fused2d_prep", c["wA"], c["wB"], frags, 32, 5)
            elif what.startswith("iter"):
                lin, lout = "zin" in what, "zout" in what
                o.fused_iter(g2, c["r"], blk(True) if lin else c["code"], c["tau"], frags, -1.0, patches,
                             out=blk(True) if lout else c["out"], lay_in="blocked" if lin else "nchw",
                             lay_out="blocked" if lout else "nchw")
            elif what.startswith("bwd"):
                lin, lout = "base" in what, "du_out" in what
                o.fused_stage_bwd(g2, c["r"], blk(True) if lin else c["code"], gate, frags, patches, dtp, True,
                                  out=blk(True) if lout else c["out"], lay_in="blocked" if lin else "nchw",
                                  lay_out="blocked" if lout else "nchw")
            else:
                ws = A.ws("wgrad_ws", o._size("cdl_fused2d_wgrad_workspace_floats", g2))
                X0, X1 = (blk("X0" in what), blk("X1" in what))
                o._call("cdl_fused2d_wgrad", g2, X0, c["r"], 1.0, A.o("dw0", g2.filter_shape()), X1, c["r"], 1.0,
                        A.o("dw1", g2.filter_shape()), ws, P32 | o._lay_in("blocked"))
        return fn

    def fusedg(g, what):
        def fn(A, bad):
            c = common(A, g)
            nfr, npt, items, _ = o._fusedg_sizes(g)
            nr = o.fusedg_rsc_buffer(g, "cpu").numel() if g is gs else 0
            frags = bad(nfr, torch.uint8) if "frags" in what else torch.zeros(nfr, dtype=torch.uint8, device="cuda")
            patches = bad(npt) if "patches" in what else A.ws("patches", npt)
            gate = A.i(torch.zeros(o._fusedg_map_shape(g), dtype=torch.int32), "gate")
            dtp = A.ws("dtp", items * g.M)
            if what == "prep frags":
                o._call("cdl_fusedg_prep", g, c["wA"], c["wB"], frags)
            elif what.startswith("iter"):
                lin, lout = "zin" in what, "zout" in what
                o.fusedg_iter(g, c["r"], bad(nr) if lin else c["code"], c["tau"], frags, -1.0, patches,
                              out=bad(nr) if lout else c["out"], lay_in="rsc" if lin else "nchw", lay_out="rsc" if lout else "nchw")
            else:
                lin, lout = "base" in what, "du_out" in what
                o.fusedg_stage_bwd(g, c["r"], bad(nr) if lin else c["code"], gate, frags, patches, dtp, True,
                                   out=bad(nr) if lout else c["out"], lay_in="rsc" if lin else "nchw",
                                   lay_out="rsc" if lout else "nchw")
        return fn

    table = {}
    for what in ("prep frags", "iter frags", "iter patches", "iter blocked zin", "iter blocked zout", "bwd frags", "bwd patches",
                 "bwd blocked base", "bwd blocked du_out", "wgrad blocked X0", "wgrad blocked X1"):
        table["fused2d " + what] = fused(what)
    for what in ("prep frags", "iter frags", "iter patches", "bwd frags", "bwd patches"):
        table["tile " + what] = fusedg(gt, what)
    for what in ("prep frags", "iter frags", "iter rsc zin", "iter rsc zout", "bwd rsc base", "bwd rsc du_out"):
        table["strip " + what] = fusedg(gs, what)
    return table


REFUSALS = ["fused2d " + w for w in ("prep frags", "iter frags", "iter patches", "iter blocked zin", "iter blocked zout",
                                     "bwd frags", "bwd patches", "bwd blocked base", "bwd blocked du_out", "wgrad blocked X0",
                                     "wgrad blocked X1")] + \
           ["tile " + w for w in ("prep frags", "iter frags", "iter patches", "bwd frags", "bwd patches")] + \
           ["strip " + w for w in ("prep frags", "iter frags", "iter rsc zin", "iter rsc zout", "bwd rsc base", "bwd rsc du_out")]


@pytest.mark.parametrize("name", REFUSALS)
def test_misaligned_library_buffer_is_refused_before_any_launch(name):
    """The exception of the alignment contract: fragment, patch and internal-layout code buffers at a 4-byte aligned base
    give CDL_EUNSUPPORTED -- no launch, no word written anywhere."""
    import cdlnet_video_amd as cva
    table = _refusals()
    assert sorted(table) == sorted(REFUSALS)
    A = Carve("off0")
    hit = []

    def bad(n, dtype=torch.float32):
        if dtype == torch.uint8:
            v = torch.zeros(int(n) + 16, dtype=torch.uint8, device="cuda")[4:4 + int(n)]
        else:
            v = A.arena.out((int(n),), 1, dtype, "misaligned")
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        hit.append(v)
        return v

    with cva.ops.trace() as t:
        with pytest.raises(cva.HipKernelError, match="CDL_EUNSUPPORTED"):
            table[name](A, bad)
        torch.cuda.synchronize()
    assert len(hit) == 1, "the case must misalign exactly one buffer"
    assert len(t) == 0, list(t)
    A.arena.check()
    for b in A.arena.bufs:
        if b.is_output:
            assert A.arena.undefined(b.view).numel() == b.view.numel(), f"{b.name} was written"


# ------------------------------------------------------------------------------------------------ the tests
PARAMS = [pytest.param(c, m, id=f"{c.name}-{m}") for c in CASES for m in c.modes]


@pytest.mark.parametrize("case_,mode", PARAMS)
def test_operator_on_guard_banded_buffers(case_, mode, hip_env):
    run_case(case_, mode, hip_env)


def test_every_case_has_the_offsets_the_contract_names():
    """off = 0, 1, 2 and the output-only offset for every operator."""
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert {"off0", "off1", "off2", "out1"} <= set(c.modes), c.name
