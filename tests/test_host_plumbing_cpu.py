"""The host side of every launch, without a device: ops._call is the one way into a stream-taking entry point and
refuses a tensor that is no contiguous tensor of the current ROCm device before the library is entered; ops._buf checks
the outputs and work buffers a caller provides; ops._sweep_tables builds the ping-pong tables of the seven one-call
sweeps; loop._save / loop._saved name what an autograd node keeps; loop._route and loop._TIERS choose a sweep's tier and
name what the nodes call on it."""
import ast
import os

import pytest
import torch

from conftest import ROOT

import cdlnet_video_amd as cva
from cdlnet_video_amd import _lib, loop, ops


class _NoEntry:
    """Stands in for the loaded library: entering any entry point fails the test."""

    def __getattr__(self, name):
        pytest.fail(f"the library was entered ({name})")


@pytest.fixture
def no_library(monkeypatch):
    """No entry point may be reached, and the inputs count as checked: what is left to refuse a bad pointer is the check
    of the caller-provided buffers (`_dev` would refuse the CPU inputs first, which is not what these tests are about)."""
    monkeypatch.setattr(_lib, "lib", lambda: _NoEntry())
    monkeypatch.setattr(ops, "_dev", lambda t, name: t)


N, C, M, H, W, K = 2, 1, 4, 6, 7, 2
G = ops.Geometry.make(N, C, M, (H, W), (3, 3), (1, 1), 1)


def _code():
    return torch.zeros(G.code_shape())


def _thin():
    return torch.zeros(G.image_shape())


def _slots():
    """(id, slot, call): every call hands CPU tensors to a wrapper; `slot` is the caller-provided output / work buffer
    under test."""
    z, x, dt_k, rows = _code(), _thin(), torch.zeros(2, M), torch.zeros(N, M)
    cmap, slope3 = torch.zeros((N, 1, H, W)), torch.zeros(3, M)
    w = torch.zeros(G.filter_shape())
    frags, patches, bits = torch.zeros(8, dtype=torch.uint8), torch.zeros(8), torch.zeros((N, 4, H, W), dtype=torch.int32)
    tau_grad = lambda: ops.tau_grad(G, z, z, None, dt_k, rows)
    prox = lambda: ops.prox_csr_bwd(G, z, z, z, rows, rows, None, dt_k, dt_k, gz_prev=z, dsum_n=torch.zeros(3, N, M))
    prox_map = lambda: ops.prox_csr_bwd(G, z, z, z, rows, rows, None, dt_k, dt_k, cmap=cmap, tslope=slope3, dcmap=cmap)
    fused_iter = lambda: ops.fused_iter(G, x, None, rows, frags, 1.0, patches, out=z, map_out=bits)
    sweep = lambda: ops.ista_backward(G, x, None, None, [w] * K, [w] * K, [z] * K, [x] * (K - 1), x, None,
                                      torch.zeros(K, 2, M), gz_prev=z)
    return [
        ("dyp_split", "q", lambda: ops.dyp_split(G, x, None, x, False)),
        ("dyp_split", "dyp", lambda: ops.dyp_split(G, x, None, x, False)),
        ("tau_grad", "dt_k", tau_grad),
        ("tau_grad", "dtau_n", tau_grad),
        ("sigma_grad", "dcmap", lambda: ops.sigma_grad(G, z, z, torch.zeros(M), cmap, False)),
        ("prox_csr_bwd", "dlam", prox),
        ("prox_csr_bwd", "gz_prev", prox),
        ("prox_csr_bwd", "dsum_n", prox),
        ("prox_csr_bwd", "dcmap", prox_map),
        ("fused_assemble", "patches", lambda: ops.fused_assemble(G, patches, acc=x)),
        ("fused_assemble", "acc", lambda: ops.fused_assemble(G, patches, acc=x)),
        ("fused_iter", "frags", fused_iter),
        ("fused_iter", "map_out", fused_iter),
        ("ista_backward", "dt", sweep),
        ("ista_backward", "gz_prev", sweep),
    ]


@pytest.mark.parametrize("slot,call", [pytest.param(s, c, id=f"{fn}-{s}") for fn, s, c in _slots()])
def test_cpu_tensor_in_a_buffer_slot_is_refused_in_python(no_library, monkeypatch, slot, call):
    """The buffer's own check refuses it, before any entry point -- a size query included -- is reached (the other
    buffers of the call are let through to show that it is this one's)."""
    buf = ops._buf
    monkeypatch.setattr(ops, "_buf", lambda t, name, *a, **kw: buf(t, name, *a, **kw) if name == slot else t)
    with pytest.raises(RuntimeError, match=rf"^{slot} is on cpu"):
        call()


def test_buf_checks_without_copying():
    assert ops._buf(None, "b") is None
    with pytest.raises(TypeError, match="b: expected a tensor"):
        ops._buf([1.0], "b")
    with pytest.raises(RuntimeError, match="b is on cpu"):          # `is_cuda` comes first: the check needs no device
        ops._buf(torch.zeros(4, 6, dtype=torch.float64)[:, ::2], "b", (3, 3))


def test_call_refuses_a_wrong_argument_count_and_a_host_pointer(no_library):
    nargs = len(_lib.SIGNATURES["cdl_thresholds"]) - 1
    for n in (nargs - 1, nargs + 1):
        with pytest.raises(TypeError, match="cdl_thresholds: takes 6 arguments before the stream"):
            ops._call("cdl_thresholds", *([None] * n))
    t = torch.zeros(3)
    with pytest.raises(RuntimeError, match="cdl_thresholds: argument 2 is on cpu"):
        ops._call("cdl_thresholds", None, None, t, 1, 1, 3)
    with pytest.raises(RuntimeError, match="cdl_project_filter_banks: argument 0 is on cpu"):     # an entry of a pointer table
        ops._call("cdl_project_filter_banks", [t, t], 2, 1, 3)


def test_every_call_site_passes_what_the_signature_declares():
    """A literal `_call("name", ...)` site has the entry point's argument count (the stream is appended): checked where
    the site spells its arguments out, i.e. has no starred argument."""
    seen = 0
    for mod in ("ops", "metrics", "nle"):
        tree = ast.parse(open(os.path.join(ROOT, "cdlnet-video_amd", mod + ".py")).read())
        for node in ast.walk(tree):
            if not (isinstance(node, ast.Call) and getattr(node.func, "id", getattr(node.func, "attr", None)) == "_call"):
                continue
            if not isinstance(node.args[0], ast.Constant) or any(isinstance(a, ast.Starred) for a in node.args):
                continue
            name = node.args[0].value
            assert len(node.args) - 1 == len(_lib.SIGNATURES[name]) - 1, (mod, node.lineno, name)
            seen += 1
    assert seen >= 40


# ------------------------------------------------------------------------------------------ buffer tables
class _Buf:
    def __init__(self, family, i):
        self.family, self.i = family, i


def _alloc(family, counts):
    def alloc(n):
        counts.append(n)
        return [_Buf(family, i) for i in range(n)]
    return alloc


def _parent_tables(K, keep, separate, zbuf, rbuf, zK):
    """The expressions of the sweeps before the helper, restated literally (ops.fused_forward / ops.ista_forward)."""
    if separate:
        nz = (K - 1) if keep else min(K - 1, 2)
        nr = (K - 1) if keep else min(K - 1, 2)
        z = [zbuf[k % nz] for k in range(K - 1)] + [zK]
    else:
        nz = K if keep else min(K, 2)
        nr = (K - 1) if keep else min(K - 1, 2)
        z = [zbuf[k % nz] for k in range(K)]
    r = [rbuf[k % nr] for k in range(K - 1)] if K > 1 else []
    return z, r, max(nz, 1), max(nr, 1)


@pytest.mark.parametrize("separate", [False, True])
@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sweep_tables(K, keep, separate):
    zc, rc = [], []
    zK = _Buf("zK", 0) if separate else None
    z, r = ops._sweep_tables(K, keep, _alloc("z", zc), _alloc("r", rc), z_K=zK)
    assert len(z) == K and len(r) == K - 1
    for table in (z, r):
        assert all(table[k] is not table[k - 1] for k in range(1, len(table)))
        if keep:
            assert len({id(b) for b in table}) == len(table)
    if separate:
        assert z[-1] is zK
    # the parent's tables over the same buffers, and its allocation sizes
    zbuf, rbuf = [_Buf("z", i) for i in range(max(K, 1))], [_Buf("r", i) for i in range(max(K, 1))]
    pz, pr, nz, nr = _parent_tables(K, keep, separate, zbuf, rbuf, zK)
    assert zc == [nz] and rc == [nr]
    assert [(b.family, b.i) for b in z] == [(b.family, b.i) for b in pz]
    assert [(b.family, b.i) for b in r] == [(b.family, b.i) for b in pr]


# ------------------------------------------------------------------------------------------ named saves
def test_named_saves_round_trip_through_a_function():
    seen = {}

    class Toy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, a, b, c):
            loop._save(ctx, x=x, nothing=None, three=[a, b, c], none_yet=[], last=c)
            return x * 2

        @staticmethod
        def backward(ctx, g):
            sv = loop._saved(ctx)
            seen.update(vars(sv))
            return g * 2, None, None, None

    x = torch.ones(3, requires_grad=True)
    a, b, c = torch.zeros(1), torch.ones(2), torch.full((3,), 2.0)
    Toy.apply(x, a, b, c).sum().backward()
    assert list(seen) == ["x", "nothing", "three", "none_yet", "last"]
    assert seen["x"] is x and seen["nothing"] is None and seen["none_yet"] == () and seen["last"] is c
    assert isinstance(seen["three"], tuple) and len(seen["three"]) == 3
    assert all(got is want for got, want in zip(seen["three"], (a, b, c)))
    assert torch.equal(x.grad, torch.full((3,), 2.0))


# ------------------------------------------------------------------------------------------ the route and the tier table
def _parent_rule(backend, exact, is_map, fused_ok, fusedg_ok):
    """The routing rule as the commit before the table spelled it (in _forward_sweep and again in TangentISTA.forward)."""
    auto = backend == "auto" and not exact
    auto = auto and not is_map
    fused = auto and fused_ok
    fusedg = auto and not fused and fusedg_ok
    return "fusedg" if fusedg else "fused" if fused else "generic"


@pytest.fixture
def sweep_spies(monkeypatch):
    """The sweeps of the three tiers replaced by recorders, and the one launch before them (the thresholds) by a stub:
    calls[i] = (name of the loop-level function reached, its arguments, its keywords)."""
    calls = []

    def spy(name, result):
        def run(*args, **kw):
            calls.append((name, args, kw))
            return result
        return run

    z = _code()
    monkeypatch.setattr(ops, "thresholds", lambda t, c, n: torch.zeros(K, n, M))
    for name in ("_forward_generic", "_forward_fused", "_forward_fusedg"):
        monkeypatch.setattr(loop, name, spy(name, (_thin(), z, [z], [], ["maps"])))
    for name in ("_tangent_generic", "_tangent_fused", "_tangent_fusedg"):
        monkeypatch.setattr(loop, name, spy(name, (_thin(), [z], [])))
    return calls


@pytest.mark.parametrize("fusedg_ok", [False, True])
@pytest.mark.parametrize("fused_ok", [False, True])
@pytest.mark.parametrize("is_map", [False, True])
@pytest.mark.parametrize("arithmetic", ["split3", "fp32"])
@pytest.mark.parametrize("backend", ["auto", "generic"])
def test_route_truth_table(monkeypatch, sweep_spies, backend, arithmetic, is_map, fused_ok, fusedg_ok):
    monkeypatch.setattr(ops, "fused_supported", lambda g: fused_ok)
    monkeypatch.setattr(ops, "fusedg_supported", lambda g: fusedg_ok)
    monkeypatch.setattr(ops, "fusedg_code_layout", lambda g, training=True: "rsc")
    monkeypatch.setattr(loop, "BACKEND", backend)
    want = _parent_rule(backend, arithmetic == "fp32", is_map, fused_ok, fusedg_ok)
    t = torch.rand(K, 2, M, 1, 1)
    c = torch.rand(N, 1, H, W) if is_map else torch.rand(N)
    w = [torch.zeros(G.filter_shape())] * K
    with loop.precision_scope(arithmetic):
        st = type("Ctx", (), {"exact": loop.PRECISION == "fp32"})()         # what _arithmetic_aware leaves on a context
        assert loop._route(G, st.exact, is_map) == want
        loop._forward_sweep(st, G, _thin(), None, c, t, w, w, False, False)
    assert (st.tier, st.fused, st.fusedg, st.is_map) == (want, want == "fused", want == "fusedg", is_map)
    (name, args, kw), = sweep_spies
    assert name == "_forward_" + want
    if is_map:                                           # the generic sweep gets the map and the slopes t[:, 1]
        assert kw["cmap"] is c and torch.equal(kw["tslope"], t[:, 1, :, 0, 0])
    else:
        assert "cmap" not in kw
        assert st.layout == {"fused": loop.CODE_LAYOUT, "fusedg": "rsc", "generic": None}[want]


def test_table_entries_follow_a_patched_sweep(monkeypatch):
    """The entries name loop._forward_generic & co. through the module when they are called: a test that swaps in the
    stepwise twin (tests/test_gpu_sigmamap.py) reaches every node that goes through the table."""
    seen = []
    monkeypatch.setattr(loop, "_forward_generic", lambda *a, **kw: seen.append(("fwd", a[0], kw)))
    monkeypatch.setattr(loop, "_backward_generic", lambda *a, **kw: seen.append(("bwd", a[0], kw)))
    st = type("Ctx", (), {})()
    tier = loop._TIERS["generic"]
    tier.forward(st, G, "yp", None, "tau", [], [], True, False, True, cmap="c", tslope="s")
    tier.reverse(st, G, K, "yp", None, None, [], [], [], [], "g_xp", None, "dt", [], "dyp", None, cmap="c", tslope="s", dcmap="d")
    assert seen == [("fwd", G, dict(cmap="c", tslope="s")),
                    ("bwd", G, dict(dyp="dyp", dtau=None, cmap="c", tslope="s", dcmap="d"))]


@pytest.mark.parametrize("tier", ["fused", "fusedg", "generic"])
def test_tangent_primal_goes_through_the_loop_level_forward(monkeypatch, sweep_spies, tier):
    """TangentISTA.forward obtains its primal through _forward_sweep and the table -- loop._forward_fused / _fusedg /
    _generic -- not from ops directly; and in the three ways it differs from UnrolledISTA's primal: the bit maps although
    nothing is kept, "nchw" codes on the fused generic tier, all K codes on the generic tier."""
    monkeypatch.setattr(ops, "fused_supported", lambda g: tier == "fused")
    monkeypatch.setattr(ops, "fusedg_supported", lambda g: tier == "fusedg")
    monkeypatch.setattr(ops, "fusedg_code_layout", lambda g, training=True: "rsc")
    monkeypatch.setattr(ops, "preprocess", lambda y, s, mask=None: (y, None, None, None))
    monkeypatch.setattr(ops, "postprocess", lambda xp, mean, pads: xp)
    w = [torch.zeros(G.filter_shape())] * K
    with torch.no_grad():
        out = loop.run_tangent(_thin(), _thin(), None, torch.rand(N), torch.rand(K, 2, M, 1, 1), w, w, 1, codes=True)
    assert len(out) == 4
    (fname, fargs, fkw), (tname, targs, tkw) = sweep_spies
    assert (fname, tname) == ("_forward_" + tier, "_tangent_" + tier)
    keep_codes, keep_resid = fargs[6], fargs[7]
    if tier == "generic":
        assert (keep_codes, keep_resid) == (True, False) and fkw == {}
        assert len(targs[5]) == 1 and torch.is_tensor(targs[5][0])      # gated by the primal's codes
    else:
        assert (keep_codes, keep_resid) == (False, False) and fkw == {"keep_maps": True}
        assert fargs[8] == (loop.CODE_LAYOUT if tier == "fused" else "nchw")
        assert targs[5] == ["maps"]                      # gated by the primal's bit maps
    assert tkw == {"last": True}


def test_code_layout_setter_takes_the_fused_2d_layouts_only():
    before = loop.CODE_LAYOUT
    try:
        for name in ("nchw", "blocked", "blocked_bf16"):
            loop.set_code_layout(name)
            assert loop.CODE_LAYOUT == name
        with pytest.raises(ValueError):
            loop.set_code_layout("rsc")                  # the strip kernels' own layout: the fused 2-D sweeps cannot store it
        assert loop.CODE_LAYOUT == "blocked_bf16"
        assert "rsc" in ops.LAYOUT                       # one code table
    finally:
        loop.set_code_layout(before)
    assert cva.loop is loop
