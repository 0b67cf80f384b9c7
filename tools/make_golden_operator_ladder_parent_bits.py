#!/usr/bin/env python3
"""Route and bits of the generic operators recorded on the commit BEFORE their tier ladder moved into cdl_operators.hip and the
dense tier's host side was folded:

    CDLNET_HIP_LIB=<that commit's libcdlnet_hip.so> CDLNET_HIP_CSRC=<that commit's cdlnet-video_amd/csrc> \
        python tools/make_golden_operator_ladder_parent_bits.py tests/golden/operator_ladder_parent_bits.npz

tests/test_gpu_operator_ladder_parent_bits.py calls `compute_case()` on the current commit and compares byte for byte.

Cases (keys, seeded data and switch settings are those of tests/test_gpu_dispatch.py, imported):
  ana|syn|wg/<tier>/<key>   every (tier, key) at which test_gpu_dispatch.py pins a launch site, through the calls it makes there:
                            ana: plain, first, iter, gated, rev (du and dt);  syn: plain, resid, gated;  wg: plain, gated, pair
  prox1|prox2/mfma/<key>    the CSR epilogue of the matrix-core analysis (z and u_out)
  ana/denseoff/<key>        the matrix-core settings with CDL_MFMA_DENSE=0
  ana|syn/mfma/<key>        the dense tier, which has no cell test: N = 1, C = 24, M = 40 at 17 x 33 with P = 3 and P = 5 (a partial
                            16-channel chunk, a padded channel-tile pair, partial tiles on both axes, the fragment copy's tail loop)
                            and at 2 x 17 x 33 with 3 x 3 x 3 (the skipped zero-padding planes)
  wg/mfma/<key>             cdl_dense_wgrad: C = M = 24 (the narrow wave layout) and C = 40, M = 72 (two output groups) at
                            2 x 9 x 33 (scalar loads) and 2 x 9 x 36 (16-byte loads): 12 tiles, above the plan's minimum of 8
  residual/<shape>          ResidualBlock forward and backward at the smallest shape of tests/test_gpu_residual.py
  perceptual/<shape>        the perceptual loss forward and backward at the smallest shape of tests/test_gpu_perceptual.py: every
                            form of cdl_dense_vgg
Each call records <case>/<call>/<output> -- code- and image-sized tensors as the (sum, xor) folds of the mfma_tier_parent_bits
tool, filter and threshold gradients in full -- and <case>/<call>/sites, the sorted launch sites of its ops.trace() as JSON in
uint8.  The record is the named file and <stem>.1.npz, ... (whole calls, each file below 1 MiB).
"""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_dispatch as D  # noqa: E402  (keys, data() and ENV)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_bits = _load("make_golden_mfma_tier_parent_bits")       # _fold, save_parts, load_parts
_fold, load_parts = _bits._fold, _bits.load_parts
_sizes = _load("make_golden_operator_ladder_parent_sizes")   # _keys, _marks: the keys inside test_gpu_dispatch.py's marks

SETTINGS = dict(D.ENV, denseoff={**D.ENV["mfma"], "CDL_MFMA_DENSE": "0"})
# test of test_gpu_dispatch.py -> (kind, the tier it forces; None: the tier is a parameter of the test)
TESTS = {"test_analysis_matrix_core_variants": ("ana", "mfma"), "test_analysis_tiled_tier": ("ana", "tiled"),
         "test_analysis_plain_kernels": ("ana", "plain"), "test_dense_tier_analysis": ("ana", "mfma"),
         "test_synthesis_matrix_core_variants": ("syn", None), "test_synthesis_tiled_tier": ("syn", None),
         "test_synthesis_plain_kernels": ("syn", "plain"), "test_dense_tier_synthesis": ("syn", "mfma"),
         "test_wgrad_matrix_core_variants": ("wg", "mfma"), "test_wgrad_tiled_tier": ("wg", None),
         "test_wgrad_plain_kernels": ("wg", "plain"), "test_dense_tier_wgrad": ("wg", "mfma")}
BELOW_ANA, BELOW_WG = (3, 1, 16, (6, 30, 61), (3, 5, 5), 1), (15, 1, 8, (60, 121), (5, 5), 1)   # written inside two test bodies
DENSE_CONV = [(1, 24, 40, (17, 33), (3, 3), 1), (1, 24, 40, (17, 33), (5, 5), 1), (1, 24, 40, (2, 17, 33), (3, 3, 3), 1)]
DENSE_WGRAD = [(1, C, M, (2, 9, W), (3, 3, 3), 1) for C, M in ((24, 24), (40, 72)) for W in (33, 36)]
RESIDUAL, PERCEPTUAL = (1, 16, (4, 8, 8)), (1, 1, 3, 37, 50)


def key_id(key):
    N, C, M, sp, P, s = key
    return f"N{N}C{C}M{M}_{'x'.join(map(str, sp))}_P{'x'.join(map(str, P))}_s{s}"


def _cases():
    """[(case id, kind, tier, key)] in a fixed order, each once."""
    out = []

    def add(kind, tier, key):
        cid = f"{kind}/{tier}/{key_id(key)}"
        if cid not in [c[0] for c in out]:
            out.append((cid, kind, tier, key))

    for name, (kind, tier) in TESTS.items():
        for args in _sizes._marks(getattr(D, name)):
            for row in args[1]:
                add(kind, tier or row[0], _sizes._keys([row], [])[0])
    add("ana", "mfma", BELOW_ANA)
    add("wg", "mfma", BELOW_WG)
    for args in _sizes._marks(D.test_analysis_matrix_core_prox_epilogue):
        if args[0] == "key":
            for key in args[1]:
                add("prox1", "mfma", key)
                add("prox2", "mfma", key)
    add("ana", "denseoff", D.DENSE[1][0])
    for key in DENSE_CONV:
        add("ana", "mfma", key)
        add("syn", "mfma", key)
    for key in DENSE_WGRAD:
        add("wg", "mfma", key)
    return out


_TABLE = _cases()
CASES = [c[0] for c in _TABLE] + ["residual/" + "x".join(map(str, RESIDUAL[2])), "perceptual/" + "x".join(map(str, PERCEPTUAL[2:]))]
# kind -> {call: the arrays it records}; every array is <case>/<call>/<name>, next to <case>/<call>/sites
CALLS = {"ana": {"plain": ["out"], "first": ["out"], "iter": ["out"], "gated": ["out"], "rev": ["du", "dt"]},
         "syn": {"plain": ["out"], "resid": ["out"], "gated": ["out"]},
         "wg": {"plain": ["dw"], "gated": ["dw"], "pair": ["dw0", "dw1"]},
         "prox1": {"prox": ["z", "u"]}, "prox2": {"prox": ["z", "u"]},
         "residual": {"fwd": ["h", "out"], "bwd": ["dx", "dw1", "dw2"]}, "perceptual": {"fwd": ["value"], "bwd": ["dx", "dy"]}}


def array_names(case):
    calls = CALLS[case.split("/")[0]]
    return [f"{case}/{c}/{n}" for c, names in calls.items() for n in names + ["sites"]]


_SITE_INDEX = []


def _sites(trace):
    """The sorted launch sites of a trace as JSON bytes.  A trace record names a source line, so the sites are looked up in
    the sources the library was built from: CDLNET_HIP_CSRC (recording on another commit's library), else this tree's."""
    import numpy as np
    if not _SITE_INDEX:
        lc = _load("launch_coverage")
        _SITE_INDEX.extend([lc, lc.index(lc.scan_sources(os.environ.get("CDLNET_HIP_CSRC") or lc.CSRC))])
    lc, by_check = _SITE_INDEX
    sites = set()
    for r in trace:
        sid = lc.site_of(by_check, (r.file, r.line, r.func, r.note))
        assert sid is not None, f"trace record that names no single launch site: {r}"
        sites.add(sid)
    return np.frombuffer(json.dumps(sorted(sites)).encode(), dtype=np.uint8).copy()


def sites_of(arr):
    return json.loads(bytes(arr).decode())


class _Rec:
    def __init__(self, o, out, case):
        self.o, self.out, self.case = o, out, case

    def call(self, name, fn):
        """Run fn() under the launch trace and keep its sites as <case>/<name>/sites."""
        with self.o.trace() as t:
            got = fn()
        self.out[f"{self.case}/{name}/sites"] = _sites(t)
        return got

    def put(self, call, name, value, full=False):
        self.out[f"{self.case}/{call}/{name}"] = value.detach().cpu().numpy() if full else _fold(value)


def _analysis(r, g, d, M):
    import torch
    o = r.o
    xd, wd, zd, ud, td = (d[k].cuda() for k in ("x", "w", "z", "u", "tau"))
    r.put("plain", "out", r.call("plain", lambda: o.analysis(g, xd, wd)))
    r.put("first", "out", r.call("first", lambda: o.analysis(g, xd, wd, 1.0, None, None, td)))
    r.put("iter", "out", r.call("iter", lambda: o.analysis(g, xd, wd, -1.0, zd, None, td)))
    r.put("gated", "out", r.call("gated", lambda: o.analysis(g, xd, wd, 1.0, ud, zd, None)))
    dt = torch.zeros(2, M, device="cuda")
    r.put("rev", "du", r.call("rev", lambda: o.analysis_rev(g, xd, wd, 0.5, ud, zd, d["c"].cuda(), dt)))
    r.put("rev", "dt", dt, full=True)


def _synthesis(r, g, d):
    o = r.o
    zd, wd, ud, md, xd = (d[k].cuda() for k in ("z", "w", "u", "mask", "x"))
    r.put("plain", "out", r.call("plain", lambda: o.synthesis(g, zd, wd)))
    r.put("resid", "out", r.call("resid", lambda: o.synthesis(g, zd, wd, 1.0, None, md, xd)))
    r.put("gated", "out", r.call("gated", lambda: o.synthesis(g, ud, wd, -1.0, zd, md, None)))


def _wgrad(r, g, d):
    o = r.o
    xd, zd, ud = (d[k].cuda() for k in ("x", "z", "u"))
    r.put("plain", "dw", r.call("plain", lambda: o.wgrad(g, zd, xd, -2.0)), full=True)
    r.put("gated", "dw", r.call("gated", lambda: o.wgrad(g, ud, xd, 1.0, gate=zd)), full=True)
    ug = (d["u"] * (d["z"] != 0)).cuda()
    d0, d1 = r.call("pair", lambda: o.wgrad_pair(g, ug, xd, 1.0, zd, xd, -2.0))
    r.put("pair", "dw0", d0, full=True)
    r.put("pair", "dw1", d1, full=True)


def _prox(r, g, d, key, both):
    """The calls of test_analysis_matrix_core_prox_epilogue."""
    import torch
    N, M = key[0], key[2]
    gen = torch.Generator().manual_seed(21)
    code = lambda: 0.3 * torch.randn(d["z"].shape, generator=gen) * (torch.rand(d["z"].shape, generator=gen) > 0.5)
    zp, za = code(), code()
    lam, g1, g2 = (torch.rand(N, M, generator=gen) * sc + 0.01 for sc in (0.2, 1.2, 1.2))
    u_out = torch.empty(d["z"].shape, device="cuda")
    z = r.call("prox", lambda: r.o.analysis_prox(g, d["x"].cuda(), d["w"].cuda(), -1.0, d["z"].cuda(), zp.cuda(), lam.cuda(),
                                                g1.cuda(), za.cuda() if both else None, g2.cuda() if both else None, u_out=u_out))
    r.put("prox", "z", z)
    r.put("prox", "u", u_out)


def _residual(r):
    """The data and calls of tests/test_gpu_residual.py's test_block_vs_oracle_dense_shapes."""
    import torch
    N, M, shape = RESIDUAL
    gen = torch.Generator().manual_seed(100 + M)
    x = torch.randn((N, M) + shape, generator=gen) * 0.5
    w1 = torch.randn((M, M, 3, 3, 3), generator=gen) / (27 * M) ** 0.5
    w2 = torch.randn((M, M, 3, 3, 3), generator=gen) / (27 * M) ** 0.5
    wgt = torch.randn((N, M) + shape, generator=gen)
    g = r.o.residual_geometry(x, w1)
    xd, w1d, w2d = x.cuda(), w1.cuda(), w2.cuda()
    h, out = r.call("fwd", lambda: r.o.residual_forward(g, xd, w1d, w2d))
    dx, dw1, dw2 = r.call("bwd", lambda: r.o.residual_backward(g, xd, h, out, w1d, w2d, wgt.cuda()))
    r.put("fwd", "h", h)
    r.put("fwd", "out", out)
    r.put("bwd", "dx", dx)
    r.put("bwd", "dw1", dw1, full=True)
    r.put("bwd", "dw2", dw2, full=True)


def _perceptual(r, cva):
    """The data and calls of tests/test_gpu_perceptual.py's test_value_and_gradients."""
    import perceptual_restate as R
    import torch
    from test_gpu_perceptual import _clips
    sd = R.random_weights(PERCEPTUAL[-2])
    o_, t_ = _clips(PERCEPTUAL, seed=sum(PERCEPTUAL) + 7)
    oc, tc = o_.cuda().requires_grad_(), t_.cuda().requires_grad_()
    val = r.call("fwd", lambda: cva.metrics.perceptual_frames(oc, tc, sd))
    r.call("bwd", lambda: val.backward(torch.tensor(0.7, device="cuda")))
    r.put("fwd", "value", val.reshape(1), full=True)
    r.put("bwd", "dx", oc.grad)
    r.put("bwd", "dy", tc.grad)


def compute_case(case, setenv):
    """{name: numpy array} of one case.  `setenv(name, value)` sets a CDL_* switch and reloads the library's options (the
    hip_env fixture of tests/conftest.py; `_setenv` of the mfma_tier_parent_bits tool)."""
    import torch
    import cdlnet_video_amd as cva
    out = {}
    r = _Rec(cva.ops, out, case)
    if case.startswith("residual/"):
        _residual(r)
    elif case.startswith("perceptual/"):
        _perceptual(r, cva)
    else:
        _, kind, tier, key = _TABLE[CASES.index(case)]
        for k, v in SETTINGS[tier].items():
            setenv(k, v)
        N, C, M, sp, P, s = key
        d = D.data(*key)
        g = cva.ops.Geometry.make(N, C, M, sp, P, d["pad"], s)
        if kind == "ana":
            _analysis(r, g, d, M)
        elif kind == "syn":
            _synthesis(r, g, d)
        elif kind == "wg":
            _wgrad(r, g, d)
        else:
            _prox(r, g, d, key, kind == "prox2")
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    import cdlnet_video_amd as cva
    rec = {}
    for case_ in CASES:
        for names_ in SETTINGS.values():
            for name_ in names_:
                os.environ.pop(name_, None)
        cva._lib.reload_options()
        rec.update(compute_case(case_, _bits._setenv))
        print("recorded", case_, flush=True)
    groups_ = [f"{case_}/{call_}" for case_ in CASES for call_ in CALLS[case_.split("/")[0]]]   # whole calls per file
    for path_, part_ in _bits.save_parts(sys.argv[1], rec, groups_).items():
        print("wrote", path_, len(part_), "arrays")
