#!/usr/bin/env python3
"""Bits of the sparse matrix-core tier (cdl_analysis_mfma.hip, cdl_synth_mfma.hip, cdl_wgrad_mfma.hip) recorded on the commit
BEFORE its three files came to share one plane gate, one plane dispatch and the device pieces of cdl_wave_dev.h (DESIGN.md
section 36):

    CDLNET_HIP_LIB=<that commit's libcdlnet_hip.so> python tools/make_golden_mfma_tier_parent_bits.py tests/golden/mfma_tier_parent_bits.npz

tests/test_gpu_mfma_tier_parent_bits.py calls `compute_case()` on the current commit and compares bit for bit.

The cells, their shapes and their seeded data are those of tests/test_gpu_generic_cells.py (imported, not restated), under
its forced-tier environment.  Cases:
  ana/<cell>   plain, first, iter, gated, map, rev and revmap (du; dt0, dt1), prox, prox2, proxmap, prox2map (z and u_out);
               the sign-mixed cells run first, iter and map, as they do there
  syn/<cell>   the cell's gate / mask / sub choice at 11 x 36 through the vector and the scalar assemble, at 11 x 37 (scalar)
  wgm/<cell>   single, gated and pair at 40 x 72 and at 40 x 70 ("W70")
  strip/<lay>  a K = 2 forward and reverse sweep of the fused generic tier at M = 100, P = 7, stride 1, 1 x 33 x 70 -- the
               smallest shape of tests/test_gpu_strip.py whose training layout is "rsc" -- with the codes in "rsc" and forced
               to "nchw": k_wgm behind the folded entry point, reading either layout, paired (k = 1) and single (k = 0)
Image- and code-sized tensors are recorded as two 64-bit folds of their int32 bit patterns, sum and xor; filter gradients
and threshold sums in full.  The record is written as the named file and <stem>.1.npz, <stem>.2.npz, ... (whole cases, each
file below 1 MiB).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_generic_cells as T  # noqa: E402  (the cell tables, cell_data and the forced-tier ENV)

STRIP = dict(K=2, M=100, P=7, s=1, shape=(1, 1, 33, 70))
ANA_CASES = [f"ana/{c.id}" for c in T.ANA_CELLS + T.SIGN_MIXED]
SYN_CASES = [f"syn/{c.id}" for c in T.SYN_CELLS]
WGM_CASES = [f"wgm/{c.id}" for c in T.WGM_CELLS]
STRIP_CASES = ["strip/rsc", "strip/nchw"]
CASES = ANA_CASES + SYN_CASES + WGM_CASES + STRIP_CASES
NAN = float("nan")


def _fold(t):
    """(sum, xor) of the int32 bit patterns of a float32 tensor, as int64."""
    import numpy as np
    bits = t.detach().contiguous().cpu().numpy().view(np.int32).astype(np.int64).ravel()
    return np.array([bits.sum(), np.bitwise_xor.reduce(bits)], dtype=np.int64)


def ana_names(c):
    """The arrays of an analysis case."""
    names = ["first", "iter", "map"]
    if not c.opt.get("mixed"):
        names += ["plain", "gated", "rev/du", "rev/dt", "revmap/du", "revmap/dt"]
        names += [f"{p}/{q}" for p in ("prox", "prox2", "proxmap", "prox2map") for q in ("z", "u")]
    return names


SYN_NAMES = ["vector", "scalar", "scalarW37"]
WGM_NAMES = [f"{n}{tag}" for tag in ("", "W70") for n in ("single", "gated", "pair0", "pair1")]
STRIP_NAMES = ["xp", "z", "dA", "dB", "dt"]


def _analysis(o, c, out, case):
    import torch
    g, dc = T._geom(o, c), T.cell_data(c.id)
    dv = {k: v.cuda() for k, v in dc.items()}
    new = lambda: torch.full(g.code_shape(), NAN, device="cuda")
    pick = lambda k: None if k is None else dv[k]

    def fwd(name, alpha, zin, gate, tau, cmap=None, tslope=None):
        out[f"{case}/{name}"] = _fold(o.analysis(g, dv["x"], dv["w"], alpha, pick(zin), pick(gate), pick(tau), new(),
                                                 cmap=pick(cmap), tslope=pick(tslope)))

    fwd("first", 1.0, None, None, "tau")
    fwd("iter", -1.0, "z", None, "tau")
    fwd("map", -1.0, "z", None, "tau", "cmap", "tslope")
    if c.opt.get("mixed"):
        return
    fwd("plain", 1.0, None, None, None)
    fwd("gated", 1.0, "u", "z", None)
    for name, cmap in (("rev", None), ("revmap", "cmap")):
        dt = torch.full((2, c.M), NAN, device="cuda")
        du = o.analysis_rev(g, dv["x"], dv["w"], 0.5, dv["u"], dv["z"], None if cmap else dv["c"], dt, new(), cmap=pick(cmap))
        out[f"{case}/{name}/du"], out[f"{case}/{name}/dt"] = _fold(du), dt.cpu().numpy()
    for name, both, cmap in (("prox", False, None), ("prox2", True, None), ("proxmap", False, "cmap"), ("prox2map", True, "cmap")):
        uo = new()
        z = o.analysis_prox(g, dv["x"], dv["w"], -1.0, dv["z"], dv["zp"], dv["lam"], dv["g1"], dv["za"] if both else None,
                            dv["g2"] if both else None, uo, new(), cmap=pick(cmap), tslope=dv["tslope3"] if cmap else None)
        out[f"{case}/{name}/z"], out[f"{case}/{name}/u"] = _fold(z), _fold(uo)


def _synthesis(o, c0, out, case, setenv):
    import torch
    gated, masked = c0.opt["gated"], c0.opt["masked"]
    for aligned in (True, False):
        c = T._sized(c0, "syn", aligned)
        g, dc = T._geom(o, c), T.cell_data(c0.id, "syn", aligned)
        dv = {k: dc[k].cuda() for k in ("z", "w", "gate", "mask", "sub")}
        for forced in ((False, True) if aligned else (False,)):
            setenv("CDL_SCALAR_ASSEMBLE", "1" if forced else "0")
            name = ("vector" if aligned and not forced else "scalar") + ("" if aligned else "W37")
            img = o.synthesis(g, dv["z"], dv["w"], 1.0 if masked else -1.0, dv["gate"] if gated else None,
                              dv["mask"] if masked else None, dv["sub"] if masked else None,
                              torch.full(g.image_shape(), NAN, device="cuda"))
            out[f"{case}/{name}"] = _fold(img)
        setenv("CDL_SCALAR_ASSEMBLE", "0")


def _filter_gradients(o, c0, out, case):
    for aligned in (True, False):
        c = T._sized(c0, "wgm", aligned)
        g, dc = T._geom(o, c), T.cell_data(c0.id, "wgm", aligned)
        dv = {k: dc[k].cuda() for k in ("z", "u", "gate", "x", "x2")}
        tag = "" if aligned else "W70"
        o._wgrad_workspace(g, dv["x"].device)[0].fill_(NAN)
        out[f"{case}/single{tag}"] = o.wgrad(g, dv["z"], dv["x"], -1.0).cpu().numpy()
        out[f"{case}/gated{tag}"] = o.wgrad(g, dv["u"], dv["x"], 0.5, dv["gate"]).cpu().numpy()
        d0, d1 = o.wgrad_pair(g, dv["z"], dv["x"], -1.0, dv["u"], dv["x2"], 1.0)
        out[f"{case}/pair0{tag}"], out[f"{case}/pair1{tag}"] = d0.cpu().numpy(), d1.cpu().numpy()


def _strip(cva, lay, out, case):
    """The sweep pair of tests/test_gpu_strip.py's test_strip_sweeps_equal_generic_on_same_activations at K = 2."""
    import torch
    o, loop = cva.ops, cva.loop
    K, M, P, s, shape = (STRIP[k] for k in ("K", "M", "P", "s", "shape"))
    torch.manual_seed(21)
    net = cva.CDLNet(K=K, M=M, P=P, s=s, C=1, t0=5e-3, adaptive=True, init=True)
    with torch.no_grad():
        for n_, p_ in net.named_parameters():
            if n_ == "t":
                p_.uniform_(2e-3, 2e-2)
            elif n_ != "g":
                p_.add_(0.05 * p_.abs().mean() * torch.randn_like(p_))
    net = net.cuda()
    x = cva.utils.synthetic_clip(shape, seed=5)
    y, sig = cva.awgn(x, (20, 30), torch.Generator().manual_seed(6))
    yp, _, _, _ = o.preprocess(y.cuda(), s, None)
    g = o.Geometry.make(shape[0], 1, M, yp.shape[2:], (P, P), (P // 2, P // 2), s)
    assert o.fusedg_supported(g) and not o.fused_supported(g) and o.fusedg_code_layout(g, training=True) == "rsc"
    c = (sig.reshape(-1) / 255.0).cuda()
    tau = o.thresholds(net.t.detach(), c, shape[0])
    A = [m.weight.detach() for m in net.A]
    B = [m.weight.detach() for m in net.B]
    xp, z, codes, resid, maps = loop._forward_fusedg(g, yp, None, tau, A, B, True, True, lay)
    g_xp = torch.randn(xp.shape, generator=torch.Generator().manual_seed(8)).cuda()
    g_z = torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).cuda() * 0.01
    dt = torch.zeros(K, 2, M, device="cuda")
    dA, dB = loop._backward_fusedg(g, K, yp, None, c, A, B, codes, resid, g_xp, g_z, dt, maps=maps, layout=lay)
    torch.cuda.synchronize()
    out[case + "/xp"], out[case + "/z"] = _fold(xp), _fold(z)
    out[case + "/dA"], out[case + "/dB"] = torch.stack(list(dA)).cpu().numpy(), torch.stack(list(dB)).cpu().numpy()
    out[case + "/dt"] = dt.cpu().numpy()


def compute_case(case, setenv):
    """{name: numpy array} of one case.  `setenv(name, value)` sets a CDL_* switch and reloads the library's options
    (the hip_env fixture of tests/conftest.py; `_setenv` below)."""
    import torch
    import cdlnet_video_amd as cva
    for k, v in T.ENV.items():
        setenv(k, v)
    kind, cid = case.split("/", 1)
    out = {}
    if kind == "ana":
        _analysis(cva.ops, T.BY_ID[cid], out, case)
    elif kind == "syn":
        _synthesis(cva.ops, T.BY_ID[cid], out, case, setenv)
    elif kind == "wgm":
        _filter_gradients(cva.ops, T.BY_ID[cid], out, case)
    else:
        _strip(cva, cid, out, case)
    torch.cuda.synchronize()
    return out


PART_BYTES = 900 << 10     # of array data per file: the filter gradients are kept in full, and a committed file stays below 1 MiB


def part_paths(path):
    """The files of the record written as `path`: path itself, then <stem>.1.npz, <stem>.2.npz, ... while they exist."""
    stem = path[:-len(".npz")]
    paths, i = [path], 1
    while os.path.exists(f"{stem}.{i}.npz"):
        paths.append(f"{stem}.{i}.npz")
        i += 1
    return paths


def save_parts(path, rec, cases=None):
    """Write {name: array} as path, <stem>.1.npz, ...: whole cases in the order of `cases` (CASES), a new file whenever the
    next case would take the current one past PART_BYTES.  Returns {file: names}."""
    import numpy as np
    assert path.endswith(".npz")
    parts, size = [[]], 0
    for case in (CASES if cases is None else cases):
        names = [k for k in rec if k.startswith(case + "/")]
        nbytes = sum(rec[k].nbytes for k in names)
        if parts[-1] and size + nbytes > PART_BYTES:
            parts.append([])
            size = 0
        parts[-1] += names
        size += nbytes
    assert sorted(k for part in parts for k in part) == sorted(rec)
    stem, out = path[:-len(".npz")], {}
    for i, names in enumerate(parts):
        out[path if i == 0 else f"{stem}.{i}.npz"] = names
        np.savez_compressed(path if i == 0 else f"{stem}.{i}.npz", **{k: rec[k] for k in names})
    return out


def load_parts(path):
    """{name: array} of the record written by save_parts."""
    import numpy as np
    rec = {}
    for part in part_paths(path):
        with np.load(part) as data:
            assert not set(data.files) & set(rec), part
            rec.update({k: data[k] for k in data.files})
    return rec


def _setenv(name, value):
    import cdlnet_video_amd as cva
    os.environ[name] = value
    cva._lib.reload_options()


if __name__ == "__main__":
    import cdlnet_video_amd as cva
    rec = {}
    for case_ in CASES:
        for name_ in list(T.ENV) + ["CDL_SCALAR_ASSEMBLE"]:
            os.environ.pop(name_, None)
        cva._lib.reload_options()
        rec.update(compute_case(case_, _setenv))
        print("recorded", case_, flush=True)
    for path_, part_ in save_parts(sys.argv[1], rec).items():
        print("wrote", path_, len(part_), "arrays")
