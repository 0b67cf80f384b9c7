#!/usr/bin/env python3
"""Generate tests/golden/operator_ladder_parent_sizes.json: what the four *_workspace_floats of the generic operators,
cdl_ista_scratch_floats and cdl_residual_scratch_floats answered on the commit BEFORE the operators' tier ladder moved into
cdl_operators.hip -- under every switch setting of tests/test_gpu_dispatch.py's ENV, each also with
cdl_set_exact_fp32(1).  tests/test_operator_ladder_cpu.py holds the library to these answers.

    CDLNET_HIP_LIB=/path/to/parent/libcdlnet_hip.so PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_operator_ladder_parent_sizes.py

No GPU is needed: without a device the library plans for 256 compute units, the MI355X's count.
"""
import ctypes
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
OUT = os.path.join(ROOT, "tests", "golden", "operator_ladder_parent_sizes.json")

FUNCS = ["cdl_analysis_workspace_floats", "cdl_analysis_rev_workspace_floats", "cdl_synthesis_workspace_floats",
         "cdl_wgrad_workspace_floats", "cdl_ista_scratch_floats", "cdl_residual_scratch_floats"]
VGG_LAYERS = [(64, 64, 0), (64, 128, 1), (128, 128, 1), (128, 256, 2), (256, 256, 2), (256, 256, 2)]   # (C, M, level), cdl_vgg.hip


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


geom = _load("make_golden_fusedg_plans").geom      # (N, C, M, spatial, P, s) -> the 15 integers of cdl_geom


def _keys(obj, out):
    """The geometry keys (N, C, M, spatial, P, stride) anywhere inside a parametrize argument or a table."""
    if isinstance(obj, tuple) and len(obj) == 6 and isinstance(obj[3], tuple) and isinstance(obj[4], tuple) \
            and all(isinstance(v, int) for v in obj[:3] + (obj[5],)):
        if obj not in out:
            out.append(obj)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            _keys(v, out)
    return out


def _marks(fn):
    return [m.args for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]


def geometries():
    import test_gpu_dispatch as D
    import test_gpu_perceptual as V
    import test_gpu_residual as R
    keys = _keys([D.MFMA_ANALYSIS, D.DENSE], [])
    for name in sorted(vars(D)):                            # the tables written into the parametrize marks
        if name.startswith("test_"):
            _keys(_marks(getattr(D, name)), keys)
    # the two keys test_gpu_dispatch.py writes inside a test body: one below each matrix-core plan's minimum
    keys += [k for k in [(3, 1, 16, (6, 30, 61), (3, 5, 5), 1), (15, 1, 8, (60, 121), (5, 5), 1)] if k not in keys]
    gs = [geom(N, C, M, sp, P, s) for N, C, M, sp, P, s in keys]
    for args in _marks(R.test_block_vs_oracle_dense_shapes):                        # ResidualBlock: C = M, 3 x 3 x 3
        gs += [geom(N, M, M, sp, 3) for N, M, sp in args[1]]
    for N, _, D_, H, W in V.SHAPES:                                                 # the VGG16 layers, one plane per frame
        gs += [geom(N * D_, C, M, (H >> lev, W >> lev), 3) for C, M, lev in VGG_LAYERS] + [geom(N * D_, 1, 64, (H, W), 3)]
    # the edges of the rules that now stand in one place
    gs += [geom(N, 1, 8, (32, 64), 5) for N in (4096, 4097)]                        # k_wgrad_l: 4096 and 4097 tiles of 64 x 32
    gs += [geom(2, 1, M, (40, 72), 5) for M in (1024, 1025, 2048, 2049)]            # k_wgrad_p: M*C*Pd around 2048 / chunks
    gs += [geom(2, 2, 512, (4, 40, 72), (2, 5, 5), pad=(1, 2, 2)), geom(2, 3, 683, (40, 72), 5)]    # ... as a product: 2048, 2049
    gs += [geom(1, 1, 8, (8, 64), 5), geom(1, 1, 8, (2, 64), 5)]                    # more chunks than row groups
    gs += [geom(1, C, M, (2, 9, 36), 3) for C, M in ((15, 16), (16, 15), (16, 16), (15, 15))]       # dense: 16 channels a side
    gs += [geom(1, 16, 16, (16, 36), P) for P in (5, 7)] + [geom(1, 16, 16, (16, 36), (7, 5))]      # dense: planes up to 5 x 5
    gs += [geom(1, 16, 16, (16, 36), 3, 2), geom(1, 16, 16, (2, 16, 36), 3, (2, 1, 1))]             # dense: unit stride only
    gs += [geom(1, 16, 16, (H, 32), 3) for H in (16, 28, 29, 32)]                   # dense wgrad: 4, 7, 8, 8 tiles of 4 x 32
    gs += [geom(1, 65, 16, (32, 32), 3), geom(1, 64, 16, (32, 32), 3)]              # dense wgrad: at most 64 image channels
    return gs


def record(setting, setenv):
    """{"exact0": [[the FUNCS per geometry]], "exact1": ...} under ENV[setting] of tests/test_gpu_dispatch.py, set through
    setenv(name, value) on an environment that holds none of the switches."""
    import cdlnet_video_amd as cva
    from test_gpu_dispatch import ENV
    for k, v in ENV[setting].items():
        setenv(k, v)
    lib, out = cva._lib.lib(), {}
    for exact in (0, 1):
        prev = lib.cdl_set_exact_fp32(exact)
        try:
            out[f"exact{exact}"] = [[int(getattr(lib, f)(ctypes.byref(cva._lib.Geom(*g)))) for f in FUNCS] for g in geometries()]
        finally:
            lib.cdl_set_exact_fp32(prev)
    return out


def main():
    import cdlnet_video_amd as cva
    from test_gpu_dispatch import ENV

    def setenv(name, value):
        os.environ[name] = value
        cva._lib.reload_options()

    rec = {"funcs": FUNCS, "geoms": geometries(), "sizes": {}}
    for setting in ENV:
        for names in ENV.values():
            for name in names:
                os.environ.pop(name, None)
        cva._lib.reload_options()
        rec["sizes"][setting] = record(setting, setenv)
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(rec['geoms'])} geometries x {len(ENV)} settings x 2 from {cva._lib.LIB_PATH}")


if __name__ == "__main__":
    main()
