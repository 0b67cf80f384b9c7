#!/usr/bin/env python3
"""Generate tests/golden/fusedg_plans.json: what the host-only size queries of the fused generic tier (cdl_fusedg_*,
include/cdlnet_hip.h) answer for a list of geometries -- the shapes of tests/test_gpu_fusedg.py and
tests/test_gpu_strip.py, the benchmark's configurations and the edges of every admission rule -- with
CDL_FUSEDG_STRIP=0 and =1.  tests/test_fusedg_plan_cpu.py holds the library to these answers, so the fixture is
recorded from the library BEFORE a change to the plans, e.g. a build of the parent commit:

    CDLNET_HIP_LIB=/path/to/parent/libcdlnet_hip.so PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_fusedg_plans.py

No GPU is needed.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "fusedg_plans.json")

LAY_NCHW, LAY_RSC = 0, 3


def geom(N, C, M, sp, P, s=1, pad=None):
    """The 15 integers of cdl_geom: N, C, M, D, H, W, Pd, Ph, Pw, pd, ph, pw, sd, sh, sw (2-D: leading axis 1)."""
    nd = len(sp)
    P = [P] * nd if isinstance(P, int) else list(P)
    s = [s] * nd if isinstance(s, int) else list(s)
    pad = [p // 2 for p in P] if pad is None else list(pad)
    three = lambda v, fill: [fill] * (3 - nd) + [int(x) for x in v]
    return [N, C, M] + three(sp, 1) + three(P, 1) + three(pad, 0) + three(s, 1)


def geometries():
    from test_gpu_fusedg import SHAPES as TILE_SHAPES
    from test_gpu_strip import SHAPES as STRIP_SHAPES
    gs = [geom(N, C, M, sp, P) for N, C, M, sp, P, _ in TILE_SHAPES]
    gs += [geom(N, 1, M, sp, P, s) for N, M, P, s, sp, _ in STRIP_SHAPES]
    # the benchmark: the flagship step, its secondary s2030-architecture line, BASELINE configs[2] (video) and [3] (JDD)
    gs += [geom(64, 1, 64, (256, 256), 7), geom(64, 1, 169, (256, 256), 7, 2),
           geom(8, 1, 48, (8, 128, 128), 5), geom(8, 3, 64, (256, 256), 7)]
    for s in (1, 2):                                        # channel counts around every rule
        gs += [geom(1, 1, M, (40, 72), 5, s) for M in (7, 8, 12, 64, 72, 192, 200)]
    gs += [geom(1, 1, 16, (40, 72), P, s) for P in (3, 5, 7, 9) for s in (1, 2)]
    gs += [geom(1, 1, 16, (40, 72), (5, 7)), geom(1, 1, 16, (40, 72), (3, 5)), geom(1, 1, 16, (6, 40, 72), (3, 5, 7))]
    gs += [geom(1, C, 16, (40, 72), 5) for C in (2, 3, 5, 7, 9)]                       # G = C
    gs += [geom(1, 1, 16, (10, 40, 72), (Pd, 5, 5)) for Pd in (3, 5, 7, 9)]             # G = Pd
    gs += [geom(1, 3, 16, (4, 40, 72), (3, 5, 5))]                                      # G = 9 = 3 * 3
    gs += [geom(1, 7, 16, (40, 72), 7), geom(1, 1, 16, (8, 40, 72), 7), geom(1, 7, 16, (40, 72), 5)]   # P = 7 with G = 7
    gs += [geom(1, 3, 16, (40, 72), 5, 2), geom(1, 3, 64, (40, 72), 7, 2)]              # several channels, stride 2
    gs += [geom(1, 1, 16, (42, 72), P, 3) for P in (5, 7)]                              # stride 3
    gs += [geom(1, 1, 16, (4, 40, 72), 5, (1, 2, 2)), geom(1, 1, 16, (4, 40, 72), 5, (2, 1, 1)),
           geom(1, 1, 16, (40, 72), 5, (1, 2))]
    gs += [geom(1, 1, 16, (H, 72), P) for H in (20, 31, 32) for P in (3, 5, 7)]         # H < 32 with P <= 5
    gs += [geom(1, 1, 16, (H, 512), 5) for H in (240, 241, 255, 256, 257)]              # stripg's 16-row segments
    gs += [geom(1, 1, 16, (2, H, 256), 5) for H in (255, 256)]
    gs += [geom(1, 1, 72, (H, 64), 5) for H in (63, 64, 127, 128, 255, 256)]            # strip: Hz at the segment steps
    gs += [geom(1, 1, 169, (2 * Hz, 64), 7, 2) for Hz in (63, 64, 127, 128, 255, 256)]
    gs += [geom(2, 1, 16, (40, W), 5) for W in (31, 32, 33, 63, 64, 65, 70)]            # W against strips and tiles
    gs += [geom(2, 1, 100, (40, W), 7, 2) for W in (62, 64, 66, 70)]
    gs += [geom(1, 1, 16, (4, 40, 72), (2, 5, 5), pad=(1, 2, 2)), geom(1, 1, 16, (40, 72), 5, pad=(1, 1)),
           geom(1, 1, 16, (4, 40, 72), (3, 5, 5), pad=(0, 2, 2)), geom(1, 1, 72, (4, 40, 72), (1, 5, 5))]
    # the range rules: buffer descriptors (2^31 bytes per sample), grid extents, item counts
    gs += [geom(1, 1, 64, (4096, 2048), 5), geom(1, 1, 64, (4095, 2048), 5), geom(1, 1, 8, (65535, 64), 3),
           geom(1, 1, 8, (65536, 64), 3), geom(65535, 1, 8, (16, 32), 3), geom(65536, 1, 8, (16, 32), 3),
           geom(1, 1, 72, (65535, 64), 5), geom(1, 1, 72, (65536, 64), 5), geom(65536, 1, 72, (16, 32), 5),
           geom(1, 1, 192, (2048, 1366), 7), geom(1, 1, 192, (2048, 1364), 7, 2), geom(1, 1, 8, (16384, 32768), 3),
           geom(1, 1, 16, (4, 8388607), 3), geom(1, 1, 16, (4, 8388577), 3), geom(1, 1, 96, (4, 1398049), 3)]
    return gs


def query(lib, Geom, g):
    import ctypes
    gs = Geom(*g)
    ref = ctypes.byref(gs)
    return {"supported": int(lib.cdl_fusedg_supported(ref)),
            "frag_bytes": int(lib.cdl_fusedg_frag_bytes(ref)),
            "patch_floats": int(lib.cdl_fusedg_patch_floats(ref)),
            "tiles": int(lib.cdl_fusedg_tiles(ref)),
            "map_words": int(lib.cdl_fusedg_map_words(ref)),
            "code_layout": [int(lib.cdl_fusedg_code_layout(ref, t)) for t in (0, 1)],
            "code_floats": {"nchw": int(lib.cdl_fusedg_code_floats(ref, LAY_NCHW)),
                            "rsc": int(lib.cdl_fusedg_code_floats(ref, LAY_RSC))},
            "fused2d_supported": int(lib.cdl_fused2d_supported(ref))}


def record(setenv):
    """[{geom, strip0, strip1}]: the answers with CDL_FUSEDG_STRIP=0 / 1; setenv(name, value) sets a library switch."""
    import cdlnet_video_amd as cva
    out = [{"geom": g} for g in geometries()]
    for flag in ("0", "1"):
        setenv("CDL_FUSEDG_STRIP", flag)
        for e in out:
            e["strip" + flag] = query(cva._lib.lib(), cva._lib.Geom, e["geom"])
    return out


def main():
    import cdlnet_video_amd as cva

    def setenv(name, value):
        os.environ[name] = value
        cva._lib.reload_options()

    entries = record(setenv)
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in entries) + "\n]\n")
    n_sup = sum(e["strip0"]["supported"] for e in entries)
    print(f"{OUT}: {len(entries)} geometries ({n_sup} supported) from {cva._lib.LIB_PATH}")


if __name__ == "__main__":
    main()
