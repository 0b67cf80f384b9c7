"""The scratch layout of cdl_vgg_forward / cdl_vgg_backward (csrc/cdl_vgg.hip: layout_of, set_at), restated: views of what the
forward keeps and the backward leaves, shared by test_gpu_perceptual.py and test_gpu_dense_cells.py."""
import math

import torch

VGG_LAYERS = ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256))     # (in, out) of the six dense-tier layers
VGG_LEVEL = (0, 1, 1, 2, 2, 2)                                                         # the resolution level each runs at


def up64(n):
    return (n + 63) // 64 * 64


def scratch_layout(P, H, W, grads):
    """Offsets (floats) of the parts of the scratch and the extents of the three levels: a dict with part, nparts, fy, sx, sy
    (None without CDL_VGG_DY), sets (one offset per activation set), g_a, g_b, total, and dims [(H, W)] * 3."""
    H2, W2 = H // 2, W // 2
    H4, W4 = H2 // 2, W2 // 2
    px0, px1, px2 = P * H * W, P * H2 * W2, P * H4 * W4
    frag = 0
    for i, o in VGG_LAYERS:
        for a, b in ((i, o), (o, i)):
            mtt = 2 * math.ceil(math.ceil(b / 32) / 2)
            frag = max(frag, math.ceil(a / 16) * 9 * mtt * 128 * 4)
    part = up64(frag) + 576
    nparts = P * math.ceil(W4 / 32) * math.ceil(H4 / 16) * 4
    fy = part + up64(2 * nparts)
    f3 = up64(256 * px2)
    sx = fy + f3
    sy = sx + f3
    base = sy + (f3 if grads & 2 else 0)
    set_floats = (up64(64 * px0) + up64(64 * px1) + up64((64 * px1 + 3) // 4) + up64(128 * px1) + up64(128 * px2)
                  + up64((128 * px2 + 3) // 4) + 2 * up64(256 * px2))
    nsets = 2 if grads & 2 else 1
    g_a = base + nsets * set_floats
    g_b = g_a + up64(max(256 * px2, 128 * px2, 64 * px1))
    total = g_b + up64(max(64 * px0, 256 * px2))
    return dict(part=part, nparts=nparts, fy=fy, sx=sx, sy=sy if grads & 2 else None, sets=[base + k * set_floats for k in range(nsets)],
                g_a=g_a, g_b=g_b, total=total, dims=[(H, W), (H2, W2), (H4, W4)], px=(px0, px1, px2))


def _set_views(scr, q, P, dims):
    (H, W), (H2, W2), (H4, W4) = dims
    px0, px1, px2 = P * H * W, P * H2 * W2, P * H4 * W4
    views = {}
    for name, n, shape, byte in (("a1", 64 * px0, (P, 64, H, W), False), ("p1", 64 * px1, (P, 64, H2, W2), False),
                                 ("am1", 64 * px1, (P, 64, H2, W2), True), ("a3", 128 * px1, (P, 128, H2, W2), False),
                                 ("p2", 128 * px2, (P, 128, H4, W4), False), ("am2", 128 * px2, (P, 128, H4, W4), True),
                                 ("a5", 256 * px2, (P, 256, H4, W4), False), ("a6", 256 * px2, (P, 256, H4, W4), False)):
        if byte:
            views[name] = scr[q:q + (n + 3) // 4].view(torch.uint8)[:n].reshape(shape)
            q += up64((n + 3) // 4)
        else:
            views[name] = scr[q:q + n].reshape(shape)
            q += up64(n)
    return views


def scratch_views(scr, P, H, W, grads):
    """The activations cdl_vgg_forward keeps, read from its scratch: (set of x, set of y or None, fy)."""
    L = scratch_layout(P, H, W, grads)
    s0 = _set_views(scr, L["sets"][0], P, L["dims"])
    s1 = _set_views(scr, L["sets"][1], P, L["dims"]) if grads & 2 else None
    H4, W4 = L["dims"][2]
    return s0, s1, scr[L["fy"]:L["fy"] + 256 * L["px"][2]].reshape(P, 256, H4, W4)


def scratch_extras(scr, P, H, W, grads):
    """What the DIFF form and the backward leave: the seeds (seed_y None without CDL_VGG_DY), the fp64 partial sums, and the
    two gradient ping-pong buffers as flat views of their whole extents (the caller shapes what the last launches left)."""
    L = scratch_layout(P, H, W, grads)
    H4, W4 = L["dims"][2]
    n3 = 256 * L["px"][2]
    seed = lambda q: None if q is None else scr[q:q + n3].reshape(P, 256, H4, W4)         # noqa: E731
    return dict(seed_x=seed(L["sx"]), seed_y=seed(L["sy"]),
                partial=scr[L["part"]:L["part"] + 2 * L["nparts"]].view(torch.float64),
                g_a=scr[L["g_a"]:L["g_b"]], g_b=scr[L["g_b"]:L["total"]])
