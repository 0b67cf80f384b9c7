"""Shared by tests/test_frame_levels_cpu.py and tests/test_gpu_frame_levels.py: the clips, nets and per-frame noise levels of
the frame-level route.

Every net is a CDLNetVideo with adaptive thresholds, t0 = 5e-3 (the thresholds stay at t0: the filters are de-tied, as in
smoke()'s video case).  The filters are scaled by a short power method on a small probe instead of the constructor's 200
iterations on 128 x 128: the tests need a contraction, not the reference's exact constant."""
import torch

# label -> M, P, clip shape (N,C,D,H,W), K.  On the 64 x 16 tile: A has 2 x 2 tiles per plane; E has 270 tiles, more than the
# device has compute units, so persistent workgroups walk on to tiles of other planes and samples in both tile orders.
CASES = {
    "A": dict(M=16, P=(3, 3, 3), shape=(2, 1, 4, 20, 70), K=3),
    "B": dict(M=48, P=(5, 5, 5), shape=(2, 1, 5, 33, 65), K=3),
    "C": dict(M=64, P=(7, 5, 5), shape=(1, 1, 7, 16, 64), K=3),
    "D": dict(M=32, P=(1, 7, 7), shape=(2, 3, 3, 18, 66), K=3, bayer=True),
    "E": dict(M=16, P=(3, 3, 3), shape=(3, 1, 5, 96, 192), K=2),
    "F": dict(M=32, P=(7, 5, 5), shape=(1, 1, 7, 16, 64), K=3),
}
# C is NOT a geometry of the fused generic tier: with P = 5 and G = 7 the tile plan's LDS carve passes 160 KB from M = 40 on
# (tests/test_gpu_fusedg_cells.py REFUSED), so at M = 64 every sigma form runs the generic tier and the knob must change
# nothing.  F is C at the largest M the plan takes: G = 7 and N = 1 on the fused tier.
REFUSED = ("C",)
# the clip of the tangent checks (net.jvp, sure_loss): xdot is taken at the primal's supports, so two routes agree on it only
# where they agree on every support -- a flipped near-tie moves xdot by a whole filter patch.  Small
# enough that the two routes' supports coincide (the tests assert that they do), 2 x 2 tiles on each of its 4 planes.
TANGENT_CASE = dict(M=8, P=(3, 3, 3), shape=(2, 1, 2, 20, 70), K=3)
T0 = 5e-3


def build(label, seed=71):
    """(net on the CPU, state dict, x, y, mask or None, w, levels (N,1,D,1,1)) of a case."""
    import cdlnet_video_amd as cva
    from cdlnet_video_amd.solvers import gram_operator, power_method
    cfg = CASES[label] if isinstance(label, str) else label
    shape, P = cfg["shape"], tuple(cfg["P"])
    N, C, D = shape[:3]
    torch.manual_seed(seed)
    net = cva.CDLNetVideo(K=cfg["K"], M=cfg["M"], P=P, s=1, C=C, t0=T0, adaptive=True, depth=D, init=False)
    with torch.no_grad():
        op = gram_operator(net.A[0].weight, net.D.weight, 1, tuple(p // 2 for p in P))
        L = power_method(op, torch.rand(1, C, D, 32, 32), num_iter=30, verbose=False)[0]
        for n, p in net.named_parameters():
            if n != "t":
                p.div_(L ** 0.5)
                p.add_(0.05 * p.abs().mean() * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(seed + 1)
    x = cva.utils.synthetic_clip(shape, seed=seed + 2)
    lev = levels(N, D, seed + 3)
    y = x + torch.randn(shape, generator=gen) * lev / 255
    mask = cva.utils.gen_bayer_mask3d(x) if cfg.get("bayer") else None
    if mask is not None:
        y = mask * y
    w = torch.randn(shape, generator=gen)
    return net, sd, x, y, mask, w, lev


def levels(N, D, seed):
    """One level per (sample, frame), all distinct: a seeded permutation of N * D evenly spaced values in [8, 60)."""
    gen = torch.Generator().manual_seed(seed)
    order = torch.randperm(N * D, generator=gen).to(torch.float32)
    return (8.0 + 52.0 * order / (N * D)).reshape(N, 1, D, 1, 1)


def misread(lev):
    """The levels a kernel would apply if it read another row of the (N*D, M) threshold table than n * D + zd: row n, row
    zd, and row d * N + n (the transposed table)."""
    N, D = lev.shape[0], lev.shape[2]
    flat = lev.reshape(-1)
    n = torch.arange(N).reshape(N, 1).expand(N, D)
    d = torch.arange(D).reshape(1, D).expand(N, D)
    pick = lambda idx: flat[idx.reshape(-1)].reshape(lev.shape)
    return {"row n": pick(n), "row zd": pick(d), "row d*N+n": pick(d * N + n)}
