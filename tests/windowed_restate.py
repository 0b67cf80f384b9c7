"""The unrolled loop on a PRE-PROCESSED frame, restated in float64 torch convolutions: the `sweep` that
loop.run_windows accepts in place of the device sweep, and the untiled result the windowed one is compared with.

    z_1     = ST(A_0 yp, tau_0)
    z_{k+1} = ST(z_k - A_k(mask B_k z_k - yp), tau_k)
    xp      = B_0 z_K                                   tau_k = t[k,0] + c t[k,1]

A_k: zero-padded strided correlation (padding P // 2), B_k: its transposed form with output_padding s - 1.  c: None, one
level per sample (N,), or a map (N, 1, *code grid)."""
import torch
import torch.nn.functional as F


def random_net(K, M, C, P, seed, scale=0.25):
    """(A, B, t) in float64: K analysis / synthesis banks (M, C, *P) and positive thresholds (K, 2, M, 1, ..)."""
    g = torch.Generator().manual_seed(seed)
    P = tuple(P)
    A = [scale * torch.randn((M, C) + P, generator=g, dtype=torch.float64) for _ in range(K)]
    B = [scale * torch.randn((M, C) + P, generator=g, dtype=torch.float64) for _ in range(K)]
    t = 0.02 + 0.05 * torch.rand((K, 2, M) + (1,) * len(P), generator=g, dtype=torch.float64)
    return A, B, t


def make_sweep(A, B, t, s):
    """sweep(yp, mask_p, c) -> xp."""
    nd = A[0].dim() - 2
    pad = tuple(p // 2 for p in A[0].shape[2:])
    conv, convT = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    K = len(A)

    def st(u, tau):
        return torch.sign(u) * torch.relu(u.abs() - tau)

    def sweep(yp, mask_p, c):
        if c is None:
            level = 0.0
        elif c.dim() == 1:
            level = c.reshape((-1, 1) + (1,) * nd)
        else:
            level = c
        tau = lambda k: t[k, 0].unsqueeze(0) + level * t[k, 1].unsqueeze(0)
        z = st(conv(yp, A[0], stride=s, padding=pad), tau(0))
        for k in range(1, K):
            r = convT(z, B[k], stride=s, padding=pad, output_padding=s - 1)
            if mask_p is not None:
                r = mask_p * r
            z = st(z - conv(r - yp, A[k], stride=s, padding=pad), tau(k))
        return convT(z, B[0], stride=s, padding=pad, output_padding=s - 1)

    return sweep
