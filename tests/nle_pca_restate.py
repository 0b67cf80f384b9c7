"""Float64 restatement of the reference's weak-texture PCA noise estimate (model/nle.py:29-89, nle_pca), used by
test_nle_pca_cpu.py and test_gpu_nle_pca.py.  Written from the algorithm, not from the reference's code:
texture strengths from 2-D prefix sums of the squared half-differences, patches by unfold, second moments and the
smallest eigenvalue in float64."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("n1", "n2", "n3", "n4", "n5", "n6")


def load(name):
    """The fixture with its arrays at their stored precision (y float32, the rest float64 / int)."""
    raw = np.load(os.path.join(GOLDEN, f"{name}_nle_pca.npz"))
    return {k: raw[k] for k in raw.files}


def _box(a, bh, bw):
    """Sums of a (N, H, W) over every bh x bw window (stride 1): (N, H-bh+1, W-bw+1), from 2-D prefix sums."""
    s = torch.nn.functional.pad(a.cumsum(1).cumsum(2), (1, 0, 1, 0))
    return s[:, bh:, bw:] - s[:, :-bh, bw:] - s[:, bh:, :-bw] + s[:, :-bh, :-bw]


def texture(y, p):
    """Xtr of every p x p patch of y (N, H, W), flattened in (n, row, col) order, float64."""
    y = y.double()
    dh = (0.5 * y[:, :, :-2] - 0.5 * y[:, :, 2:]) ** 2
    dv = (0.5 * y[:, :-2, :] - 0.5 * y[:, 2:, :]) ** 2
    return (_box(dh, p, p - 2) + _box(dv, p - 2, p)).reshape(-1)


def patches(y, p):
    """(Np, p^2) float64 matrix of the p x p patches of y (N, H, W), rows in (n, row, col) order."""
    return y.double().unfold(1, p, 1).unfold(2, p, 1).reshape(-1, p * p)


def gram(y, p, tau):
    """(sum over patches with Xtr < tau of x x^T, their number) for one channel y (N, H, W)."""
    keep = texture(y, p) < tau
    X = patches(y, p)[keep]
    return X.T @ X, int(keep.sum())


def estimate(img, p, tau0, itr):
    """(nlevel, th, num) per channel of img (N, C, H, W) as float64 arrays (length C), steps 1-7 of the reference."""
    C = img.shape[1]
    out = np.zeros((3, C))
    for c in range(C):
        y = img[:, c]
        X, xtr = patches(y, p), texture(y, p)
        tau = np.inf
        if X.shape[0] < p * p:
            sig2 = 0.0
        else:
            sig2 = float(torch.linalg.eigvalsh(X.T @ X / (X.shape[0] - 1))[0])
        for _ in range(2, itr):
            tau = sig2 * tau0
            keep = xtr < tau
            X, xtr = X[keep], xtr[keep]
            if X.shape[0] < p * p:
                break
            sig2 = float(torch.linalg.eigvalsh(X.T @ X / (X.shape[0] - 1))[0])
        out[:, c] = np.sqrt(sig2), tau, X.shape[0]
    return out


def gap_threshold(xtr, q, q_hi=None):
    """A tau lying in the widest relative gap between neighbouring texture strengths xtr (float64) of the quantile
    range q..q_hi (default 0.8q..1.2q), float32-representable inside it: a kernel that computes Xtr in fp32 sees the
    same predicate as this float64 restatement.  Returns (tau, number of xtr below it)."""
    v, _ = torch.sort(xtr)
    n = v.numel()
    if q_hi is None:
        q, q_hi = 0.8 * q, 1.2 * q
    lo, hi = max(int(q * n), 0), min(int(q_hi * n), n - 1)
    rel = (v[lo + 1:hi + 1] - v[lo:hi]) / v[lo + 1:hi + 1]
    i = lo + int(torch.argmax(rel))
    tau = float(np.float32(0.5 * (float(v[i]) + float(v[i + 1]))))
    assert float(v[i]) < tau < float(v[i + 1]) and float(rel.max()) > 1e-5, "no usable gap"
    return tau, i + 1
