"""The call chains of the cm* / cd1 fixtures (tools/make_golden_csr_map.py), written once over an abstract
`call(y, z_prev, z_after, sigma) -> (xhat, z)`: the CPU oracle and the product's csr_step replay the same sequence."""
import torch

FIXTURES = {"cm1": "cm1_csr_chain_map", "cm1b": "cm1b_csr_s2_odd_map", "cm2": "cm2_csrf2_chain_map",
            "cd1": "cd1_csr_chain_datagrad"}
VARIANT = {"cm1": "csr", "cm1b": "csr", "cm2": "f2", "cd1": "csr"}
mse = lambda a, b: torch.mean((a - b) ** 2)

# The recorded gradient of a code that the chain hands on (grad_z0, grad_zp, ...) is the reference's retained .grad: it
# includes the path through the same call's own xhat = D z, which is inside the product's autograd node; the device test
# adds that path to the .grad of the code csr_step returned.
INTERNAL = ("grad_z0", "grad_z1", "grad_zp", "grad_zc", "grad_za")


def replay(kind, g, call, dev="cpu"):
    """Runs fixture `kind` through `call`.  Returns (loss, outs {recorded name: tensor}, leaves {recorded gradient name:
    the tensor whose .grad it is}); call loss.backward() to fill the gradients."""
    T = lambda k: g[k].to(dev)
    leaf = lambda k: g[k].to(dev).clone().requires_grad_(True)
    w = T("w")
    if kind in ("cm1", "cd1"):
        y0, y1, s0 = leaf("y0"), leaf("y1"), leaf("sigma0")
        s1 = leaf("sigma1") if kind == "cm1" else s0
        xh0, z0 = call(y0, None, None, s0)
        xh1, z1 = call(y1, z0, None, s1)
        xh0b, z0b = call(y0, z1, None, s0)
        z0.retain_grad()
        z1.retain_grad()
        outs = dict(xh0=xh0, z0=z0, xh1=xh1, z1=z1, xh0b=xh0b, z0b=z0b)
        loss = mse(T("x0"), xh0) + mse(T("x1"), xh1) + mse(T("x0"), xh0b) + torch.mean(w * xh0) + torch.mean(w * xh1) \
            + torch.mean(w * xh0b)
        leaves = dict(dy0=y0, dy1=y1, grad_z0=z0, grad_z1=z1, dsigma0=s0)
        if kind == "cm1":
            leaves["dsigma1"] = s1
        return loss, outs, leaves
    if kind == "cm1b":
        y, zprev, s0 = leaf("y"), leaf("zprev"), leaf("sigma0")
        xh, z = call(y, zprev, None, s0)
        loss = mse(T("x"), xh) + 0.1 * z.abs().mean() + torch.mean(w * xh)
        return loss, dict(xhat=xh, z=z), dict(dy=y, grad_zprev=zprev, dsigma0=s0)
    ys, s0 = [leaf(k) for k in ("y0", "y1", "y2")], leaf("sigma0")
    xp, zp = call(ys[0], None, None, s0)
    xc, zc = call(ys[1], zp, None, s0)
    xa, za = call(ys[2], zc, None, s0)
    xc2, zc2 = call(ys[1], zp, za, s0)
    xp2, zp2 = call(ys[0], None, za, s0)
    for z in (zp, zc, za):
        z.retain_grad()
    outs = dict(xp=xp, zp=zp, xc=xc, zc=zc, xa=xa, za=za, xc2=xc2, zc2=zc2, xp2=xp2, zp2=zp2)
    loss = mse(T("x0"), xp) + mse(T("x1"), xc) + mse(T("x2"), xa) + mse(T("x1"), xc2) + mse(T("x0"), xp2) \
        + sum(torch.mean(w * outs[k]) for k in ("xp", "xc", "xa", "xc2", "xp2"))
    return loss, outs, dict(dy0=ys[0], dy1=ys[1], dy2=ys[2], grad_zp=zp, grad_zc=zc, grad_za=za, dsigma0=s0)
