"""tests/mamba_ref.py's layer with a store() hook at exactly the tensors the 16-bit-storage path of
deepsense6g_tii_amd/mamba.py keeps in bf16 / f16 (its module docstring has the storage map); everything else runs in the
dtype of the inputs (fp64 in the tests).

    activations   u, xz, xc, y, out: rounded on the way forward, their gradients (du, dxz, dxc, dy, dout) on the way back.
                  dxc is the SUM of the scan's du and x_proj's data gradient, rounded once - autograd sums before the hook.
    weights       in_proj, out_proj: the GEMMs read a 16-bit copy forward and for the data gradient; x_proj: forward only
                  (its data gradient is an fp32 GEMM on the fp32 master).  Weight gradients are fp32: never rounded.
With the identity hook this is mamba_ref.mamba_ref bit for bit (tests/test_mamba16_cpu.py)."""
import torch

from tests import mamba_ref as mr


def rounder(dtype):
    """-> store(t): t rounded to `dtype` (RNE) and back to t's own dtype; None -> the identity"""
    if dtype is None:
        return lambda t: t
    return lambda t: t.to(dtype).to(t.dtype)


class _Act(torch.autograd.Function):
    """a stored activation: value rounded forward, gradient rounded backward"""

    @staticmethod
    def forward(ctx, t, store):
        ctx.store = store
        return store(t)

    @staticmethod
    def backward(ctx, g):
        return ctx.store(g), None


class _Weight(torch.autograd.Function):
    """the 16-bit copy of an fp32 master: rounded forward, its gradient passes unrounded"""

    @staticmethod
    def forward(ctx, w, store):
        return store(w)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _XProj(torch.autograd.Function):
    """x @ store(w)^T forward; backward on the master: dx = g @ w, dw = g^T x"""

    @staticmethod
    def forward(ctx, x, w, store):
        ctx.save_for_backward(x, w)
        return x @ store(w).t()

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2, x2 = g.reshape(-1, g.shape[-1]), x.reshape(-1, x.shape[-1])
        return g @ w, (x2.t() @ g2).t(), None


def mamba16_ref(p, u, reverse=False, store=lambda t: t):
    D = p["D"].shape[0]
    r = p["dt_proj.weight"].shape[1]
    act = lambda t: _Act.apply(t, store)
    u = act(u)
    xz = act(u @ _Weight.apply(p["in_proj.weight"], store).t())
    x, z = xz[..., :D], xz[..., D:]
    x = act(mr.conv_ref(x, p["conv1d.weight"], p["conv1d.bias"], reverse))
    x_dbl = _XProj.apply(x, p["x_proj.weight"], store)
    dt, Bm, Cm = x_dbl[..., :r], x_dbl[..., r:r + mr.N], x_dbl[..., r + mr.N:]
    y = act(mr.scan_ref(x, dt @ p["dt_proj.weight"].t(), p["dt_proj.bias"], p["A_log"], Bm, Cm, p["D"], z, reverse))
    return act(y @ _Weight.apply(p["out_proj.weight"], store).t())


def layer_run16(p64, u64, dout64, reverse, store, dtype=torch.float64):
    """mamba_ref.layer_run on mamba16_ref: -> {"out", "input", <nine names>}"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    u = u64.to(dtype).clone().requires_grad_(True)
    out = mamba16_ref(p, u, reverse, store)
    (out * dout64.to(dtype)).sum().backward()
    res = {"out": out.detach(), "input": u.grad}
    res.update({k: p[k].grad for k in mr.NAMES})
    return res
