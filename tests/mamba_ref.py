"""Pure-torch restatement of mamba_ssm.Mamba(d_model, d_state=16, d_conv=4, expand=2), slow-path semantics, written from
the layer's definition (explicit loop over t, gradients from autograd).  Run in fp64 it is the reference of the Mamba
tests, run in fp32 on the CPU it is their yardstick.  Parity with the mamba_ssm CUDA kernels themselves is not pinned: the
library runs on no machine this project is tested on.

    xz = u in_proj^T;  x = silu(causal conv1d(x) + b);  x_dbl = x x_proj^T -> dt | Bm | Cm
    delta = softplus(dt dt_proj^T + dt_bias);  h_t = exp(delta_t A) h_{t-1} + delta_t x_t Bm_t;  y_t = <h_t, Cm_t> + D x_t
    out = (y silu(z)) out_proj^T
reverse=True walks the sequence back to front (== flip(f(flip(u))) along the sequence axis)."""
import math

import torch
import torch.nn.functional as F

NAMES = ("in_proj.weight", "conv1d.weight", "conv1d.bias", "x_proj.weight", "dt_proj.weight", "dt_proj.bias", "A_log", "D",
         "out_proj.weight")
N = 16


def shapes(d_model):
    D, r = 2 * d_model, math.ceil(d_model / 16)
    return {"in_proj.weight": (2 * D, d_model), "conv1d.weight": (D, 1, 4), "conv1d.bias": (D,),
            "x_proj.weight": (r + 2 * N, D), "dt_proj.weight": (D, r), "dt_proj.bias": (D,), "A_log": (D, N), "D": (D,),
            "out_proj.weight": (d_model, D)}


def _uniform(gen, shape, bound):
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1) * bound


def make_params(d_model, seed=0, wide=False):
    """fp64 parameter dict with mamba_ssm's names, shapes and initialisation (torch's default bounds for the Linear / Conv1d
    weights: U(+-1/sqrt(fan_in))).  wide: dt_proj.bias += U(0, 30) (softplus's linear branch, decays that underflow to 0),
    A_log += U(+-0.5), D += U(+-0.5)."""
    g = torch.Generator().manual_seed(seed)
    D, r = 2 * d_model, math.ceil(d_model / 16)
    p = {}
    p["in_proj.weight"] = _uniform(g, (2 * D, d_model), d_model ** -0.5)
    p["conv1d.weight"] = _uniform(g, (D, 1, 4), 0.5)
    p["conv1d.bias"] = _uniform(g, (D,), 0.5)
    p["x_proj.weight"] = _uniform(g, (r + 2 * N, D), D ** -0.5)
    p["dt_proj.weight"] = _uniform(g, (D, r), r ** -0.5)
    dt = torch.exp(torch.rand(D, generator=g, dtype=torch.float64) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
    dt = dt.clamp(min=1e-4)
    p["dt_proj.bias"] = dt + torch.log(-torch.expm1(-dt))
    p["A_log"] = torch.log(torch.arange(1, N + 1, dtype=torch.float64)).repeat(D, 1)
    p["D"] = torch.ones(D, dtype=torch.float64)
    p["out_proj.weight"] = _uniform(g, (d_model, D), D ** -0.5)
    if wide:
        p["dt_proj.bias"] = p["dt_proj.bias"] + torch.rand(D, generator=g, dtype=torch.float64) * 30
        p["A_log"] = p["A_log"] + _uniform(g, (D, N), 0.5)
        p["D"] = p["D"] + _uniform(g, (D,), 0.5)
    return p


def softplus(v):
    return torch.where(v > 20, v, torch.log1p(torch.exp(torch.clamp(v, max=20))))


def conv_ref(x, w, b, reverse=False):
    """x (B, L, D) -> silu(causal depthwise conv1d + bias)"""
    if reverse:
        return conv_ref(x.flip(1), w, b).flip(1)
    L = x.shape[1]
    y = F.conv1d(x.transpose(1, 2), w, b, padding=3, groups=w.shape[0])[..., :L]
    return F.silu(y).transpose(1, 2)


def scan_ref(u, delta_raw, dt_bias, A_log, Bm, Cm, Dp, z, reverse=False):
    """u, delta_raw, z (B, L, D); Bm, Cm (B, L, 16) -> (B, L, D); explicit loop over t"""
    Bsz, L, D = u.shape
    delta = softplus(delta_raw + dt_bias)
    A = -torch.exp(A_log)
    h = torch.zeros(Bsz, D, A.shape[1], dtype=u.dtype)
    ys = [None] * L
    order = range(L - 1, -1, -1) if reverse else range(L)
    for t in order:
        dA = torch.exp(delta[:, t, :, None] * A)
        h = dA * h + (delta[:, t] * u[:, t])[:, :, None] * Bm[:, t, None, :]
        ys[t] = (h * Cm[:, t, None, :]).sum(-1) + Dp * u[:, t]
    return torch.stack(ys, 1) * F.silu(z)


def mamba_ref(p, u, reverse=False):
    D = p["D"].shape[0]
    r = p["dt_proj.weight"].shape[1]
    xz = u @ p["in_proj.weight"].t()
    x, z = xz[..., :D], xz[..., D:]
    x = conv_ref(x, p["conv1d.weight"], p["conv1d.bias"], reverse)
    x_dbl = x @ p["x_proj.weight"].t()
    dt, Bm, Cm = x_dbl[..., :r], x_dbl[..., r:r + N], x_dbl[..., r + N:]
    y = scan_ref(x, dt @ p["dt_proj.weight"].t(), p["dt_proj.bias"], p["A_log"], Bm, Cm, p["D"], z, reverse)
    return y @ p["out_proj.weight"].t()


def make_input(d_model, B, L, seed=0, wide=False):
    g = torch.Generator().manual_seed(1000 + seed)
    u = torch.randn(B, L, d_model, generator=g, dtype=torch.float64)
    dout = torch.randn(B, L, d_model, generator=g, dtype=torch.float64)
    return (u * 2 if wide else u), dout


def layer_run(p64, u64, dout64, reverse, dtype):
    """-> {"out", "input", <nine names>}: output and the ten gradients of sum(out * dout), computed in `dtype` on the CPU"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    u = u64.to(dtype).clone().requires_grad_(True)
    out = mamba_ref(p, u, reverse)
    (out * dout64.to(dtype)).sum().backward()
    res = {"out": out.detach(), "input": u.grad}
    res.update({k: p[k].grad for k in NAMES})
    return res


def rel_err(a, ref):
    """max |a - ref| / max |ref| against the fp64 reference; an identically zero reference demands an exact zero"""
    a, ref = a.double().cpu(), ref.double()
    assert torch.isfinite(a).all() and torch.isfinite(ref).all()
    m = ref.abs().max().item()
    if m == 0.0:
        assert (a == 0).all(), "reference is identically zero, result is not"
        return 0.0
    return ((a - ref).abs().max() / m).item()


def bar(e_32):
    """the gate on e_hip: one decimal order over the CPU's own fp32 error, floor 1e-5"""
    return max(10 * e_32, 1e-5)
