"""Pure-torch, dtype-generic restatement of the reference's bi-branch Mamba fusion stage (MambaBlock, MambaFusion;
mambafuser_seq.py:74-231) over tests/mamba_ref.mamba_ref, written from the stage's definition with the flips spelled out.
Run in fp64 it is the reference of the fusion-stage tests, run in fp32 on the CPU it is their yardstick; in fp64 it is pinned
to the reference's own MambaFusion by tests/golden/make_golden_mambafusion.py.

    MambaBlock   x1 = fc1(LayerNorm_(T, C)(x));  fm = mamba_f(x1);  xf = flip(x1, 1);  bm = mamba_b(xf)
                 out = bm * leaky_relu_0.2(fc2(xf)) + fm * bm                        (no residual, nothing flipped back)
    MambaFusion  tokens = pos_emb + cat(swapped image / lidar / radar tokens, gps);  blocks;  ln_f;  unpack without a swap
Parameters are a flat dict under the reference's state-dict names."""
import math

import torch
import torch.nn.functional as F

from tests import mamba_ref as mr

BLOCK_PLAIN = ("ln1.weight", "ln1.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
BRANCHES = ("forward_mamba", "backward_mamba")


def block_names():
    """the 24 parameter names of one MambaBlock, in the module's registration order"""
    return BLOCK_PLAIN + tuple(f"{br}.{k}" for br in BRANCHES for k in mr.NAMES)


def block_shapes(C, T):
    s = {"ln1.weight": (T, C), "ln1.bias": (T, C), "fc1.weight": (C, C), "fc1.bias": (C,), "fc2.weight": (C, C),
         "fc2.bias": (C,)}
    for br in BRANCHES:
        s.update({f"{br}.{k}": v for k, v in mr.shapes(C).items()})
    return s


def fusion_names(n_layer):
    return ("pos_emb",) + tuple(f"mambablocks.{i}.{k}" for i in range(n_layer) for k in block_names()) + \
        ("ln_f.weight", "ln_f.bias")


def fusion_shapes(C, S, n_layer):
    T = 192 * S + 2
    s = {"pos_emb": (1, T, C), "ln_f.weight": (C,), "ln_f.bias": (C,)}
    for i in range(n_layer):
        s.update({f"mambablocks.{i}.{k}": v for k, v in block_shapes(C, T).items()})
    return s


def _uniform(g, shape, bound):
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound


def _normal(g, shape, std):
    return torch.randn(shape, generator=g, dtype=torch.float64) * std


def make_block_params(C, T, seed=0, spread=True, wide=False):
    """fp64 parameters of one block.
    spread=True : Linear weights U(+-fan_in^-1/2); biases and the LN bias U(+-0.5); LN weight 1 + U(+-0.5); the Mamba
                  parameters of mr.make_params (wide: its wide set).  Outputs and gradients are O(1).
    spread=False: the reference's initialisation (self.apply(_init_weights)): every Linear N(0, 0.02) with zero bias - the
                  four inside each Mamba too, so dt_proj.bias is 0 - LN (1, 0); A_log, D, conv1d as mamba_ssm sets them."""
    g = torch.Generator().manual_seed(7000 + seed)
    p = {}
    if spread:
        p["ln1.weight"] = 1 + _uniform(g, (T, C), 0.5)
        p["ln1.bias"] = _uniform(g, (T, C), 0.5)
        for fc in ("fc1", "fc2"):
            p[f"{fc}.weight"] = _uniform(g, (C, C), C ** -0.5)
            p[f"{fc}.bias"] = _uniform(g, (C,), 0.5)
    else:
        p["ln1.weight"] = torch.ones(T, C, dtype=torch.float64)
        p["ln1.bias"] = torch.zeros(T, C, dtype=torch.float64)
        for fc in ("fc1", "fc2"):
            p[f"{fc}.weight"] = _normal(g, (C, C), 0.02)
            p[f"{fc}.bias"] = torch.zeros(C, dtype=torch.float64)
    for j, br in enumerate(BRANCHES):
        m = mr.make_params(C, seed=seed * 2 + j, wide=wide and spread)
        if not spread:
            for k in ("in_proj.weight", "x_proj.weight", "dt_proj.weight", "out_proj.weight"):
                m[k] = _normal(g, tuple(m[k].shape), 0.02)
            m["dt_proj.bias"] = torch.zeros_like(m["dt_proj.bias"])
        p.update({f"{br}.{k}": v for k, v in m.items()})
    return {k: p[k] for k in block_names()}


def make_fusion_params(C, S, n_layer, seed=0, spread=True, wide=False):
    T = 192 * S + 2
    g = torch.Generator().manual_seed(8000 + seed)
    p = {"pos_emb": _uniform(g, (1, T, C), 0.5) if spread else torch.zeros(1, T, C, dtype=torch.float64)}
    for i in range(n_layer):
        b = make_block_params(C, T, seed=seed * 16 + i, spread=spread, wide=wide)
        p.update({f"mambablocks.{i}.{k}": v for k, v in b.items()})
    p["ln_f.weight"] = 1 + _uniform(g, (C,), 0.5) if spread else torch.ones(C, dtype=torch.float64)
    p["ln_f.bias"] = _uniform(g, (C,), 0.5) if spread else torch.zeros(C, dtype=torch.float64)
    return {k: p[k] for k in fusion_names(n_layer)}


def block_ref(p, x, pre="", probe=None):
    """x (B, T, C) -> (B, T, C).  probe: a list that receives fc2's output (the LeakyReLU pre-activation)"""
    T, C = x.shape[1:]
    sub = lambda br: {k: p[f"{pre}{br}.{k}"] for k in mr.NAMES}
    x1 = F.linear(F.layer_norm(x, (T, C), p[pre + "ln1.weight"], p[pre + "ln1.bias"], 1e-5), p[pre + "fc1.weight"],
                  p[pre + "fc1.bias"])
    fm = mr.mamba_ref(sub("forward_mamba"), x1)
    xf = x1.flip(1)
    bm = mr.mamba_ref(sub("backward_mamba"), xf)
    f2 = F.linear(xf, p[pre + "fc2.weight"], p[pre + "fc2.bias"])
    if probe is not None:
        probe.append(f2.detach())
    return bm * F.leaky_relu(f2, 0.2) + fm * bm


def swap_pack_ref(image, lidar, radar, gps, S):
    """three (B*S, C, 8, 8) maps + gps (B, 2, C) -> tokens (B, 192 S + 2, C) before pos_emb, channel swap included"""
    C = image.shape[1]
    B = image.shape[0] // S
    maps = [t.reshape(B, S, C, 64) for t in (image, lidar, radar)]
    s1, s2 = C // 3, C // 3 * 2
    seg = torch.zeros(C, dtype=torch.long)
    seg[s1:s2], seg[s2:] = 1, 2
    stack = torch.stack(maps, 0)                                  # (3, B, S, C, 64)
    toks = []
    for m in range(3):
        src = (m + seg) % 3                                       # source modality of every channel
        cs = stack[src, :, :, torch.arange(C)]                    # (C, B, S, 64)
        toks.append(cs.permute(1, 2, 3, 0).reshape(B, S * 64, C))
    return torch.cat(toks + [gps], 1)


def unpack_ref(x, S):
    """tokens (B, T, C) -> (image, lidar, radar (B*S, C, 8, 8), gps rows (B, 2, C)), no swap"""
    B, T, C = x.shape
    body = x[:, :T - 2].reshape(B, 3, S, 8, 8, C).permute(0, 1, 2, 5, 3, 4)
    return tuple(body[:, m].reshape(B * S, C, 8, 8) for m in range(3)) + (x[:, T - 2:],)


def fusion_ref(p, n_layer, S, image, lidar, radar, gps, probe=None):
    C = image.shape[1]
    x = p["pos_emb"] + swap_pack_ref(image, lidar, radar, gps, S)
    for i in range(n_layer):
        x = block_ref(p, x, f"mambablocks.{i}.", probe)
    x = F.layer_norm(x, (C,), p["ln_f.weight"], p["ln_f.bias"], 1e-5)
    return unpack_ref(x, S)


OUT_KEYS = ("image_out", "lidar_out", "radar_out", "gps_out")
IN_KEYS = ("image", "lidar", "radar", "gps")


def make_block_input(C, B, T, seed=0):
    g = torch.Generator().manual_seed(9000 + seed)
    return torch.randn(B, T, C, generator=g, dtype=torch.float64), torch.randn(B, T, C, generator=g, dtype=torch.float64)


def make_fusion_inputs(C, B, S, seed=0):
    """-> (inputs dict, output-gradient dict), fp64"""
    g = torch.Generator().manual_seed(9500 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ins = {"image": rn(B * S, C, 8, 8), "lidar": rn(B * S, C, 8, 8), "radar": rn(B * S, C, 8, 8), "gps": rn(B, 2, C)}
    douts = {"image_out": rn(B * S, C, 8, 8), "lidar_out": rn(B * S, C, 8, 8), "radar_out": rn(B * S, C, 8, 8),
             "gps_out": rn(B, 2, C)}
    return ins, douts


def kink_margin(probe):
    """min over the blocks of min|fc2 output| / max|fc2 output|"""
    return min((f.abs().min() / f.abs().max()).item() for f in probe)


def block_run(p64, x64, dout64, dtype):
    """-> ({"out", "input", <24 names>}, kink margin): output and the 25 gradients of sum(out * dout) in `dtype` on the CPU"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    x = x64.to(dtype).clone().requires_grad_(True)
    probe = []
    out = block_ref(p, x, "", probe)
    (out * dout64.to(dtype)).sum().backward()
    res = {"out": out.detach(), "input": x.grad}
    res.update({k: p[k].grad for k in p})
    return res, kink_margin(probe)


def fusion_run(p64, ins64, douts64, n_layer, S, dtype):
    """-> ({four outputs, "d" + four inputs, every parameter name}, kink margin)"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    ins = {k: v.to(dtype).clone().requires_grad_(True) for k, v in ins64.items()}
    probe = []
    outs = fusion_ref(p, n_layer, S, *(ins[k] for k in IN_KEYS), probe=probe)
    sum((o * douts64[k].to(dtype)).sum() for k, o in zip(OUT_KEYS, outs)).backward()
    res = {k: o.detach() for k, o in zip(OUT_KEYS, outs)}
    res.update({"d" + k: ins[k].grad for k in IN_KEYS})
    res.update({k: p[k].grad for k in p})
    return res, kink_margin(probe)


KINK_MIN = 2e-6   # every module-level case: min|fc2 out| >= KINK_MIN * max|fc2 out| in every block, on the fp64 run

# The module-level cases of the CPU and GPU tests.  The seeds were picked on the CPU so that the kink condition holds.
# (B, L, C, wide, seed)
BLOCK_CASES = [(2, 37, 64, False, 1), (2, 37, 64, True, 1), (2, 194, 128, False, 1), (2, 194, 128, True, 1)]
# (C, seq_len, n_layer, B, spread, parameter seed, input seed)
FUSION_CASES = [(64, 1, 2, 2, True, 1, 1), (64, 1, 2, 2, False, 10, 10), (128, 1, 1, 2, True, 1, 1), (64, 5, 1, 1, True, 1, 1)]
