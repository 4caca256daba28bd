"""tests/mamba_fusion_ref.py's block and the walk-form stage composition with a store() hook at exactly the tensors the
16-bit-storage path of deepsense6g_tii_amd/mamba_fusion.py keeps in bf16 / f16 (its module docstring has the storage map);
everything else runs in the dtype of the inputs (fp64 in the tests).

    block   x, xl = ln1(x), x1 = fc1(xl), fm, bm, f2, out: rounded on the way forward, their gradients on the way back.
            dx1 is the SUM of fc2's data gradient and the two Mamba layers' input gradients, rounded once - autograd sums
            before x1's hook; so the layers are restated WITHOUT tests/mamba16_ref.py's hook on their input (its value is
            x1, already stored; its gradient joins the fp32 sum unrounded).
            fc1 / fc2 weights: a 16-bit copy forward and in the data gradient; their gradients and the biases are fp32.
    stage   the three NHWC maps in and out and the tokens out of the pack: rounded, gradients too (a map's gradient is the sum
            of the residual path's and the pack's, rounded once).  gemb, pos_emb, the widened ln_f input, the returned tokens
            and their gradients: not rounded.
With the identity hook the block is mamba_fusion_ref.block_ref and the stage the composition torch average pool -> swap ->
blocks -> ln_f -> F.interpolate -> add, bit for bit (tests/test_mamba_fusion16_cpu.py)."""
import torch
import torch.nn.functional as F

from tests import mamba16_ref as m16
from tests import mamba_fusion_ref as fr
from tests import mamba_ref as mr


def _layer(p, u, reverse, store):
    """m16.mamba16_ref without the hook on u"""
    D = p["D"].shape[0]
    r = p["dt_proj.weight"].shape[1]
    act = lambda t: m16._Act.apply(t, store)                       # noqa: E731
    xz = act(u @ m16._Weight.apply(p["in_proj.weight"], store).t())
    x, z = xz[..., :D], xz[..., D:]
    x = act(mr.conv_ref(x, p["conv1d.weight"], p["conv1d.bias"], reverse))
    x_dbl = m16._XProj.apply(x, p["x_proj.weight"], store)
    dt, Bm, Cm = x_dbl[..., :r], x_dbl[..., r:r + mr.N], x_dbl[..., r + mr.N:]
    y = act(mr.scan_ref(x, dt @ p["dt_proj.weight"].t(), p["dt_proj.bias"], p["A_log"], Bm, Cm, p["D"], z, reverse))
    return act(y @ m16._Weight.apply(p["out_proj.weight"], store).t())


def block16_ref(p, x, pre="", probe=None, store=lambda t: t):
    """fr.block_ref with the hooks; probe receives fc2's output BEFORE it is stored (the LeakyReLU pre-activation)"""
    T, C = x.shape[1:]
    act = lambda t: m16._Act.apply(t, store)                       # noqa: E731
    wt = lambda k: m16._Weight.apply(p[pre + k], store)            # noqa: E731
    sub = lambda br: {k: p[f"{pre}{br}.{k}"] for k in mr.NAMES}    # noqa: E731
    x = act(x)
    xl = act(F.layer_norm(x, (T, C), p[pre + "ln1.weight"], p[pre + "ln1.bias"], 1e-5))
    x1 = act(F.linear(xl, wt("fc1.weight"), p[pre + "fc1.bias"]))
    fm = _layer(sub("forward_mamba"), x1, False, store)
    xf = x1.flip(1)
    bm = _layer(sub("backward_mamba"), xf, False, store)
    f2 = F.linear(xf, wt("fc2.weight"), p[pre + "fc2.bias"])
    if probe is not None:
        probe.append(f2.detach())
    f2 = act(f2)
    return act(bm * F.leaky_relu(f2, 0.2) + fm * bm)


def block_run16(p64, x64, dout64, store, dtype=torch.float64):
    """fr.block_run on block16_ref -> ({"out", "input", <24 names>}, kink margin on the pre-store f2)"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    x = x64.to(dtype).clone().requires_grad_(True)
    probe = []
    out = block16_ref(p, x, "", probe, store)
    (out * dout64.to(dtype)).sum().backward()
    res = {"out": out.detach(), "input": x.grad}
    res.update({k: p[k].grad for k in p})
    return res, fr.kink_margin(probe)


def stage_run16(p64, x64, d64, n_layer, S, store, dtype=torch.float64):
    """the walk-form stage: x64 = {feat0..2 (NHWC [B * S, H, H, C]), gemb}, d64 = {out0..2, gps_out} ->
    ({out0..2, gps_out, dfeat0..2, dgemb, <parameter names>}, kink margin)"""
    act = lambda t: m16._Act.apply(t, store)                       # noqa: E731
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    x = {k: v.to(dtype).clone().requires_grad_(True) for k, v in x64.items()}
    feats = [act(x[f"feat{m}"]) for m in range(3)]
    H, C = feats[0].shape[1], feats[0].shape[3]
    probe = []
    pooled = [F.adaptive_avg_pool2d(f.permute(0, 3, 1, 2), 8) for f in feats]
    t = act(p["pos_emb"] + fr.swap_pack_ref(*pooled, x["gemb"], S))
    for i in range(n_layer):
        t = block16_ref(p, t, f"mambablocks.{i}.", probe, store)
    t = F.layer_norm(t, (C,), p["ln_f.weight"], p["ln_f.bias"], 1e-5)
    *maps, gps_out = fr.unpack_ref(t, S)
    outs = []
    for f, mp in zip(feats, maps):
        up = mp if H == 8 else F.interpolate(mp, scale_factor=H // 8, mode="bilinear", align_corners=False)
        outs.append(act(f + up.permute(0, 2, 3, 1)))
    loss = sum((o * d64[f"out{m}"].to(dtype)).sum() for m, o in enumerate(outs)) + (gps_out * d64["gps_out"].to(dtype)).sum()
    loss.backward()
    res = {f"out{m}": o.detach() for m, o in enumerate(outs)}
    res["gps_out"] = gps_out.detach()
    res.update({f"dfeat{m}": x[f"feat{m}"].grad for m in range(3)})
    res["dgemb"] = x["gemb"].grad
    res.update({k: p[k].grad for k in p})
    return res, fr.kink_margin(probe)
