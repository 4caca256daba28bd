"""Pure-torch, dtype-generic restatement of the reference's temporal Mamba fusion head (TimeMamba, mambafuser_seq.py:233-284)
over tests/mamba_ref.mamba_ref, written from the head's definition.  Run in fp64 it is the reference of the TimeMamba tests,
run in fp32 on the CPU it is their yardstick; in fp64 it is pinned to the reference's own TimeMamba by
tests/golden/make_golden_timemamba.py.

    y_m = mamba(x_m) for image, lidar, radar (B, 5, 512), one shared layer - pushed through it here as ONE (3 B, 5, 512) batch
    s[r] = max_c row[r][c] + mean_c row[r][c]   for the rows of y_m and of gps (B, 2, 512)
    a_m = softmax(mlp.0(s_m)) over 5 frames,  a_g = softmax(mlp_gps.0(s_g)) over 2 rows
    out = sum_m sum_t a_m[t] y_m[t] + sum_j a_g[j] gps[j]
Per-sample tensors of the head are laid out [B][17]: row 5 m + t for modality m = image, lidar, radar and frame t, then the two
gps rows.  Parameters are a flat dict under the reference's state-dict names."""
import torch
import torch.nn.functional as F

from tests import mamba_ref as mr

C = 512
S = 5
ROWS = 17
HEAD_NAMES = ("mlp.0.weight", "mlp.0.bias", "mlp_gps.0.weight", "mlp_gps.0.bias")
NAMES = tuple(f"mamba.{k}" for k in mr.NAMES) + HEAD_NAMES
IN_KEYS = ("image", "lidar", "radar", "gps")
MARGIN_MIN = 1e-4        # (top1 - top2) / max|row| of every row, on the fp64 run: about 100x the fp32 error of y

# (B, parameter seed, input seed) of the module-level cases: B = 1, and an odd count that is no power of two.  The seeds were
# picked on the CPU for an argmax margin >= 1e-3 (tests/golden/README_timemamba.md lists the margins)
CASES = [(1, 0, 0), (3, 3, 3)]


def shapes():
    s = {f"mamba.{k}": v for k, v in mr.shapes(C).items()}
    s.update({"mlp.0.weight": (S, S), "mlp.0.bias": (S,), "mlp_gps.0.weight": (2, 2), "mlp_gps.0.bias": (2,)})
    return s


def make_head_params(seed=0):
    """fp64 mlp / mlp_gps parameters with torch's nn.Linear initialisation bounds: U(+-fan_in^-1/2) for weight and bias"""
    g = torch.Generator().manual_seed(9000 + seed)
    return {"mlp.0.weight": mr._uniform(g, (S, S), S ** -0.5), "mlp.0.bias": mr._uniform(g, (S,), S ** -0.5),
            "mlp_gps.0.weight": mr._uniform(g, (2, 2), 2 ** -0.5), "mlp_gps.0.bias": mr._uniform(g, (2,), 2 ** -0.5)}


def make_params(seed=0):
    """fp64 parameter dict under the reference's 13 names: the Mamba layer's own initialisation (mr.make_params) and torch's
    for the two small linears - what the reference constructs, since it applies no _init_weights to this module"""
    p = {f"mamba.{k}": v for k, v in mr.make_params(C, seed=seed).items()}
    p.update(make_head_params(seed))
    return p


def make_inputs(B, seed=0):
    """-> ({image, lidar, radar (B, 5, 512), gps (B, 2, 512)}, dout (B, 512)), fp64 randn"""
    g = torch.Generator().manual_seed(9500 + seed)
    ins = {k: torch.randn(B, S, C, generator=g, dtype=torch.float64) for k in IN_KEYS[:3]}
    ins["gps"] = torch.randn(B, 2, C, generator=g, dtype=torch.float64)
    return ins, torch.randn(B, C, generator=g, dtype=torch.float64)


def _pool_score(x):
    """(N, L, 512) -> (N, L): the reference's MaxPool1d(512) + AvgPool1d(512)"""
    return (F.max_pool1d(x, C) + F.avg_pool1d(x, C)).squeeze(-1)


def per_sample(t3, tg):
    """(3 B, 5, ...) of the modality-major batch and (B, 2, ...) of gps -> (B, 17, ...)"""
    B = tg.shape[0]
    return torch.cat([t3.reshape(3, B, S, *t3.shape[2:]).transpose(0, 1).reshape(B, 3 * S, *t3.shape[2:]), tg], 1)


def row_margin(y, gps):
    """min over all 17 rows of every sample of (top1 - top2) / max|row|"""
    rows = per_sample(y, gps)
    top = rows.topk(2, dim=-1).values
    return float(((top[..., 0] - top[..., 1]) / rows.abs().amax(-1)).min())


def head_ref(p, y, gps, probe=None):
    """everything behind the layer: y (3 B, 5, 512) modality-major, gps (B, 2, 512) -> out (B, 512).
    probe (dict): receives score, attn (B, 17), argmax (B, 17; lowest channel of the maximum) and the argmax margin"""
    B = gps.shape[0]
    s, sg = _pool_score(y), _pool_score(gps)
    a = torch.softmax(s @ p["mlp.0.weight"].t() + p["mlp.0.bias"], -1)
    ag = torch.softmax(sg @ p["mlp_gps.0.weight"].t() + p["mlp_gps.0.bias"], -1)
    feat = (y * a.unsqueeze(-1)).sum(1).reshape(3, B, C)
    gfeat = (gps * ag.unsqueeze(-1)).sum(1)
    if probe is not None:
        rows = per_sample(y, gps).detach()
        probe.update(score=per_sample(s, sg).detach(), attn=per_sample(a, ag).detach(),
                     argmax=(rows == rows.amax(-1, keepdim=True)).int().argmax(-1).to(torch.int32),
                     margin=row_margin(y.detach(), gps.detach()))
    return feat[0] + feat[1] + feat[2] + gfeat


def time_mamba_ref(p, image, lidar, radar, gps, probe=None):
    mp = {k: p[f"mamba.{k}"] for k in mr.NAMES}
    return head_ref(p, mr.mamba_ref(mp, torch.cat([image, lidar, radar], 0)), gps, probe)


def head_run(p64, y64, gps64, dout64, dtype):
    """-> {out, attn, score, argmax, dy, dgps, the four head parameter gradients}, margin: the head alone on given rows"""
    p = {k: p64[k].to(dtype).clone().requires_grad_(True) for k in HEAD_NAMES}
    y, gps = (t.to(dtype).clone().requires_grad_(True) for t in (y64, gps64))
    probe = {}
    out = head_ref(p, y, gps, probe)
    (out * dout64.to(dtype)).sum().backward()
    res = {"out": out.detach(), "attn": probe["attn"], "score": probe["score"], "argmax": probe["argmax"],
           "dy": y.grad.reshape(-1, C), "dgps": gps.grad}
    res.update({k: p[k].grad for k in HEAD_NAMES})
    return res, probe["margin"]


def time_run(p64, ins64, dout64, dtype):
    """-> {out, dimage, dlidar, dradar, dgps, the 13 parameter gradients of sum(out * dout)}, margin; computed in `dtype`"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    ins = {k: v.to(dtype).clone().requires_grad_(True) for k, v in ins64.items()}
    probe = {}
    out = time_mamba_ref(p, *(ins[k] for k in IN_KEYS), probe=probe)
    (out * dout64.to(dtype)).sum().backward()
    res = {"out": out.detach()}
    res.update({"d" + k: ins[k].grad for k in IN_KEYS})
    res.update({k: p[k].grad for k in NAMES})
    return res, probe["margin"]
