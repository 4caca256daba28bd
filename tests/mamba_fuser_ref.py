"""Pure-torch, dtype-generic restatement of the reference's MambaFuser.forward (mambafuser_seq.py:393-597: EncoderWithMamba
followed by the join MLP), composed from pieces that are pinned on their own:

    the ResNet trunks, normalize_imagenet and join    oracle.fusion_ref (_stem, _layer, normalize_imagenet, join_forward)
    the four fusion stages                            tests/mamba_fusion_ref.fusion_ref
    the temporal head (config.TFM)                    tests/time_mamba_ref.time_mamba_ref
    F.adaptive_avg_pool2d, F.interpolate(bilinear)    torch

Run in fp64 it is the reference of the model tests, run in fp32 on the CPU it is their yardstick; in fp64 it is pinned to the
reference's own MambaFuser by tests/golden/make_golden_mambafuser.py.  Parameters and BatchNorm buffers are one flat dict
under the reference's state-dict names."""
import torch
import torch.nn.functional as F

from oracle import fusion_ref as fr
from tests import mamba_fusion_ref as mfr
from tests import time_mamba_ref as tmr

STAGE_WIDTH = fr.STAGE_WIDTH
KINK_MIN = mfr.KINK_MIN
MARGIN_MIN = tmr.MARGIN_MIN


def make_params(cfg, seed=0, stage_seeds=None):
    """fp64 state dict of a MambaFuser for cfg (an oracle.fusion_ref.RefConfig: seq_len, n_layer, add_velocity).  Trunks,
    vel_emb and join: oracle.fusion_ref.make_state without its encoder.transformer* entries.  Stages: the spread set of
    tests/mamba_fusion_ref (at the reference's initialisation a stage underflows to zero in fp32, and a relative error
    against zero checks nothing), stage s under seed stage_seeds[s - 1] (default 4 * seed + s): the LeakyReLU margin of a
    whole model is the minimum over about a million pre-activations, so a test case picks the seed of each stage in turn.
    Head: tests/time_mamba_ref.make_params."""
    sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in fr.make_state(cfg, seed=seed).items()
          if not k.startswith("encoder.transformer")}
    for s, C in enumerate(STAGE_WIDTH, start=1):
        sseed = 4 * seed + s if stage_seeds is None else stage_seeds[s - 1]
        p = mfr.make_fusion_params(C, cfg.seq_len, cfg.n_layer, seed=sseed, spread=True)
        sd.update({f"encoder.mambafusion{s}.{k}": v for k, v in p.items()})
    sd.update({f"encoder.time_mamba.{k}": v for k, v in tmr.make_params(seed).items()})
    return sd


def make_inputs(cfg, batch, seed=100):
    """-> (image_list, lidar_list, radar_list, gps, soft target): oracle.fusion_ref.make_inputs (fp32 values)"""
    return fr.make_inputs(cfg, batch, seed=seed)[:5]


def cast_state(sd, dtype, grad=True):
    """a copy of the state in `dtype`; the parameters (not the BatchNorm buffers) require grad"""
    out = {}
    for k, v in sd.items():
        if not v.is_floating_point():
            out[k] = v.clone()
        elif fr.is_buffer(k):
            out[k] = v.to(dtype).clone()
        else:
            out[k] = v.to(dtype).clone().requires_grad_(grad)
    return out


def _tokens(maps, gps_rows, B, S):
    """the stage's output tokens (B, T, C) back from its unpacked maps (B*S, C, 8, 8) and gps rows"""
    C = gps_rows.shape[2]
    return torch.cat([t.reshape(B, S, C, 64).permute(0, 1, 3, 2).reshape(B, S * 64, C) for t in maps] + [gps_rows], 1)


def encoder_forward(sd, image_list, lidar_list, radar_list, gps, cfg, tfm, ctx, probe=None):
    """EncoderWithMamba.forward (mambafuser_seq.py:393-550), n_views == 1, no missing modality -> fused (B, 512).
    probe (dict): receives "kink" (the LeakyReLU margin over all blocks of all stages) and, with tfm, "margin" (the temporal
    head's argmax margin)"""
    image_list = [fr.normalize_imagenet(x) for x in image_list]
    B, S = lidar_list[0].shape[0], cfg.seq_len
    assert len(image_list) == S and len(lidar_list) == S and len(radar_list) == S

    def stack(lst):  # frame index = b * S + t
        return torch.stack(lst, dim=1).reshape(B * len(lst), *lst[0].shape[1:])

    trunks = fr.trunk_prefixes()
    feats = [fr._stem(sd, p, f, ctx) for (p, _), f in zip(trunks, (stack(image_list), stack(lidar_list), stack(radar_list)))]
    ctx.tap("stem", feats)
    gps_tok, kink = gps, []
    for s in range(1, 5):
        feats = [fr._layer(sd, p, arch, s, f, ctx) for (p, arch), f in zip(trunks, feats)]
        ctx.tap(f"layer{s}", feats)
        emb = [F.adaptive_avg_pool2d(f, (8, 8)) for f in feats]
        gps_emb = F.linear(gps_tok, sd[f"encoder.vel_emb{s}.weight"], sd[f"encoder.vel_emb{s}.bias"])
        pre = f"encoder.mambafusion{s}."
        p = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        *outs, gps_tok = mfr.fusion_ref(p, cfg.n_layer, S, emb[0], emb[1], emb[2], gps_emb, probe=kink)
        ctx.tap(f"mamba{s}", _tokens(outs, gps_tok, B, S))
        scale = 8 // (2 ** (s - 1))
        if scale > 1:
            outs = [F.interpolate(o, scale_factor=scale, mode="bilinear") for o in outs]
        feats = [f + o for f, o in zip(feats, outs)]
        ctx.tap(f"fused{s}", feats)
    pooled = [f.mean(dim=(2, 3)).view(B, S, 512) for f in feats]
    tprobe = {}
    if tfm:
        pre = "encoder.time_mamba."
        fused = tmr.time_mamba_ref({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, *pooled, gps_tok,
                                   probe=tprobe)
    else:
        fused = torch.cat(pooled + [gps_tok], dim=1).sum(dim=1)
    ctx.tap("fused", fused)
    if probe is not None:
        probe["kink"] = mfr.kink_margin(kink)
        if tfm:
            probe["margin"] = tprobe["margin"]
    return fused


def mambafuser_forward(sd, image_list, lidar_list, radar_list, gps, cfg, tfm, ctx=None, probe=None):
    """MambaFuser.forward (mambafuser_seq.py:583-597) -> logits (B, 64)"""
    ctx = ctx or fr.Ctx()
    return fr.join_forward(sd, encoder_forward(sd, image_list, lidar_list, radar_list, gps, cfg, tfm, ctx, probe))


def focal_loss(logits, target, alpha=0.25, gamma=2.0):
    """torchvision.ops.sigmoid_focal_loss(reduction="mean") in the dtype of logits"""
    t = target.to(logits.dtype)
    p = torch.sigmoid(logits)
    ce = F.binary_cross_entropy_with_logits(logits, t, reduction="none")
    pt = p * t + (1 - p) * (1 - t)
    return ((alpha * t + (1 - alpha) * (1 - t)) * ce * (1 - pt) ** gamma).mean()


def train_run(sd64, inputs, cfg, tfm, dtype):
    """one training forward + backward of the restatement in `dtype` on the CPU ->
    dict(logits, loss, cap (taps), grads {name: gradient or None}, state (the run's state dict: BatchNorm buffers updated),
    kink, margin (None without tfm))"""
    imgs, lids, rads, gps, target = inputs
    sd = cast_state(sd64, dtype)
    cast = lambda seq: [t.to(dtype) for t in seq]   # noqa: E731
    cap, probe = {}, {}
    logits = mambafuser_forward(sd, cast(imgs), cast(lids), cast(rads), gps.to(dtype), cfg, tfm,
                                fr.Ctx(training=True, capture=cap), probe)
    loss = focal_loss(logits, target)
    loss.backward()
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point() and not fr.is_buffer(k)}
    detach = lambda v: [t.detach() for t in v] if isinstance(v, (list, tuple)) else v.detach()   # noqa: E731
    return dict(logits=logits.detach(), loss=loss.detach(), cap={k: detach(v) for k, v in cap.items()}, grads=grads, state=sd,
                kink=probe["kink"], margin=probe.get("margin"))


def eval_run(state, inputs, cfg, tfm, dtype):
    """eval-mode logits of the restatement on `state` (running statistics as they are there)"""
    imgs, lids, rads, gps, _ = inputs
    sd = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in state.items()}
    with torch.no_grad():
        return mambafuser_forward(sd, [t.to(dtype) for t in imgs], [t.to(dtype) for t in lids], [t.to(dtype) for t in rads],
                                  gps.to(dtype), cfg, tfm, fr.Ctx(training=False))
