"""f16 storage against bf16 storage in one process (GPU box): the bench configuration (full fusion, bs 12, n_layer 8, dropout
0.1, AdamW + EMA, one synthetic batch) timed in each mode, and the train-mode logit deviation of each mode against "f32" on
the same weights and inputs (dropout off for that comparison, so the three runs see identical masks).  f16 trains with the
dynamic loss scaler (train.DynamicLossScaler, default settings), bf16 without one.

    python tools/bench_f16.py [--steps 20] [--warmup 5] [--batch 12]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepsense6g_tii_amd import ops  # noqa: E402
from deepsense6g_tii_amd.model import GlobalConfig, TransFuser  # noqa: E402
from deepsense6g_tii_amd.synthetic import make_batch  # noqa: E402
from deepsense6g_tii_amd.train import EMA, DynamicLossScaler, FusedAdamW, train_iteration  # noqa: E402


def throughput(dev, mode, batch, steps, warmup):
    ops.set_compute_mode(mode)
    cfg = GlobalConfig()
    torch.manual_seed(100)
    model = TransFuser(cfg, dev)
    model.train()
    opt = FusedAdamW(model, lr=1e-4, ema_decay=0.999, loss_scaler=DynamicLossScaler() if mode == "f16" else None)
    ema = EMA(model, 0.999, opt)
    ema.register()
    data = make_batch(batch, cfg.seq_len, cfg.n_views, cfg.add_velocity, seed=100, device=dev)[:5]
    for _ in range(warmup):
        loss, _ = train_iteration(model, opt, data, ema)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss, _ = train_iteration(model, opt, data, ema)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = dict(samples_per_s=round(batch * steps / el, 1), ms_per_step=round(el / steps * 1e3, 2), loss=float(loss))
    if opt.loss_scaler is not None:
        out.update(loss_scale=opt.loss_scaler.get_scale(), applied_steps=opt.applied_steps(), iterations=warmup + steps)
    return out


def logits_by_mode(dev, batch):
    cfg = GlobalConfig(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    torch.manual_seed(100)
    sd = {k: v.detach().clone() for k, v in TransFuser(cfg, dev).state_dict().items()}
    data = make_batch(batch, cfg.seq_len, cfg.n_views, cfg.add_velocity, seed=100, device=dev)[:5]
    out = {}
    for mode in ("f32", "bf16", "f16"):
        ops.set_compute_mode(mode)
        model = TransFuser(cfg, dev)
        model.load_state_dict(sd)
        model.train()
        _, logits = model.train_step_loss(*data)
        out[mode] = logits.detach().double().cpu()
        del model
    ref = out["f32"]
    return {m: ((out[m] - ref).abs().max() / ref.abs().max()).item() for m in ("bf16", "f16")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=12)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    try:
        res = {m: throughput(dev, m, args.batch, args.steps, args.warmup) for m in ("bf16", "f16")}
        dev_ = logits_by_mode(dev, args.batch)
    finally:
        ops.set_compute_mode("f32")
    for m in res:
        res[m]["logits_max_dev_vs_f32_rel"] = float(f"{dev_[m]:.3e}")
    res["f16_over_bf16_samples_per_s"] = round(res["f16"]["samples_per_s"] / res["bf16"]["samples_per_s"], 4)
    res["config"] = (f"full fusion, bs {args.batch}, n_layer 8, dropout 0.1 (timed) / 0 (logit deviation), AdamW + EMA 0.999 "
                     f"(f16: + DynamicLossScaler), {args.steps} timed steps after {args.warmup} warm-up, eager train_iteration")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
