"""GPU tests of MambaFuser (deepsense6g_tii_amd/mamba_fuser.py): the reference's default model on the kernel walk.

Model parity, two cases - the smallest shapes at which the indexing can still go wrong:
    A  TFM = 0, seq_len = 1, n_layer = 2, B = 3, dropout 0   the four stages, an odd batch, the token-sum head at T = 194
    B  TFM = 1, seq_len = 5, n_layer = 1, B = 2, dropout 0   the temporal head, the strided gps rows, the sample stride
Reference: tests/mamba_fuser_ref.py in fp64 on the CPU; yardstick: the same restatement in fp32.  Forward taps, logits and loss
are held to the TOL of tests/test_model_gpu.py; the parameter gradients to that file's yardstick (median <= 3 x the fp32
restatement's median + 1e-4, worst <= max(3 x its worst, 0.05), none above 0.15), every compared fp64 tensor non-zero.  The
seeds (one per stage, tests/mamba_fuser_ref.make_params) were picked on the CPU so that the LeakyReLU margin and the temporal
head's argmax margin hold on the fp64 run; both are asserted.

Golden cross-check: the fixture's configuration (tests/golden/mambafuser_golden.npz: B = 1, seq_len 5, n_layer 1, both TFM
settings) on the HIP model against numbers that came out of the reference's own MambaFuser."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fusion_ref as fr
from tests import mamba_fuser_ref as mr
from tests.test_mamba_fuser_cpu import GOLD, golden_case
from tests.test_model_gpu import TOL, _host_threads, _nchw, rel

pytestmark = pytest.mark.gpu

F64 = torch.float64
# name: (TFM, seq_len, n_layer, B, parameter seed, the four stage seeds)
CASES = {"A": (0, 1, 2, 3, 1, (1014, 2024, 3011, 4092)),
         "B": (1, 5, 1, 2, 2, (1030, 2004, 3000, 10611))}


def _config(tfm, seq_len, n_layer, **kw):
    from deepsense6g_tii_amd.model import GlobalConfig
    return GlobalConfig(TFM=tfm, seq_len=seq_len, n_layer=n_layer, **{"embd_pdrop": 0.0, **kw})


def _build(dev, tfm, seq_len, n_layer, p64, **kw):
    from deepsense6g_tii_amd.mamba_fuser import MambaFuser
    model = MambaFuser(_config(tfm, seq_len, n_layer, **kw), dev)
    model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in p64.items()}, strict=True)
    assert model.params_in_arena()
    return model


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (cfg, fp64 parameters, inputs, fp64 run, fp32 run, fp64 eval logits) of the restatement on the CPU, computed once"""
    tfm, S, n_layer, B, seed, stage_seeds = CASES[name]
    torch.set_num_threads(_host_threads())
    cfg = fr.RefConfig(seq_len=S, n_layer=n_layer, embd_pdrop=0.0)
    p64 = mr.make_params(cfg, seed, stage_seeds)
    inputs = mr.make_inputs(cfg, B, seed=100 + seed)
    r64 = mr.train_run(p64, inputs, cfg, tfm, F64)
    r32 = mr.train_run(p64, inputs, cfg, tfm, torch.float32)
    return cfg, p64, inputs, r64, r32, mr.eval_run(r64["state"], inputs, cfg, tfm, F64)


@functools.lru_cache(maxsize=None)
def _hip(name):
    """one train_step_loss of the HIP model on the case, then an eval forward on the updated running statistics"""
    tfm, S, n_layer, B, _, _ = CASES[name]
    cfg, p64, inputs, *_ = _case(name)
    model = _build(torch.device("cuda:0"), tfm, S, n_layer, p64)
    model.train()
    cap = {}
    model._capture = cap
    loss, logits = model.train_step_loss(*inputs)
    model._capture = None
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().cpu().clone()) for n, p in model.named_parameters()}
    bufs = {n: b.detach().cpu().clone() for n, b in model.named_buffers()}
    model.eval()
    with torch.no_grad():
        logits_eval = model(*inputs[:4]).cpu()
    return dict(loss=loss.cpu(), logits=logits.cpu(), cap={k: v for k, v in cap.items()}, grads=grads, bufs=bufs,
                logits_eval=logits_eval)


@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_taps_logits_and_loss_match_the_fp64_restatement(name):
    tfm, S, n_layer, B, _, _ = CASES[name]
    cfg, p64, inputs, r64, r32, _ = _case(name)
    assert r64["kink"] >= mr.KINK_MIN, r64["kink"]
    assert not tfm or r64["margin"] >= mr.MARGIN_MIN, r64["margin"]
    h = _hip(name)
    report = []
    for tap in ["stem"] + [f"{k}{s}" for s in range(1, 5) for k in ("layer", "fused")]:
        for m in range(3):
            report.append((f"{tap}[{m}]", rel(_nchw(h["cap"][tap][m]), r64["cap"][tap][m])))
    for s in range(1, 5):
        tok = r64["cap"][f"mamba{s}"]
        report.append((f"mamba{s}", rel(h["cap"][f"mamba{s}"].view(tok.shape), tok)))
    report.append(("fused", rel(h["cap"]["fused"], r64["cap"]["fused"])))
    report.append(("logits", rel(h["logits"], r64["logits"])))
    report.append(("loss", abs(float(h["loss"]) - float(r64["loss"])) / abs(float(r64["loss"]))))
    msg = "\n".join(f"case {name} {k:12s} {v:.3e}" for k, v in report)
    print("\n" + msg)
    assert max(v for _, v in report) < TOL, msg


@pytest.mark.parametrize("name", ["A", "B"])
def test_parameter_gradients_match_the_fp64_restatement(name):
    tfm = CASES[name][0]
    cfg, p64, inputs, r64, r32, _ = _case(name)
    assert r64["kink"] >= mr.KINK_MIN and (not tfm or r64["margin"] >= mr.MARGIN_MIN)
    h = _hip(name)
    hip, o32 = [], []
    assert set(h["grads"]) == set(r64["grads"])
    for k, ref in r64["grads"].items():
        if ref is None:   # only the temporal head without TFM: no gradient - None or exactly zero, not NaN, not stale
            assert k.startswith("encoder.time_mamba.") and not tfm, k
            assert h["grads"][k] is None or bool((h["grads"][k] == 0).all()), k
            continue
        scale = ref.abs().max().item()
        assert scale > 0, k
        hip.append(((h["grads"][k].double() - ref).abs().max().item() / scale, k))
        o32.append(((r32["grads"][k].double() - ref).abs().max().item() / scale, k))
    hip.sort(reverse=True)
    o32.sort(reverse=True)
    med = lambda v: v[len(v) // 2][0]   # noqa: E731
    print("\ncase %s grad err vs fp64: HIP median %.3e max %.3e (%s) | restatement32 median %.3e max %.3e (%s)" %
          (name, med(hip), hip[0][0], hip[0][1], med(o32), o32[0][0], o32[0][1]), flush=True)
    print("worst five:", hip[:5])
    assert med(hip) < 3 * med(o32) + 1e-4
    assert hip[0][0] < max(3 * o32[0][0], 0.05), hip[:5]
    assert hip[0][0] < 0.15, hip[0]


@pytest.mark.parametrize("name", ["A", "B"])
def test_bn_running_statistics_and_eval_logits(name):
    cfg, p64, inputs, r64, r32, eval64 = _case(name)
    h = _hip(name)
    b = h["bufs"]
    assert int(b["encoder.radar_encoder._model.layer3.1.bn2.num_batches_tracked"]) == 1
    worst = 0.0
    for k, v in r64["state"].items():
        if k.endswith(("running_mean", "running_var")):
            worst = max(worst, rel(b[k], v))
    print(f"\ncase {name} running statistics worst {worst:.3e}, eval logits {rel(h['logits_eval'], eval64):.3e}")
    assert worst < 1e-3, worst
    assert rel(h["logits_eval"], eval64) < TOL


# per-tensor bars of the golden cross-check, (head error / absmax, l2 error) per TFM setting: 10 x what was measured on an
# MI355X, rounded up to one digit, never below 1e-6 (10 x the fp32 rounding of an entry).  Measured, head / norm (all of them in
# profiles/mamba_fuser_parity.txt) - TFM on: join.4.bias 1.5e-6 / 4e-8, time_mamba.mlp.0.weight 3.4e-6 / 1.7e-6,
# mambafusion4 A_log 1.9e-6 / 3.5e-6, mambafusion3 fc2 1.2e-4 / 3.6e-6, mambafusion1.pos_emb 6.6e-5 / 3.5e-5, vel_emb1 1.6e-4 /
# 9e-5, camera stem conv1 8.8e-4 / 2.6e-5; TFM off: join.4.bias 6e-7 / 1.4e-7, mambafusion3 fc2 9.7e-4 / 9e-5, mambafusion2
# conv1d 2.9e-3 / 3.3e-4, vel_emb1 1.8e-3 / 2.4e-4, camera stem conv1 3.9e-3 / 1.4e-5.  The deeper a tensor sits below ReLU /
# max-pool decisions the larger single entries move (about ten times more with the token-sum head than with the temporal one).
GOLD_BARS = {
    "tfm1": {
        "join.4.bias": (2e-05, 1e-06),
        "join.0.weight": (6e-06, 4e-06),
        "encoder.time_mamba.mamba.in_proj.weight": (1e-06, 4e-06),
        "encoder.time_mamba.mlp.0.weight": (4e-05, 2e-05),
        "encoder.vel_emb4.weight": (4e-06, 1e-05),
        "encoder.mambafusion4.ln_f.weight": (6e-05, 6e-06),
        "encoder.mambafusion4.mambablocks.0.forward_mamba.A_log": (2e-05, 4e-05),
        "encoder.radar_encoder._model.layer4.1.bn2.weight": (2e-06, 3e-06),
        "encoder.mambafusion3.mambablocks.0.fc2.weight": (0.002, 4e-05),
        "encoder.mambafusion2.mambablocks.0.backward_mamba.conv1d.weight": (0.003, 0.0004),
        "encoder.lidar_encoder._model.layer2.0.downsample.0.weight": (0.002, 0.0002),
        "encoder.mambafusion1.pos_emb": (0.0007, 0.0004),
        "encoder.vel_emb1.weight": (0.002, 0.0009),
        "encoder.image_encoder.features.conv1.weight": (0.009, 0.0003),
    },
    "tfm0": {
        "join.4.bias": (7e-06, 2e-06),
        "join.0.weight": (1e-06, 2e-06),
        "encoder.vel_emb4.weight": (5e-06, 6e-06),
        "encoder.mambafusion4.ln_f.weight": (6e-06, 1e-06),
        "encoder.mambafusion4.mambablocks.0.forward_mamba.A_log": (6e-06, 6e-06),
        "encoder.radar_encoder._model.layer4.1.bn2.weight": (2e-05, 3e-06),
        "encoder.mambafusion3.mambablocks.0.fc2.weight": (0.01, 0.001),
        "encoder.mambafusion2.mambablocks.0.backward_mamba.conv1d.weight": (0.03, 0.004),
        "encoder.lidar_encoder._model.layer2.0.downsample.0.weight": (0.03, 0.002),
        "encoder.mambafusion1.pos_emb": (0.007, 0.0006),
        "encoder.vel_emb1.weight": (0.02, 0.003),
        "encoder.image_encoder.features.conv1.weight": (0.04, 0.0002),
    },
}


@pytest.mark.parametrize("tfm", [1, 0])
def test_golden_configuration_matches_the_reference_fixture(dev, tfm):
    gold = np.load(GOLD)
    cfg, p64, inputs = golden_case()
    model = _build(dev, tfm, cfg.seq_len, cfg.n_layer, p64)
    model.train()
    loss, logits = model.train_step_loss(*inputs)
    tag = f"tfm{tfm}"
    e_logits = rel(logits, gold[f"{tag}:logits"])
    print(f"\ngolden {tag} logits {e_logits:.3e} loss {float(loss):.8f} vs {float(gold[f'{tag}:loss']):.8f}")
    assert e_logits < TOL
    assert abs(float(loss) - float(gold[f"{tag}:loss"])) < TOL * float(gold[f"{tag}:loss"])
    named = dict(model.named_parameters())
    bad = []
    for key in gold.files:
        if key.startswith(f"{tag}:grad:") and key.endswith(":head"):
            k = key[len(tag) + 6:-len(":head")]
            g = named[k].grad.cpu()
            scale = float(gold[f"{tag}:grad:{k}:absmax"])
            e_head = (g.flatten()[:16].double() - torch.from_numpy(gold[key])).abs().max().item() / scale
            e_norm = abs(float(g.double().norm()) - float(gold[f"{tag}:grad:{k}:l2"])) / float(gold[f"{tag}:grad:{k}:l2"])
            print(f"golden {tag} {k:70s} head {e_head:.2e} of the largest entry, norm {e_norm:.2e}", flush=True)
            bar_head, bar_norm = GOLD_BARS[tag][k]
            if not (e_head < bar_head and e_norm < bar_norm):
                bad.append((k, e_head, e_norm))
    assert not bad, bad


# ---- behaviour ----------------------------------------------------------------------------------------------------------------
def _small(dev, tfm=0, seed=1, B=1, **kw):
    S = 5 if tfm else 1
    cfg = fr.RefConfig(seq_len=S, n_layer=1, embd_pdrop=0.0)
    p64 = mr.make_params(cfg, seed)
    return _build(dev, tfm, S, 1, p64, **kw), p64, mr.make_inputs(cfg, B, seed=100 + seed)


@pytest.mark.parametrize("tfm", [0, 1])
def test_autograd_boundary_and_grad_accumulation(dev, tfm):
    from oracle import train_ref as tr
    model, p64, inputs = _small(dev, tfm)
    imgs, lids, rads, gps, target = inputs
    model.train()
    loss1, _ = model.train_step_loss(*inputs)
    g1 = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    logits = model(imgs, lids, rads, gps)
    loss2 = tr.sigmoid_focal_loss(logits, target.to(dev))
    loss2.backward()
    assert abs(float(loss1) - float(loss2.detach())) < 1e-5
    for n, p in model.named_parameters():
        assert (p.grad - g1[n]).abs().max().item() <= 1e-4 * g1[n].abs().max().item() + 1e-9, n
    logits = model(imgs, lids, rads, gps)     # no zero_grad: the second backward accumulates
    tr.sigmoid_focal_loss(logits, target.to(dev)).backward()
    for n in ("join.4.weight", "encoder.mambafusion2.mambablocks.0.forward_mamba.A_log", "encoder.mambafusion4.pos_emb",
              "encoder.mambafusion1.mambablocks.0.backward_mamba.conv1d.weight", "encoder.mambafusion3.ln_f.bias",
              "encoder.vel_emb2.weight", "encoder.lidar_encoder._model.conv1.weight", "encoder.time_mamba.mlp.0.weight",
              "encoder.time_mamba.mamba.dt_proj.bias"):
        p = dict(model.named_parameters())[n]
        if not tfm and n.startswith("encoder.time_mamba."):
            assert bool((p.grad == 0).all()), n
        else:
            assert g1[n].abs().max().item() > 0 and rel(p.grad, 2 * g1[n]) < 2e-3, n


def test_embedding_dropout_is_seeded_and_eval_ignores_the_seed(dev):
    model, p64, inputs = _small(dev, 0, B=2, embd_pdrop=0.1)
    model.train()

    def run(seed):
        model.set_dropout_seed(seed)
        model.set_rng_state(dict(seed=seed, counter=0))
        model.zero_grad(set_to_none=True)
        _, logits = model.train_step_loss(*inputs)
        return logits.clone(), model.encoder.mambafusion1.pos_emb.grad.clone()

    a, b, c = run(11), run(11), run(12)
    assert torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    model.eval()
    with torch.no_grad():
        model.set_dropout_seed(11)
        e1 = model(*inputs[:4]).clone()
        model.set_dropout_seed(12)
        e2 = model(*inputs[:4]).clone()
    assert torch.equal(e1, e2) and not torch.equal(e1, a[0])


def test_two_training_iterations_with_the_fused_optimizer_and_ema(dev):
    from deepsense6g_tii_amd.train import EMA, FusedAdamW, train_iteration
    tfm, S, n_layer, B, seed, stage_seeds = CASES["A"]
    cfg = fr.RefConfig(seq_len=S, n_layer=n_layer, embd_pdrop=0.0)
    p64 = mr.make_params(cfg, seed, stage_seeds)
    inputs = mr.make_inputs(cfg, B, seed=100 + seed)
    model = _build(dev, tfm, S, n_layer, p64)
    model.train()
    opt = FusedAdamW(model, lr=1e-3, weight_decay=0.0, ema_decay=0.999)
    ema = EMA(model, 0.999, opt)
    ema.register()
    before = model.flat_parameters()[0].clone()
    for _ in range(2):
        loss, logits = train_iteration(model, opt, inputs, ema)
        assert torch.isfinite(loss).all() and torch.isfinite(logits).all()
    torch.cuda.synchronize()
    assert model.params_in_arena()
    after = model.flat_parameters()[0]
    for n, p in model.named_parameters():
        off, cnt = model._pslice[n]
        moved = bool((after[off:off + cnt] != before[off:off + cnt]).any())
        nonzero = bool((p.grad != 0).any())
        if n.startswith("encoder.time_mamba."):
            assert not nonzero and not moved, n            # TFM is off: exactly zero gradient, no weight decay
        elif nonzero:
            assert moved, n
    ema.apply_shadow()
    assert not model.params_in_arena()
    model.eval()
    with torch.no_grad():
        shadow_logits = model(*inputs[:4])                 # the walk reads the re-pointed parameters
    assert torch.isfinite(shadow_logits).all()
    ema.restore()
    assert model.params_in_arena()
    with torch.no_grad():
        assert not torch.equal(model(*inputs[:4]), shadow_logits)


def test_grad_ready_hook_announces_final_ranges_in_order(dev):
    model, p64, inputs = _small(dev, 1)
    model.train()
    garena = model.flat_parameters()[1]
    seen = []
    model.grad_ready_hook = lambda k, lo, hi: seen.append((k, lo, hi, garena[lo:hi].clone()))
    model.train_step_loss(*inputs)
    model.grad_ready_hook = None
    torch.cuda.synchronize()
    assert [k for k, *_ in seen] == list(range(10))
    assert seen[0][1] == 0 and seen[-1][2] == model._arena_used
    assert all(a[2] == b[1] for a, b in zip(seen, seen[1:]))
    for k, lo, hi, snap in seen:
        assert torch.equal(snap, garena[lo:hi]), k         # a range announced as final is final
    lo1, hi1 = seen[1][1], seen[1][2]
    off, cnt = model._pslice["encoder.time_mamba.mlp.0.weight"]
    assert lo1 <= off and off + cnt <= hi1 and bool((garena[off:off + cnt] != 0).any())


def test_graph_capture_and_the_frozen_engine_are_refused(dev):
    from deepsense6g_tii_amd.train import CapturedTrainStep, FusedAdamW
    model, p64, inputs = _small(dev, 0)
    opt = FusedAdamW(model, lr=1e-3)
    with pytest.raises(NotImplementedError):
        CapturedTrainStep(model, opt, inputs)
    model.eval()
    with pytest.raises(NotImplementedError):
        model.freeze_inference()
    with pytest.raises(NotImplementedError):
        model.capture_inference(*inputs[:4])
