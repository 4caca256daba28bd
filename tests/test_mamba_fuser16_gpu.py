"""GPU tests of MambaFuser in compute modes "bf16" and "f16" (deepsense6g_tii_amd/mamba_fuser.py on 16-bit storage), on cases A
and B of tests/test_mamba_fuser_gpu.py - the smallest shapes at which the indexing can go wrong, with seeds that hold the
LeakyReLU and argmax margins.

  1  the 16-bit path is the one that ran, and mode "f32" is bit for bit what it was before and after a 16-bit step
  2  the trunks are TransFuser's: stem and layer1 taps equal a TransFuser's in the same mode, bit for bit
  3  the stage wiring: every stage and (TFM) the head of the model's step replayed through mamba_fusion.stage_forward /
     stage_backward (w16=None: the stage's own casts), ops.pool_rows3_* and time_mamba_forward / _backward called directly -
     outputs, tokens, data gradients and every parameter gradient bit-identical.  This pins the shadow-sourced weights, the
     dtype plumbing and the arena destinations.
  4  end to end against fp64.  The yardstick is not the code under test: tests/mamba_fuser_ref.train_run(..., fp32) under
     torch.autocast("cpu", dtype) (tests/mamba_fuser16_yard.py), both measured against the same restatement in fp64; margins of
     tests/test_bf16_gpu.py: logits e_hip < 2 e_ac + 2e-3, gradient L2-relative median < 1.5 med_ac + 0.02, worst < 2 worst_ac,
     share of tensors with cosine > 0.9 >= share_ac - 0.05.  bf16: the yardstick is computed live, and it is coarse (logits
     2e-2 .. 6e-2, gradient median 0.4 .. 0.6, cosine share 0.5 / 0.2): on bf16 this check only excludes gross errors.  The
     discriminating power is in items 2 and 3 and in the f16 run, whose yardstick takes minutes on a CPU and is therefore
     recorded: F16_FLOOR below, from tools/mamba_fuser16_floor.py (profiles/mamba_fuser16_floor.txt).
  5  training: the loss falls in fp32 (checked here, on the parent's path) and then in each 16-bit mode, f16 under the dynamic
     loss scaler; mode switches between steps; eval() logits against the fp64 eval logits
  6  what stays refused
The figures are printed (pytest -s); the committed copy is profiles/mamba_fuser16_parity.txt."""
import functools

import pytest
import torch

from tests import mamba_fuser16_yard as yard
from tests import mamba_fuser_ref as mr
from tests.test_mamba_fuser_gpu import CASES, _build, _case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
MODE = {F32: "f32", BF16: "bf16", F16: "f16"}
_name = MODE.get

# tools/mamba_fuser16_floor.py on the CPU (torch.autocast("cpu", torch.float16) against the fp64 restatement), the rows
# "f16 A" and "f16 B" of profiles/mamba_fuser16_floor.txt: logits / eval = max-norm relative error of the train / eval logits,
# med / worst = per-tensor L2-relative gradient error, cos = share of tensors with cosine > 0.9
F16_FLOOR = {
    "A": dict(logits=4.078e-03, med=1.702e-01, worst=1.071e+00, cos=0.975, eval=7.920e-04),
    "B": dict(logits=9.427e-03, med=2.585e-01, worst=1.139e+00, cos=0.961, eval=3.086e-03),
}


@pytest.fixture(autouse=True)
def _f32_mode_after_each_test():
    yield
    from deepsense6g_tii_amd import ops
    ops.set_compute_mode("f32")


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


def _model(name):
    tfm, S, n_layer, B, _, _ = CASES[name]
    cfg, p64, inputs, *_ = _case(name)
    return _build(torch.device(DEV), tfm, S, n_layer, p64), p64, inputs


def _reset(model, p64):
    """the case's parameters and the initial BatchNorm buffers again"""
    model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in p64.items()}, strict=True)
    assert model.params_in_arena()


def _step(model, inputs, mode, scaled=False):
    """one train_step_loss in `mode` -> dict(tape, cap, logits, loss, grads (unscaled, on the CPU))"""
    from deepsense6g_tii_amd.train import DynamicLossScaler
    _ops().set_compute_mode(mode)
    model.train()
    model.zero_grad(set_to_none=True)
    tapes, run_backward = [], model._run_backward
    model._run_backward = lambda tape, dlogits: (tapes.append(tape), run_backward(tape, dlogits))
    cap = {}
    model._capture = cap
    scaler = DynamicLossScaler().bind(model.device, model.flat_parameters()[0].numel()) if scaled else None
    try:
        loss, logits = model.train_step_loss(*inputs, loss_scaler=scaler)
        torch.cuda.synchronize()
    finally:
        model._capture = None
        del model._run_backward
    scale = scaler.get_scale() if scaled else 1.0
    grads = {n: (None if p.grad is None else p.grad.detach().cpu() / scale) for n, p in model.named_parameters()}
    return dict(tape=tapes[0], cap=cap, logits=logits.detach().cpu().clone(), loss=loss.detach().cpu().clone(), grads=grads,
                scale=scale)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_the_16bit_path_ran_and_f32_is_bit_for_bit_unchanged(dtype, name):
    n_layer = CASES[name][2]
    model, p64, inputs = _model(name)
    a = _step(model, inputs, "f32")
    assert a["tape"].walk.dtype == F32 and all(r.copies is None for r in a["tape"].stages)
    _reset(model, p64)
    b = _step(model, inputs, MODE[dtype], scaled=dtype == F16)
    tape, cap = b["tape"], b["cap"]
    assert tape.walk.dtype == dtype, "the 16-bit walk must be the one that ran"
    assert tape.head.fdtype == dtype
    for s in range(1, 5):
        rec = tape.stages[s - 1]
        assert rec.tape[-1][0] == dtype                              # the stage tape's storage
        assert rec.tape[0][0][0].dtype == dtype                      # the first block's input tokens
        assert all(t.dtype == dtype for t in cap[f"layer{s}"]) and all(t.dtype == dtype for t in cap[f"fused{s}"])
        assert cap[f"mamba{s}"].dtype == F32                         # xo
        # stage 1 (C = 64): the two x_proj weights of each block are zero-padded copies, everything else reads the shadow
        assert model.w16_routes[s] == ((6 * n_layer, 2 * n_layer) if s == 1 else (8 * n_layer, 0)), model.w16_routes
        assert len(rec.copies) == (2 * n_layer if s == 1 else 0)
    assert cap["fused"].dtype == F32 and b["logits"].dtype == F32
    assert torch.isfinite(b["logits"]).all() and not torch.equal(a["logits"], b["logits"])
    _reset(model, p64)
    c = _step(model, inputs, "f32")
    assert torch.equal(a["logits"], c["logits"]) and torch.equal(a["loss"], c["loss"])
    for k, g in a["grads"].items():
        assert torch.equal(g, c["grads"][k]), k


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_trunks_are_the_parents(dtype, name):
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
    S = CASES[name][1]
    model, p64, inputs = _model(name)
    trunk = ("encoder.image_encoder.", "encoder.lidar_encoder.", "encoder.radar_encoder.")
    tf = TransFuser(GlobalConfig(seq_len=S, n_layer=1, embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0), torch.device(DEV))
    sub = {k: (v.float() if v.is_floating_point() else v) for k, v in p64.items() if k.startswith(trunk)}
    assert sub and {k for k in tf.state_dict() if k.startswith(trunk)} == set(sub)
    res = tf.load_state_dict(sub, strict=False)
    assert not res.unexpected_keys and tf.params_in_arena()
    a = _step(model, inputs, MODE[dtype], scaled=dtype == F16)
    b = _step(tf, inputs, MODE[dtype], scaled=dtype == F16)
    assert a["tape"].walk.dtype == b["tape"].walk.dtype == dtype
    for tap in ("stem", "layer1"):
        for m in range(3):
            assert a["cap"][tap][m].dtype == b["cap"][tap][m].dtype
            assert torch.equal(a["cap"][tap][m], b["cap"][tap][m]), (tap, m)
    assert a["cap"]["layer1"][0].dtype == dtype


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def _record_calls(model, monkeypatch):
    """wrap the model's stage and head methods on the instance, and the stage functions they call, to keep their arguments
    and results"""
    from deepsense6g_tii_amd import mamba_fusion
    calls = dict(fwd=[], bwd=[], sf=[], sb=[], hf=[], hb=[])
    stage_fwd, stage_bwd, head_fwd, head_bwd = model._stage_fwd, model._stage_bwd, model._head_fwd, model._head_bwd
    sf, sb = mamba_fusion.stage_forward, mamba_fusion.stage_backward

    def rec_sf(fus, ws, save, feats, gemb, outs, B, drop=(0.0, 0, 0), w=None, w16=None):
        calls["sf"].append(dict(gemb=gemb.clone(), drop=drop, w16=w16, w=w))
        return sf(fus, ws, save, feats, gemb, outs, B, drop=drop, w=w, w16=w16)

    def rec_sb(fus, ws, tape, dfeats_out, dgps_tok, dfeats, dgemb, B, g, w=None):
        sb(fus, ws, tape, dfeats_out, dgps_tok, dfeats, dgemb, B, g, w=w)
        calls["sb"].append(dict(dgemb=dgemb.clone()))
    monkeypatch.setattr(mamba_fusion, "stage_forward", rec_sf)
    monkeypatch.setattr(mamba_fusion, "stage_backward", rec_sb)

    def fwd(wk, s, feats, gps_src, B):
        ins = [t.clone() for t in feats]
        outs, xo, rec = stage_fwd(wk, s, feats, gps_src, B)
        calls["fwd"].append(dict(s=s, feats=ins, outs=[t.clone() for t in outs], xo=xo.clone(), B=B))
        return outs, xo, rec

    def bwd(wk, rec, dfeats_out, dgps_tok, B):
        douts, dgps = [t.clone() for t in dfeats_out], (dgps_tok[0].clone(), dgps_tok[1])
        dfeats, dprev = stage_bwd(wk, rec, dfeats_out, dgps_tok, B)
        calls["bwd"].append(dict(s=rec.s, dfeats_out=douts, dgps_tok=dgps, dfeats=[t.clone() for t in dfeats]))
        return dfeats, dprev

    def hfwd(wk, feats, xo, B, T):
        ins = [t.clone() for t in feats]
        fused, hook = head_fwd(wk, feats, xo, B, T)
        calls["hf"].append(dict(feats=ins, xo=xo.clone(), fused=fused.clone(), T=T))
        return fused, hook

    def hbwd(wk, head, dfused, B):
        d = dfused.clone()
        dfeats, dgps = head_bwd(wk, head, dfused, B)
        calls["hb"].append(dict(dfused=d, dfeats=[t.clone() for t in dfeats], dgps=dgps[0].clone()))
        return dfeats, dgps
    model._stage_fwd, model._stage_bwd, model._head_fwd, model._head_bwd = fwd, bwd, hfwd, hbwd
    return calls


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_stage_and_head_wiring_against_the_stage_code_called_directly(dtype, name, monkeypatch):
    from deepsense6g_tii_amd import mamba_fusion
    from deepsense6g_tii_amd.time_mamba import time_mamba_backward, time_mamba_forward
    ops = _ops()
    tfm = CASES[name][0]
    model, p64, inputs = _model(name)
    stage_forward, stage_backward = mamba_fusion.stage_forward, mamba_fusion.stage_backward   # the unwrapped ones
    calls = _record_calls(model, monkeypatch)
    try:
        _step(model, inputs, MODE[dtype], scaled=dtype == F16)
    finally:
        for k in ("_stage_fwd", "_stage_bwd", "_head_fwd", "_head_bwd"):
            delattr(model, k)
    assert [c["s"] for c in calls["fwd"]] == [1, 2, 3, 4] and [c["s"] for c in calls["bwd"]] == [4, 3, 2, 1]
    garena = model.flat_parameters()[1]
    scratch = torch.full_like(garena, float("nan"))
    names = {id(p): n for n, p in model._plist}

    def g(p):        # a scratch gradient table with the arena's layout, written fresh
        return scratch.data_ptr() + 4 * model._pslice[names[id(p)]][0], 0
    for i, c in enumerate(calls["fwd"]):
        s, B = c["s"], c["B"]
        fus = getattr(model.encoder, f"mambafusion{s}")
        sfc, bwc, sbc = calls["sf"][i], calls["bwd"][4 - s], calls["sb"][4 - s]
        assert sfc["w16"] is not None and len(sfc["w16"]) == len(fus.mambablocks) and sfc["w"] is None
        assert all(t.dtype == dtype for t in c["feats"]) and sfc["gemb"].dtype == F32
        ws = model._mamba_ws(mamba_fusion.stage_workspace_bytes(fus, B))
        outs = [torch.full_like(t, float("nan")) for t in c["feats"]]
        xo, tape = stage_forward(fus, ws, True, c["feats"], sfc["gemb"], outs, B, drop=sfc["drop"], w16=None)
        assert tape[-1][2] is not None, "the direct call must have cast its own weights"
        assert xo.dtype == F32 and torch.equal(xo, c["xo"]), s
        for m in range(3):
            assert outs[m].dtype == dtype and torch.equal(outs[m], c["outs"][m]), (s, m)
        dfeats = [torch.full_like(t, float("nan")) for t in c["feats"]]
        dgemb = torch.full_like(sfc["gemb"], float("nan"))
        stage_backward(fus, ws, tape, bwc["dfeats_out"], bwc["dgps_tok"], dfeats, dgemb, B, g)
        torch.cuda.synchronize()
        for m in range(3):
            assert dfeats[m].dtype == dtype and torch.equal(dfeats[m], bwc["dfeats"][m]), (s, m)
        assert torch.equal(dgemb, sbc["dgemb"]), s
        checked = 0
        for n, p in model._plist:
            if n.startswith(f"encoder.mambafusion{s}."):
                off, cnt = model._pslice[n]
                assert torch.isfinite(scratch[off:off + cnt]).all(), n
                assert torch.equal(scratch[off:off + cnt], garena[off:off + cnt]), n
                checked += 1
        assert checked == 3 + 24 * len(fus.mambablocks)
    if not tfm:
        return
    # the head: ops.pool_rows3_* and the fp32 temporal head called directly
    hf, hb = calls["hf"][0], calls["hb"][0]
    tm = model.encoder.time_mamba
    B, T = calls["fwd"][0]["B"], hf["T"]
    assert all(t.dtype == dtype for t in hf["feats"]) and hf["fused"].dtype == F32
    rows = torch.full((3 * B * 5, 512), float("nan"), dtype=F32, device=DEV)
    ops.pool_rows3_fwd(hf["feats"], rows)
    gps = hf["xo"].view(-1)[(T - 2) * 512:]
    ws = model._mamba_ws(tm.mamba.workspace_bytes(3 * B, 5))
    fused, tape = time_mamba_forward(tm, ws, True, rows, gps, T * 512, B)
    assert torch.equal(fused, hf["fused"])
    drows, dgps, _ = time_mamba_backward(tm, ws, tape, hb["dfused"], gps, T * 512, B, gdst=[g(p) for p in tm._params()])
    dfeats = [torch.full_like(t, float("nan")) for t in hf["feats"]]
    ops.pool_rows3_bwd(drows, None, dfeats)
    torch.cuda.synchronize()
    assert torch.equal(dgps, hb["dgps"])
    for m in range(3):
        assert dfeats[m].dtype == dtype and torch.equal(dfeats[m], hb["dfeats"][m]), m
    for n, p in model._plist:
        if n.startswith("encoder.time_mamba."):
            off, cnt = model._pslice[n]
            assert torch.equal(scratch[off:off + cnt], garena[off:off + cnt]), n


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _floor(name, dtype):
    """the autocast yardstick of the case: bf16 computed here (seconds), f16 the recorded one"""
    if dtype == F16:
        return F16_FLOOR[name]
    cfg, p64, inputs, r64, r32, eval64 = _case(name)
    return yard.autocast_floor(p64, inputs, cfg, CASES[name][0], dtype, r64, eval64)


@functools.lru_cache(maxsize=None)
def _hip16(name, dtype):
    """one train_step_loss of the HIP model in the dtype's mode (f16: under the loss scaler), then eval forwards on the updated
    running statistics: with folded BatchNorm (the fp32-storage fallback) and without (16-bit storage)"""
    ops = _ops()
    model, p64, inputs = _model(name)
    try:
        r = _step(model, inputs, MODE[dtype], scaled=dtype == F16)
        r["walk"] = r["tape"].walk.dtype
        del r["tape"], r["cap"]
        model.eval()
        with torch.no_grad():
            r["eval_folded"] = model(*inputs[:4]).cpu()
            model.fold_bn_eval = False
            r["eval_16"] = model(*inputs[:4]).cpu()
    finally:
        ops.set_compute_mode("f32")
    return r


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_end_to_end_against_fp64_on_the_autocast_yardstick(dtype, name):
    """On bf16 the yardstick is so coarse that this only excludes gross errors (module docstring)."""
    tfm = CASES[name][0]
    cfg, p64, inputs, r64, r32, eval64 = _case(name)
    assert r64["kink"] >= mr.KINK_MIN and (not tfm or r64["margin"] >= mr.MARGIN_MIN)
    h, f = _hip16(name, dtype), _floor(name, dtype)
    assert h["walk"] == dtype
    assert set(h["grads"]) == set(r64["grads"])
    for k, ref in r64["grads"].items():
        if ref is None:      # the temporal head without TFM: exactly zero, not NaN, not stale
            assert k.startswith("encoder.time_mamba.") and not tfm, k
            assert h["grads"][k] is None or bool((h["grads"][k] == 0).all()), k
        else:
            assert torch.isfinite(h["grads"][k]).all(), k
    l2, cos = yard.grad_stats(h["grads"], r64["grads"])
    e_hip = yard.rel64(h["logits"], r64["logits"])
    print(f"\nfuser16 {_name(dtype):<5s} case {name} over {len(l2)} tensors (vs fp64)  HIP: logits {e_hip:.3e} median "
          f"{yard.median(l2):.3e} worst {l2[0][0]:.3e} ({l2[0][1]}) cos>0.9 {cos:.3f} scale {h['scale']:g} | autocast: logits "
          f"{f['logits']:.3e} median {f['med']:.3e} worst {f['worst']:.3e} cos>0.9 {f['cos']:.3f}", flush=True)
    assert len(l2) > 150
    assert e_hip < 2.0 * f["logits"] + 2e-3
    assert yard.median(l2) < 1.5 * f["med"] + 0.02
    assert l2[0][0] < 2.0 * f["worst"]
    assert cos >= f["cos"] - 0.05


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_eval_logits_against_the_fp64_eval_logits(dtype, name):
    """eval() in a 16-bit mode: with folded BatchNorm the walk falls back to fp32 storage as the parent's does, without it
    the 16-bit walk runs on the running statistics; both within 2 e_ac + 2e-3 of the fp64 eval logits"""
    *_, eval64 = _case(name)
    h, f = _hip16(name, dtype), _floor(name, dtype)
    e_fold, e_16 = yard.rel64(h["eval_folded"], eval64), yard.rel64(h["eval_16"], eval64)
    print(f"\nfuser16 {_name(dtype):<5s} case {name} eval logits vs fp64: folded BN (fp32 storage) {e_fold:.3e}, 16-bit storage "
          f"{e_16:.3e} | autocast {f['eval']:.3e}", flush=True)
    assert e_fold < 2.0 * f["eval"] + 2e-3
    assert e_16 < 2.0 * f["eval"] + 2e-3


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
LR, ITERS = 2e-4, 8


@pytest.mark.parametrize("name", ["A", "B"])
def test_the_loss_falls_in_every_mode(name):
    from deepsense6g_tii_amd.train import DynamicLossScaler, FusedAdamW, train_iteration
    ops = _ops()
    model, p64, inputs = _model(name)
    report = []
    for mode in ("f32", "bf16", "f16"):      # f32 first: LR / ITERS must make the parent's path learn on this case
        _reset(model, p64)
        model.zero_grad(set_to_none=True)
        ops.set_compute_mode(mode)
        model.train()
        scaler = DynamicLossScaler() if mode == "f16" else None
        opt = FusedAdamW(model, lr=LR, loss_scaler=scaler)
        losses = []
        for _ in range(ITERS):
            loss, logits = train_iteration(model, opt, inputs)
            losses.append(float(loss))
            assert torch.isfinite(logits).all(), (mode, losses)
        torch.cuda.synchronize()
        steps = opt.applied_steps() if scaler is not None else ITERS
        report.append(f"fuser16 train case {name} {mode:<5s} loss {losses[0]:.6f} -> {losses[-1]:.6f}, {steps} of {ITERS} "
                      f"steps applied" + (f", scale {scaler.get_scale():g}" if scaler else ""))
        print("\n" + report[-1], flush=True)
        assert losses[-1] < losses[0], (mode, losses)
        assert torch.isfinite(model.flat_parameters()[0]).all(), mode
        if scaler is not None:
            sc = scaler.get_scale()
            assert sc > 0 and sc < float("inf"), sc
            assert 1 <= steps <= ITERS, steps          # applied_steps(): skipped (overflowed) steps are not counted


def test_modes_switch_between_steps_on_one_model():
    from deepsense6g_tii_amd.train import DynamicLossScaler, FusedAdamW, train_iteration
    ops = _ops()
    model, p64, inputs = _model("A")
    model.train()
    opt = FusedAdamW(model, lr=LR, loss_scaler=DynamicLossScaler())
    want = {"f32": None, "bf16": BF16, "f16": F16}
    for mode in ("f32", "bf16", "f16", "f32"):
        ops.set_compute_mode(mode)
        loss, logits = train_iteration(model, opt, inputs)
        assert torch.isfinite(loss).all() and torch.isfinite(logits).all(), mode
        if want[mode] is not None:
            assert model._arena16.dtype == want[mode], mode      # the shadow was reallocated for the mode
    torch.cuda.synchronize()
    assert torch.isfinite(model.flat_parameters()[0]).all()


def test_an_applied_ema_shadow_falls_back_to_fp32_storage():
    from deepsense6g_tii_amd.train import EMA, FusedAdamW, train_iteration
    ops = _ops()
    model, p64, inputs = _model("A")
    model.train()
    opt = FusedAdamW(model, lr=LR, ema_decay=0.999)
    ema = EMA(model, 0.999, opt)
    ema.register()
    ops.set_compute_mode("bf16")
    train_iteration(model, opt, inputs, ema)
    ema.apply_shadow()
    assert not model.params_in_arena()
    model.eval()
    model.fold_bn_eval = False
    seen = []
    stage_fwd = model._stage_fwd
    model._stage_fwd = lambda wk, s, feats, gps_src, B: (seen.append((wk.dtype, feats[0].dtype)),
                                                        stage_fwd(wk, s, feats, gps_src, B))[1]
    with torch.no_grad():
        logits = model(*inputs[:4])
    del model._stage_fwd
    assert seen == [(F32, F32)] * 4 and torch.isfinite(logits).all()
    ema.restore()
    assert model.params_in_arena()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32x3", "f32x6"])
def test_the_split_modes_are_still_refused_at_the_first_forward(mode):
    ops = _ops()
    model, p64, inputs = _model("A")
    ops.set_compute_mode(mode)
    model.train()
    with pytest.raises(RuntimeError):
        model.train_step_loss(*inputs)
    model.eval()
    with pytest.raises(RuntimeError), torch.no_grad():
        model(*inputs[:4])


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_graph_capture_and_the_frozen_engine_are_refused_in_every_mode(mode):
    from deepsense6g_tii_amd.train import CapturedTrainStep, FusedAdamW
    ops = _ops()
    model, p64, inputs = _model("A")
    ops.set_compute_mode(mode)
    opt = FusedAdamW(model, lr=1e-3)
    with pytest.raises(NotImplementedError):
        CapturedTrainStep(model, opt, inputs)
    model.eval()
    for storage in ("f32", "bf16", "f16"):
        with pytest.raises(NotImplementedError):
            model.freeze_inference(storage)
    with pytest.raises(NotImplementedError):
        model.capture_inference(*inputs[:4])
