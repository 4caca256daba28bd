"""GPU: the frozen inference engine (TransFuser.freeze_inference -> infer.InferenceEngine) and its kernels - the BN fold to a
16-bit filter, the 16-bit conv with the bias / residual / ReLU epilogue, the inference stem - then the engine itself: the
"f32" engine is bit-identical to model.eval(), the snapshot rule, the captured graph, and the 16-bit engines against the only
16-bit eval the code had before (unfolded BN under compute mode "bf16" / "f16")."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}   # unit roundoff of the storage type
NODROP = dict(embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)


def r16(t, dtype):  # round to the 16-bit type and back (RNE): what the storage does to every 16-bit tensor
    return t.to(dtype).double()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


def within_one_rounding(y16, ref, u):
    """|y - ref| <= u |ref| + 2e-5 max|ref| elementwise (one rounding of the stored output plus fp32 accumulation): the
    project's one-rounding bound (tests/test_f16_gpu.py) with the unit roundoff of the storage type"""
    y, r = y16.double().cpu(), ref.double().cpu()
    bound = u * r.abs() + 2e-5 * r.abs().max()
    return bool(((y - r).abs() <= bound).all()), ((y - r).abs() / (r.abs() + 1e-30)).max().item()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _model(dev, kw, seed, cls=None, batch=2, **rkw):
    """model with fr.make_state weights whose BN running statistics were moved off their initial values by one training
    step (no optimizer step: the parameters are still those of the state dict)"""
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
    from oracle import fusion_ref as fr
    rcfg = fr.RefConfig(**kw, **rkw)
    model = (cls or TransFuser)(GlobalConfig(**kw), dev)
    model.load_state_dict(fr.make_state(rcfg, seed=seed))
    model.train()
    imgs, lids, rads, gps, target, _ = fr.make_inputs(rcfg, batch, seed=seed + 1000)
    if model.gru_head:
        target = torch.rand(batch, model.pred_len, 64, generator=torch.Generator().manual_seed(1)) * 0.5
    model.train_step_loss(imgs, lids, rads, gps, target)
    for p in model.parameters():
        p.grad = None
    return model, rcfg


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("K,taps,cin,cpad", [(128, 9, 64, 64), (256, 1, 128, 128), (64, 49, 3, 4)])
def test_bn_fold_to_16_bit_is_the_fp32_fold_rounded_once(dev, kind, K, taps, cin, cpad):
    from deepsense6g_tii_amd import ops
    g = torch.Generator().manual_seed(K + taps)
    bn = torch.nn.BatchNorm2d(K)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(K, generator=g))
        bn.bias.copy_(torch.randn(K, generator=g))
        bn.running_mean.copy_(torch.randn(K, generator=g))
        bn.running_var.copy_(torch.rand(K, generator=g) * 2 + 0.05)
    bn = bn.to(dev)
    w = (torch.randn(K, taps, cin, generator=g) / math.sqrt(taps * cin)).to(dev)
    w32, b32 = ops.bn_fold(w.data_ptr(), bn, K, taps, cin, cpad)
    w16, b16 = ops.bn_fold(w.data_ptr(), bn, K, taps, cin, cpad, dtype=DTYPES[kind])
    assert w16.dtype == DTYPES[kind] and b16.dtype == torch.float32 and w16.shape == w32.shape
    assert torch.equal(w16, w32.to(DTYPES[kind]))
    assert torch.equal(b16, b32)
    # into caller-owned buffers (the engine's refresh): same values
    w16b, b16b = torch.zeros_like(w16), torch.zeros_like(b16)
    ops.bn_fold(w.data_ptr(), bn, K, taps, cin, cpad, out=(w16b, b16b))
    assert torch.equal(w16b, w16) and torch.equal(b16b, b16)
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    want = torch.zeros(K, taps, cpad, dtype=torch.float64, device=dev)
    want[:, :, :cin] = w.double() * scale[:, None, None]
    assert relerr(w32, want) < 1e-6
    assert relerr(b32, bn.bias.double() - bn.running_mean.double() * scale) < 1e-6


def _conv_case(dev, kind, N, H, C, K, R, stride, seed, res_scale=1.0):
    """every (relu, residual) combination of the epilogue kernel at one shape against the fp64 act(conv + bias [+ residual])
    of the same rounded operands"""
    from deepsense6g_tii_amd import ops
    dt, u = DTYPES[kind], UNIT[kind]
    g = torch.Generator().manual_seed(seed)
    pad = R // 2
    x = torch.randn(N, C, H, H, generator=g)
    w = torch.randn(K, C, R, R, generator=g) / math.sqrt(C * R * R)
    bias = torch.randn(K, generator=g)
    Ho = (H + 2 * pad - R) // stride + 1
    res = torch.randn(N, K, Ho, Ho, generator=g) * res_scale
    xh, wh, rh, bg = nhwc(x).to(dt).to(dev), nhwc(w).to(dt).to(dev), nhwc(res).to(dt).to(dev), bias.to(dev)
    conv = F.conv2d(r16(x, dt), r16(w, dt), None, stride, pad)
    cb = conv + bias.double()[None, :, None, None]
    worst_all = 0.0
    for relu in (0, 1, 2):
        for residual in (None, rh):
            y = ops.bf16_conv2d_bias_act_fwd(xh, wh.data_ptr(), bg.data_ptr(), K, R, R, stride, pad, relu=relu,
                                             residual=residual)
            assert y.dtype == dt and tuple(y.shape) == (N, Ho, Ho, K)
            ref = torch.relu(cb) if relu == 1 else cb
            if residual is not None:
                ref = ref + r16(res, dt)
            if relu == 2:
                ref = torch.relu(ref)
                assert (y.float() >= 0).all()
            ok, worst = within_one_rounding(y.permute(0, 3, 1, 2), ref, u)
            worst_all = max(worst_all, worst)
            assert ok, (relu, residual is not None, worst)
    # zero bias, no residual, no ReLU: the plain 16-bit conv, bit for bit
    zero = torch.zeros(K, device=dev)
    y0 = ops.bf16_conv2d_bias_act_fwd(xh, wh.data_ptr(), zero.data_ptr(), K, R, R, stride, pad)
    assert torch.equal(y0, ops.bf16_conv2d_fwd(xh, wh.data_ptr(), K, R, R, stride, pad))
    return worst_all


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("R,stride", [(3, 1), (3, 2), (1, 2)])
def test_conv_bias_act_16_bit_at_bench_shape(dev, kind, R, stride):
    worst = _conv_case(dev, kind, 60, 16, 64, 128, R, stride, seed=10 * R + stride)
    print(f"{kind} {R}x{R}/{stride}: worst relative error {worst:.3e}")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_conv_bias_act_16_bit_other_tiles_and_large_residual(dev, kind):
    """K = 64 (one 64-wide tile column); a 32x32 map (480 workgroups: the 128 x 128 tile); a ragged pixel count (N = 3, 14x14:
    the last tile row is partly out of range); and a residual 100x the conv's magnitude (the add must happen in fp32, before
    the one rounding)"""
    _conv_case(dev, kind, 60, 16, 64, 64, 3, 1, seed=5)
    _conv_case(dev, kind, 60, 32, 64, 128, 3, 1, seed=6)
    _conv_case(dev, kind, 3, 14, 128, 72, 3, 1, seed=7)
    _conv_case(dev, kind, 60, 16, 64, 128, 3, 1, seed=8, res_scale=100.0)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("cin", [3, 1, 2])
def test_inference_stem_16_bit(dev, kind, cin):
    """fold (cpad 4) -> pack -> relu(conv7x7/2 + bias) -> index-free max-pool, against fp64 on the same rounded operands; the
    pool of the stored map is exact"""
    from deepsense6g_tii_amd import ops
    dt, u = DTYPES[kind], UNIT[kind]
    g = torch.Generator().manual_seed(cin)
    N, H, W = 3, 64, 96
    x = torch.zeros(N, 4, H, W)
    x[:, :cin] = torch.randn(N, cin, H, W, generator=g)
    w16 = torch.zeros(64, 49, 4)
    w16[:, :, :cin] = torch.randn(64, 49, cin, generator=g) / math.sqrt(49 * cin)
    bias = torch.randn(64, generator=g)
    xh, wh, bg = nhwc(x).to(dt).to(dev), w16.to(dt).to(dev), bias.to(dev)
    wp = ops.bf16_stem_pack_filter(wh)
    a1 = ops.bf16_stem_bias_relu_fwd(xh, wp, bg)
    assert a1.dtype == dt and tuple(a1.shape) == (N, H // 2, W // 2, 64)
    wref = r16(w16, dt).view(64, 7, 7, 4).permute(0, 3, 1, 2)
    ref = torch.relu(F.conv2d(r16(x, dt), wref, bias.double(), 2, 3))
    ok, worst = within_one_rounding(a1.permute(0, 3, 1, 2), ref, u)
    assert ok, worst
    p1 = ops.bf16_maxpool3x3s2_fwd(a1)
    want = F.max_pool2d(a1.permute(0, 3, 1, 2).float(), 3, 2, 1)
    assert torch.equal(p1.permute(0, 3, 1, 2).float(), want)


# ------------------------------------------------------------------------------------------------ the engine
def _eval(model, x):
    was = model.training
    model.eval()
    with torch.no_grad():
        out = model(*x).clone()
    model.train(was)
    return out


@pytest.mark.parametrize("B", [2, 1])
def test_f32_engine_is_bit_identical_to_model_eval(dev, B):
    from oracle import fusion_ref as fr
    model, rcfg = _model(dev, dict(n_layer=1, **NODROP), seed=31)
    x = fr.make_inputs(rcfg, B, seed=35)[:4]
    eng = model.freeze_inference()      # the model is in train mode: the engine is the eval forward regardless
    assert eng.storage == "f32" and eng.nbytes > 0 and eng.training is False
    out = eng(*x)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 64) and not out.requires_grad
    assert torch.equal(out, _eval(model, x))
    assert model.training and all(p.grad is None for p in model.parameters())


def test_engines_take_packed_inputs(dev):
    """data.PackedInputs (stem-ready NHWC x4 fp32) goes through the same door as the frame lists, in every storage"""
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd._lib import lib
    from deepsense6g_tii_amd.data import PackedInputs
    from oracle import fusion_ref as fr
    model, rcfg = _model(dev, dict(n_layer=1, **NODROP), seed=31)
    imgs, lids, rads, gps = fr.make_inputs(rcfg, 2, seed=35)[:4]
    packed = []
    for frames, cin, norm in ((imgs, 3, 1), (lids, 1, 0), (rads, 2, 0)):
        B, _, H, W = frames[0].shape
        S = len(frames)
        dst = torch.zeros((B * S, H, W, 4), device=dev)
        for t, f in enumerate(frames):
            src = f.to(dev, torch.float32).contiguous()
            lib().pack_input(src.data_ptr(), dst.data_ptr(), B, cin, H, W, 4, S, t, norm, ops._stream())
        packed.append(dst)
    pk = PackedInputs(packed[0], packed[1], packed[2], gps.to(dev), 2, len(lids))
    for storage in ("f32", "bf16", "f16"):
        eng = model.freeze_inference(storage)
        assert torch.equal(eng(pk, None, None, None), eng(imgs, lids, rads, gps)), storage
    assert torch.equal(model.freeze_inference()(pk), _eval(model, (imgs, lids, rads, gps)))


def test_f32_engine_is_bit_identical_for_the_30to5_model(dev):
    from deepsense6g_tii_amd.model import TransFuser30to5
    from oracle import fusion_ref as fr
    kw = dict(seq_len=10, n_layer=1, pred_len=5, **NODROP)
    model, rcfg = _model(dev, kw, seed=9, cls=TransFuser30to5, batch=1, gru_head=True)
    x = fr.make_inputs(rcfg, 1, seed=100)[:4]
    out = model.freeze_inference("f32")(*x)
    assert tuple(out.shape) == (1, 5, 64)
    assert torch.equal(out, _eval(model, x))


def test_engine_is_a_snapshot_until_refresh(dev):
    """after freeze_inference the model trains on (a bias edit, a training step that moves every gradient and the BN
    statistics, an optimizer step): the engine's output does not move; refresh() takes the new state; with an EMA shadow
    applied at refresh time the engine equals the model evaluated under the shadow"""
    from deepsense6g_tii_amd.train import EMA, FusedAdamW
    from oracle import fusion_ref as fr
    model, rcfg = _model(dev, dict(n_layer=1, **NODROP), seed=41)
    imgs, lids, rads, gps, target, _ = fr.make_inputs(rcfg, 2, seed=50)
    x = (imgs, lids, rads, gps)
    opt = FusedAdamW(model, lr=1e-3)
    eng = model.freeze_inference("f32")
    before = eng(*x).clone()
    assert torch.equal(before, _eval(model, x))
    model.join[4].bias.data.add_(1.0)
    opt.zero_grad()
    model.train_step_loss(imgs, lids, rads, gps, target)
    opt.step()
    assert torch.equal(eng(*x), before)
    now = _eval(model, x)
    assert not torch.equal(now, before)
    assert eng.refresh() is eng
    assert torch.equal(eng(*x), now)
    # EMA: a shadow that differs from the live weights, applied while the engine refreshes
    ema = EMA(model, 0.5)
    ema.register()
    opt.zero_grad()
    model.train_step_loss(imgs, lids, rads, gps, target)
    opt.step()
    ema.update()
    live = _eval(model, x)
    ema.apply_shadow()
    under_shadow = _eval(model, x)
    eng.refresh()
    ema.restore()
    assert not torch.equal(under_shadow, live)
    assert torch.equal(eng(*x), under_shadow)
    assert torch.equal(_eval(model, x), live)


@pytest.mark.parametrize("storage", ["f32", "bf16", "f16"])
def test_engine_graph_matches_eager_and_sees_refresh(dev, storage):
    from oracle import fusion_ref as fr
    model, rcfg = _model(dev, dict(n_layer=1, **NODROP), seed=41)
    a = fr.make_inputs(rcfg, 1, seed=50)[:4]
    b = fr.make_inputs(rcfg, 1, seed=51)[:4]
    eng = model.freeze_inference(storage)
    run = eng.capture(*a)
    assert torch.equal(run(*a), eng(*a))
    assert torch.equal(run(*b), eng(*b))
    old = eng(*b).clone()
    model.join[4].bias.data.add_(1.0)
    model.encoder.image_encoder.features.layer1[0].bn1.running_mean.add_(0.25)
    assert torch.equal(run(*b), old)            # a snapshot: the graph does not follow the live weights ...
    eng.refresh()
    new = eng(*b).clone()
    assert not torch.equal(new, old)
    assert torch.equal(run(*b), new)            # ... but the SAME graph serves the refreshed snapshot
    assert torch.isfinite(new).all()


def _deviations(dev, model, x):
    """(e32, {kind: d_old}, {kind: d_new}): e32 = model.eval() logits in mode "f32"; d_old = max-norm relative deviation from
    e32 of the only 16-bit eval the code had before the engine (mode kind, model.eval(), fold_bn_eval False); d_new = the same
    deviation of freeze_inference(storage=kind) run in mode "f32" """
    from deepsense6g_tii_amd import ops
    d_old, d_new = {}, {}
    try:
        ops.set_compute_mode("f32")
        e32 = _eval(model, x)
        for kind in ("bf16", "f16"):
            ops.set_compute_mode(kind)
            model.fold_bn_eval = False
            d_old[kind] = relerr(_eval(model, x), e32)
            model.fold_bn_eval = True
            ops.set_compute_mode("f32")
            eng = model.freeze_inference(storage=kind)
            out = eng(*x)
            assert out.dtype == torch.float32 and torch.isfinite(out).all()
            d_new[kind] = relerr(out, e32)
            del eng
    finally:
        model.fold_bn_eval = True
        ops.set_compute_mode("f32")
    return e32, d_old, d_new


def test_16_bit_engines_against_the_unfolded_16_bit_eval(dev):
    """n_layer 2, B = 2, state seed 3, inputs seed 100 (the configuration of the f16 whole-path test).  Measured on an MI355X
    (the four values are printed): d_old bf16 3.94e-3, f16 5.83e-4; d_new bf16 5.17e-3, f16 4.34e-4."""
    from oracle import fusion_ref as fr
    kw = dict(n_layer=2, **NODROP)
    model, rcfg = _model(dev, kw, seed=3)
    x = fr.make_inputs(rcfg, 2, seed=100)[:4]
    _, d_old, d_new = _deviations(dev, model, x)
    print(f"n_layer 2, B 2: d_old bf16 {d_old['bf16']:.3e} f16 {d_old['f16']:.3e}; "
          f"d_new bf16 {d_new['bf16']:.3e} f16 {d_new['f16']:.3e}")
    for kind in ("bf16", "f16"):
        assert d_new[kind] <= 1.5 * d_old[kind], (kind, d_new[kind], d_old[kind])
    assert d_new["f16"] < d_new["bf16"]
    # the project's existing whole-path bars for the same storage (tests/test_bf16_gpu.py, tests/test_f16_gpu.py)
    assert d_new["bf16"] < 3e-2 and d_new["f16"] < 3e-3


def test_16_bit_engines_at_the_benchmark_shape(dev):
    """B = 12, n_layer 8, default config, make_batch(12, seed=100)"""
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
    from deepsense6g_tii_amd.synthetic import make_batch
    from oracle import fusion_ref as fr
    model = TransFuser(GlobalConfig(), dev)
    model.load_state_dict(fr.make_state(fr.RefConfig(), seed=3))
    fronts, lidars, radars, gps, soft, _ = make_batch(12, seed=100, device=dev)
    model.train()
    model.train_step_loss(fronts, lidars, radars, gps, soft)
    for p in model.parameters():
        p.grad = None
    x = (fronts, lidars, radars, gps)
    e32, d_old, d_new = _deviations(dev, model, x)
    print(f"n_layer 8, B 12: d_old bf16 {d_old['bf16']:.3e} f16 {d_old['f16']:.3e}; "
          f"d_new bf16 {d_new['bf16']:.3e} f16 {d_new['f16']:.3e}")
    top = e32.argmax(1)
    for kind in ("bf16", "f16"):
        out = model.freeze_inference(kind)(*x)
        assert torch.isfinite(out).all()
        print(f"{kind}: top-1 beam differs from the fp32 eval on {(out.argmax(1) != top).float().mean().item():.3f} of the samples")
        assert d_new[kind] <= 1.5 * d_old[kind], (kind, d_new[kind], d_old[kind])


def test_validate_and_test_accept_the_engine(dev, tmp_path):
    from deepsense6g_tii_amd import train
    from deepsense6g_tii_amd.synthetic import make_batch
    model, _ = _model(dev, dict(n_layer=1, **NODROP), seed=31)
    batches = []
    for seed in (7, 8):
        fronts, lidars, radars, gps, _, beam = make_batch(2, seed=seed, device=dev)
        batches.append((fronts, lidars, radars, gps, beam))
    eng = model.freeze_inference("f32")
    assert model.training
    dba_e, acc_e, pred_e = train.validate(eng, batches)
    assert model.training                       # validate(engine) never touches the model's flag
    dba_m, acc_m, pred_m = train.validate(model, batches)
    assert (pred_e == pred_m).all() and dba_e == dba_m and (acc_e == acc_m).all()
    p_e, c_e = train.test(eng, batches, target_csv=str(tmp_path / "e.csv"), confidence_csv=str(tmp_path / "ec.csv"))
    p_m, c_m = train.test(model, batches, target_csv=str(tmp_path / "m.csv"), confidence_csv=str(tmp_path / "mc.csv"))
    assert (p_e == p_m).all() and (c_e == c_m).all()
    assert model.training
    assert eng.train(True) is eng and eng.training is False and eng.eval() is eng
