"""GPU: a model walk's result does not depend on stream timing or on what freed memory holds (tests/perturb.py).

Configurations - the smallest that walk every stage: n_layer 1, seq_len 1, B 2, dropout 0.1 (the mask counters run):
    f32     TransFuser, exact fp32
    bf16    TransFuser, bf16 storage
    f16     TransFuser, f16 storage with train.DynamicLossScaler
    30to5   TransFuser30to5 (the GRU head)
    mamba   MambaFuser (TFM 0: the temporal head hard-wires 5 frames)

A run builds its model from the configuration's state dict and dropout seed, does step 1 (train_step_loss + FusedAdamW.step
with the fused EMA shadow) on 0x00-filled memory so that the lazy streams and workspaces exist, applies its perturbation and
does step 2.  Of step 2 the logits, the loss, the gradient arena, parameters / both moments / the EMA shadow after the update,
the BatchNorm running statistics and num_batches_tracked, the optimizer's device scalars and the loss scaler's state are
compared BIT FOR BIT (moat.bits) with the baseline R0 (default streams, 0x00 fill, no delay); all of it must be finite.

A fill covers every free block of the model's streams and its persistent per-stream workspaces, in R0 too (with 0x00): the runs
differ in the byte alone, also in what the device did just before the timed step.

Step-2 runs:  ff      the fill byte is 0xFF (NaN / 255 / -1)
              <name>  ff, and the stream <name> (trunk0 / trunk1 / trunk2 / wgrad / main) is late: perturb.delayed
              single  multi_stream = False; here and in its own baseline the calling stream's scratch has the 256 MiB of a
                      side stream's, so that every kernel plans on the scratch size it sees in the default run
MambaFuser sends no launch to a companion stream (its stages differentiate in one call, the trunks' weight gradients stay
on the trunk streams): it has no wgrad case, and the ff case asserts that no companion stream exists.

What keeps these from passing by accident is asserted, not assumed:
  - after a fill, fresh torch.empty tensors of 4 B .. 64 MiB on every stream of the model hold only the fill byte;
  - memory_reserved() after step 2 equals what the fill returned: step 2 took no segment the fill had not seen;
  - the delay is 2 x the longest host time between a _fork() and its _join(), measured in R0's step 2: a consumer without a
    wait is enqueued within that time and would run at once on its idle stream; it stays below the sleeper's 2 s bound;
  - a delayed run injected at least one sleeper, and its wall time exceeds R0's by at least half of injections x delay.
    Both wall times are taken behind a gate (_gate) that keeps the device from starting before the host has enqueued the step.
"""
import functools
import time

import pytest
import torch

from tests import moat, perturb

pytestmark = pytest.mark.gpu

B = 2
KW = dict(n_layer=1, seq_len=1, embd_pdrop=0.1, attn_pdrop=0.1, resid_pdrop=0.1)
SIDE_WS = 256 << 20
DROPOUT_SEED = 20260
# name: (model, compute mode, loss scaler, state seed, input seed)
CONFIGS = {"f32": ("TransFuser", "f32", False, 61, 161),
           "bf16": ("TransFuser", "bf16", False, 62, 162),
           "f16": ("TransFuser", "f16", True, 63, 163),
           "30to5": ("TransFuser30to5", "f32", False, 64, 164),
           "mamba": ("MambaFuser", "f32", False, 65, 165)}
DELAYS = {n: [s for s in perturb.STREAM_NAMES if not (n == "mamba" and s == "wgrad")] for n in CONFIGS}


@pytest.fixture(scope="module", autouse=True)
def _drop_baselines():
    """the baselines (about 1 GB of device memory per configuration) live as long as this module's tests"""
    yield
    for f in (_case, _baseline, _eval_model):
        f.cache_clear()


def _gate(micros):
    """Holds the calling stream for `micros` at the start of a timed step (the sleeper of perturb.delayed; every other stream
    waits for the calling stream at the first fork, so no stream is late relative to another).  At B = 2 a step is host-bound:
    the device idles between launches, and a stream that is made late catches up while the host is still enqueueing - measured
    without the gate, 8 sleepers of 2.0 ms added 7.7 ms (bf16, trunk1) to 14.7 ms (f32, trunk0) to a 10 - 12 ms step, on either
    side of the bound below.  Behind a gate longer than the host needs for the step the device has everything queued when it
    starts: the wall times measure the device's schedule, and a consumer without a wait is enqueued before its producer ran."""
    if micros:
        from deepsense6g_tii_amd import ops
        from deepsense6g_tii_amd._lib import lib
        lib().debug_occupy_cus(1, 0, int(micros), ops._stream())


def _note(msg):
    print(f"[schedule] {msg}", flush=True)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (config keywords, state dict, batch) of a configuration, made once on the CPU"""
    from oracle import fusion_ref as fr
    cls, _, _, seed, iseed = CONFIGS[name]
    if cls == "MambaFuser":
        from tests import mamba_fuser_ref as mr
        kw = dict(KW, TFM=0)
        rcfg = fr.RefConfig(**KW)
        sd = {k: (v.float() if v.is_floating_point() else v) for k, v in mr.make_params(rcfg, seed).items()}
    else:
        kw = dict(KW)
        rcfg = fr.RefConfig(gru_head=cls == "TransFuser30to5", **KW)
        sd = fr.make_state(rcfg, seed=seed)
    imgs, lids, rads, gps, target, _ = fr.make_inputs(rcfg, B, seed=iseed)
    if cls == "TransFuser30to5":
        target = torch.rand(B, rcfg.pred_len, 64, generator=torch.Generator().manual_seed(iseed)) * 0.5
    return kw, sd, (imgs, lids, rads, gps, target)


def _build(name, dev):
    from deepsense6g_tii_amd import mamba_fuser, model as M
    from deepsense6g_tii_amd.train import DynamicLossScaler, FusedAdamW
    cls, _, scaled, _, _ = CONFIGS[name]
    kw, sd, _ = _case(name)
    ctor = mamba_fuser.MambaFuser if cls == "MambaFuser" else getattr(M, cls)
    model = ctor(M.GlobalConfig(**kw), dev)
    model.load_state_dict(sd, strict=True)
    assert model.params_in_arena()
    model.set_dropout_seed(DROPOUT_SEED)
    model.train()
    opt = FusedAdamW(model, lr=1e-4, ema_decay=0.999, loss_scaler=DynamicLossScaler() if scaled else None)
    return model, opt


def _state(model, opt, loss, logits):
    """what is compared: {name: tensor} (clones, on the device)"""
    p, g = model.flat_parameters()
    stats = [b.reshape(-1) for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))]
    out = dict(logits=logits, loss=loss, grads=g, params=p, m=opt.m, v=opt.v, shadow=opt.shadow, bn_stats=torch.cat(stats),
               num_batches_tracked=model._nbt, adam_scalars=opt._dev)
    if opt.loss_scaler is not None:
        out["scaler"] = opt.loss_scaler.state
    return {k: v.detach().clone() for k, v in out.items()}


def _assert_finite(state, what):
    for k, v in state.items():
        if v.is_floating_point():
            assert bool(torch.isfinite(v).all()), f"{what}: {k} holds {int((~torch.isfinite(v)).sum())} non-finite values"


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    bad = []
    for k in want:
        a, b = moat.bits(got[k]), moat.bits(want[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if not torch.equal(a, b):
            diff = a != b
            bad.append(f"{k}: {int(diff.sum())} of {a.numel()} words differ, first at {int(diff.reshape(-1).nonzero()[0])}")
    assert not bad, f"{what} differs from its baseline bit for bit:\n  " + "\n  ".join(bad)


def _train_run(name, dev, byte, which=None, micros=None, single=False, small_main=False, gate=None):
    """one run as the module docstring describes it -> dict(state, wall [s] of step 2, longest fork-to-join host time [s],
    injections)"""
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.train import train_iteration
    _, mode, _, _, _ = CONFIGS[name]
    batch = _case(name)[2]
    ops.set_compute_mode(mode)
    model = own_ws = None
    try:
        model, opt = _build(name, dev)
        own_ws = model._ws_main
        if single:
            model.multi_stream = False
        if small_main:
            model._ws_main = ops.Workspace(dev, SIDE_WS)
        perturb.fill_free_memory(0x00, perturb.model_streams(model))
        train_iteration(model, opt, batch)                      # step 1: the lazy streams and workspaces exist after it
        torch.cuda.synchronize()
        streams = perturb.model_streams(model)
        assert len(streams) == (1 if single else 4 + len(model._wg_map)), len(streams)
        if name == "mamba":
            assert not model._wg_map, "MambaFuser now has a companion stream: give it the wgrad case"
        elif not single:
            assert len(model._wg_map) == 1, model._wg_map
        ctx = perturb.delayed(model, which, micros) if which is not None else perturb.timed(model)
        with perturb.no_gc():
            reserved = perturb.fill_free_memory(byte, streams)
            perturb.assert_filled(byte, streams)
            perturb.fill_workspaces(model, byte)
            torch.cuda.synchronize()
            with ctx:
                t0 = time.perf_counter()
                _gate(gate)
                loss, logits = train_iteration(model, opt, batch)   # step 2
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
        assert not any(n in model.__dict__ for n in perturb._Wrapped.NAMES)
        now = torch.cuda.memory_reserved()
        assert now == reserved, (f"step 2 took {now - reserved} bytes of new segments: the fill was too small, part of the "
                                 "step ran on memory it had not filled")
        if opt.loss_scaler is not None:
            assert not opt.loss_scaler.found_inf(), "the loss scaler skipped step 2: nothing was compared"
        state = _state(model, opt, loss, logits)
        return dict(state=state, wall=wall, longest=getattr(ctx, "longest", None), sections=getattr(ctx, "sections", None),
                    injections=getattr(ctx, "injections", 0))
    finally:
        ops.set_compute_mode("f32")
        if model is not None:
            model.multi_stream = True
            model._ws_main = own_ws


@functools.lru_cache(maxsize=None)
def _baseline(name, small_main=False):
    """R0 (or, small_main, the single-stream run's own baseline): default streams, 0x00 fill, no delay.  R0 is run four times, as it
    comes and three times behind the gate every perturbed run has (_gate): all must agree bit for bit (a baseline that does not
    repeat compares nothing); its wall time is the shortest of the gated runs, the fork-to-join time the longest of all"""
    r = _train_run(name, torch.device("cuda:0"), 0x00, small_main=small_main)
    _assert_finite(r["state"], f"{name} baseline")
    if not small_main:
        natural = r["wall"]
        gate = min(int(2e6 * natural), perturb.MAX_MICROS)       # twice the host-bound step: the host is done when it opens
        r["wall"] = None
        for _ in range(3):
            again = _train_run(name, torch.device("cuda:0"), 0x00, gate=gate)
            _assert_same(again["state"], r["state"], f"{name} R0 repeated behind the gate")
            r["wall"] = again["wall"] if r["wall"] is None else min(r["wall"], again["wall"])
            r["longest"] = max(r["longest"], again["longest"])
            del again
        r["gate"] = gate
        _note(f"{name:6s} train R0      natural wall {natural * 1e3:6.1f} ms -> gate {gate} us")
        micros = int(2e6 * r["longest"])
        assert r["sections"] >= 8 and 0 < micros < perturb.MAX_MICROS, (r["sections"], micros)
        r["micros"] = micros
        _note(f"{name:6s} train R0      wall {r['wall'] * 1e3:8.1f} ms  fork sections {r['sections']:2d}  longest "
              f"{r['longest'] * 1e6:7.0f} us  -> delay {micros} us")
    return r


def _check_delay(r, r0, micros, what):
    assert r["injections"] > 0, f"{what}: no sleeper was injected"
    extra = r["wall"] - r0["wall"]
    _note(f"{what:20s} wall {r['wall'] * 1e3:8.1f} ms  injections {r['injections']:3d} x {micros} us  extra "
          f"{extra * 1e3:8.1f} ms")
    assert extra >= 0.5 * r["injections"] * micros * 1e-6, \
        f"{what}: {r['injections']} sleepers of {micros} us added only {extra * 1e3:.1f} ms: the delay did nothing"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_train_step_on_poisoned_memory_equals_baseline(dev, name):
    """ff: a buffer that is read before it is written reads NaN / 255 / -1 instead of zeros or last step's values"""
    r0 = _baseline(name)
    r = _train_run(name, dev, 0xFF, gate=r0["gate"])
    _note(f"{name:6s} train ff      wall {r['wall'] * 1e3:8.1f} ms")
    _assert_finite(r["state"], f"{name} ff")
    _assert_same(r["state"], r0["state"], f"{name} ff")


@pytest.mark.parametrize("name,which", [(n, w) for n in CONFIGS for w in DELAYS[n]])
def test_train_step_with_a_late_stream_equals_baseline(dev, name, which):
    """ff and one stream late: a consumer without a wait reads poison, an early reuse overwrites what a late reader needs"""
    r0 = _baseline(name)
    r = _train_run(name, dev, 0xFF, which=which, micros=r0["micros"], gate=r0["gate"])
    _check_delay(r, r0, r0["micros"], f"{name} train {which}")
    _assert_finite(r["state"], f"{name} {which}")
    _assert_same(r["state"], r0["state"], f"{name} {which}")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_train_step_on_one_stream_equals_the_default_streams(dev, name):
    """single: the same launches in one stream order.  Both runs plan on a 256 MiB scratch everywhere (in the default run the
    trunk and companion streams have that; the calling stream's 1 GiB is replaced), so no planner may choose another split"""
    r0 = _baseline(name, small_main=True)
    r = _train_run(name, dev, 0x00, single=True, small_main=True)
    _note(f"{name:6s} train single  wall {r['wall'] * 1e3:8.1f} ms (baseline on 256 MiB main scratch {r0['wall'] * 1e3:.1f} ms)")
    assert r["sections"] == 0
    _assert_finite(r["state"], f"{name} single")
    _assert_same(r["state"], r0["state"], f"{name} single")


# ---------------------------------------------------------------------------------------------------------------- eval
@functools.lru_cache(maxsize=None)
def _eval_model(name):
    """a model of the configuration after one training step (every lazy stream exists, the running statistics moved),
    in eval mode"""
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.train import train_iteration
    _, mode, _, _, _ = CONFIGS[name]
    ops.set_compute_mode(mode)
    try:
        model, opt = _build(name, torch.device("cuda:0"))
        train_iteration(model, opt, _case(name)[2])
        torch.cuda.synchronize()
    finally:
        ops.set_compute_mode("f32")
    model.eval()
    return model


def _eval_run(model, fwd, inputs, byte, which=None, micros=None, large_bytes=128 * perturb.MIB, gate=None):
    """one inference forward `fwd(*inputs)` on `byte`-filled memory -> dict(logits, wall, longest, sections, injections)"""
    streams = perturb.model_streams(model)
    ctx = perturb.delayed(model, which, micros) if which is not None else perturb.timed(model)
    with perturb.no_gc():
        reserved = perturb.fill_free_memory(byte, streams, large_bytes=large_bytes)
        perturb.assert_filled(byte, streams)
        perturb.fill_workspaces(model, byte)
        torch.cuda.synchronize()
        with ctx, torch.no_grad():
            t0 = time.perf_counter()
            _gate(gate)
            logits = fwd(*inputs)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
    now = torch.cuda.memory_reserved()
    assert now == reserved, f"the forward took {now - reserved} bytes of new segments: the fill was too small"
    assert bool(torch.isfinite(logits).all()), "non-finite logits"
    return dict(logits=logits.clone(), wall=wall, longest=getattr(ctx, "longest", None),
                sections=getattr(ctx, "sections", None), injections=getattr(ctx, "injections", 0))


def _same_logits(r, r0, what):
    _assert_same(dict(logits=r["logits"]), dict(logits=r0["logits"]), what)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_eval_forward_under_every_perturbation_equals_baseline(dev, name):
    """the eval forward has no tape: nothing but the stated discipline keeps a cross-stream tensor alive.  One model, its
    forward repeated: 0x00 baseline, ff, ff + each late stream, and one stream against a baseline on the same scratch size.
    An eval forward launches no weight gradient: the wgrad case must inject nothing (and still equal the baseline)."""
    from deepsense6g_tii_amd import ops
    model = _eval_model(name)
    inputs = _case(name)[2][:4]
    _, mode, _, _, _ = CONFIGS[name]
    ops.set_compute_mode(mode)
    own_ws = model._ws_main
    try:
        _eval_run(model, model, inputs, 0x00)                     # warm: the eval path's own lazy work is done
        first = _eval_run(model, model, inputs, 0x00)
        gate = int(2e6 * first["wall"])
        r0 = _eval_run(model, model, inputs, 0x00, gate=gate)
        _same_logits(first, r0, f"{name} eval R0 behind the gate")
        for _ in range(2):
            again = _eval_run(model, model, inputs, 0x00, gate=gate)
            _same_logits(again, r0, f"{name} eval R0 repeated")
            r0["wall"] = min(r0["wall"], again["wall"])
            r0["longest"] = max(r0["longest"], first["longest"], again["longest"])
        micros = int(2e6 * r0["longest"])
        assert r0["sections"] >= 4 and 0 < micros < perturb.MAX_MICROS, (r0["sections"], micros)
        _note(f"{name:6s} eval  R0      wall {r0['wall'] * 1e3:8.1f} ms  fork sections {r0['sections']:2d}  longest "
              f"{r0['longest'] * 1e6:7.0f} us  -> delay {micros} us")
        _same_logits(_eval_run(model, model, inputs, 0xFF, gate=gate), r0, f"{name} eval ff")
        for which in perturb.STREAM_NAMES:
            r = _eval_run(model, model, inputs, 0xFF, which=which, micros=micros, gate=gate)
            if which == "wgrad":
                assert r["injections"] == 0, "an eval forward launched a weight gradient"
            else:
                _check_delay(r, r0, micros, f"{name} eval  {which}")
            _same_logits(r, r0, f"{name} eval {which}")
        model._ws_main = ops.Workspace(dev, SIDE_WS)
        b = _eval_run(model, model, inputs, 0x00)
        model.multi_stream = False
        s = _eval_run(model, model, inputs, 0xFF)
        assert s["sections"] == 0
        _same_logits(s, b, f"{name} eval single")
    finally:
        ops.set_compute_mode("f32")
        model.multi_stream = True
        model._ws_main = own_ws


def test_frozen_engines_on_poisoned_memory(dev):
    """freeze_inference("f32") is documented as bit-identical to model.eval(); an engine's snapshot buffers come from
    torch.empty and are written by refresh().  Engines frozen AND run on 0xFF-filled memory: "f32" equals the model's eval
    forward, "bf16" equals the "bf16" engine frozen and run on 0x00-filled memory."""
    model = _eval_model("f32")
    inputs = _case("f32")[2][:4]
    base = _eval_run(model, model, inputs, 0x00)
    perturb.fill_free_memory(0x00, perturb.model_streams(model))
    e16_zero = model.freeze_inference("bf16")
    want16 = _eval_run(model, e16_zero, inputs, 0x00)
    del e16_zero
    perturb.fill_free_memory(0xFF, perturb.model_streams(model))
    e32, e16 = model.freeze_inference("f32"), model.freeze_inference("bf16")
    _same_logits(_eval_run(model, e32, inputs, 0xFF), base, "engine f32 on ff against model.eval()")
    _same_logits(_eval_run(model, e16, inputs, 0xFF), want16, "engine bf16 on ff against itself on 0x00")


def test_captured_inference_graph_matches_eager_on_poisoned_memory(dev):
    """the body of tests/test_model_gpu.py::test_captured_inference_graph_matches_eager with the EAGER side on 0xFF-filled
    memory and scratch (the graph's private pool cannot be filled).  That test once failed depending on which tests ran
    before it in the process; an eager forward that reads stale memory would differ from the replay here."""
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
    from oracle import fusion_ref as fr
    kw = dict(n_layer=1, embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    rcfg = fr.RefConfig(**kw)
    model = TransFuser(GlobalConfig(**kw), dev)
    model.load_state_dict(fr.make_state(rcfg, seed=41), strict=True)
    model.eval()
    a = fr.make_inputs(rcfg, 1, seed=50)[:4]
    b = fr.make_inputs(rcfg, 1, seed=51)[:4]
    run = model.capture_inference(*a)

    def both(inputs, what):
        replayed = run(*inputs).clone()
        eager = _eval_run(model, model, inputs, 0xFF, large_bytes=512 * perturb.MIB)   # five 256 x 256 frames per trunk
        assert bool(torch.isfinite(replayed).all())
        _same_logits(eager, dict(logits=replayed), what)
        again = run(*inputs)                                      # the replay after the scratch was poisoned
        _same_logits(dict(logits=again), dict(logits=replayed), what + " (replay on poisoned scratch)")

    both(a, "captured graph, first inputs")
    both(b, "captured graph, new inputs")
    model.join[4].bias.data.add_(1.0)
    both(b, "captured graph, changed weights")


# ---------------------------------------------------------------------------------------------------- launch discipline
@pytest.mark.parametrize("name", ["f32", "bf16", "mamba"])
def test_launch_discipline_of_a_training_step_and_an_eval_forward(dev, name):
    """what _fork()'s docstring states instead of record_stream(), on the recorded launches of one training step and one eval
    forward: between _fork() and _join() no launch on the calling stream; every launch on the calling stream, a trunk stream
    or a companion stream; nothing outstanding on a companion stream after the last _wg_join()."""
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.train import train_iteration
    _, mode, _, _, _ = CONFIGS[name]
    batch = _case(name)[2]
    ops.set_compute_mode(mode)
    try:
        model, opt = _build(name, dev)
        train_iteration(model, opt, batch)
        torch.cuda.synchronize()
        with perturb.Recorder(model) as rec:
            train_iteration(model, opt, batch)
            assert not rec.forked, "the step ended inside a fork section"
            assert not rec.outstanding and not model._wg_used and not model._wg_keep, \
                f"weight-gradient launches outstanding after the step: {rec.outstanding}"
            n_train, n_sections = len(rec.launches), rec.sections
            model.eval()
            with torch.no_grad():
                model(*batch[:4])
            assert not rec.forked and not rec.outstanding
        torch.cuda.synchronize()
        assert ops._stream() == rec.calling
        assert n_sections == 8 and rec.sections == 12, (n_sections, rec.sections)   # 4 forward + 4 backward; 4 eval
        assert n_train > 200 and len(rec.launches) > n_train + 100, (n_train, len(rec.launches))
        inside = [l for l in rec.launches if l[2]]
        trunks = {s.cuda_stream for s in model._side_streams}
        assert inside and {raw for _, raw, _ in inside} == trunks, "a fork section did not use exactly the three trunk streams"
        comps = {s.cuda_stream for s in model._wg_map.values()}
        on_comp = [l for l in rec.launches if l[1] in comps]
        assert (not comps and not on_comp) if name == "mamba" else (len(on_comp) > 0 and rec.joins >= 8), (len(on_comp), rec.joins)
        _note(f"{name:6s} discipline    {len(rec.launches)} launches recorded, {len(inside)} inside {rec.sections} fork sections, "
              f"{len(on_comp)} on the companion stream, {len(rec.violations)} violations")
        assert not rec.violations, "\n".join(rec.violations[:20])
        assert not any(n in model.__dict__ for n in perturb._Wrapped.NAMES)
    finally:
        ops.set_compute_mode("f32")
