"""GPU parity of the temporal Mamba fusion head (csrc/time_mamba.hip, deepsense6g_tii_amd/time_mamba.py) against
tests/time_mamba_ref.py.

Reference: the restatement in fp64.  Yardstick: the same restatement in fp32 on the CPU.  For every compared tensor
    e_hip = max|hip - ref64| / max|ref64|,   e_32 = the same for the fp32 CPU run (computed here, not hard-coded)
and the bar is e_hip <= max(10 * e_32, 1e-5) (tests/mamba_ref.rel_err / bar).  Every e_hip / e_32 pair is printed (pytest -s);
the committed summary is profiles/time_mamba_parity.txt.

Argmax margin: a row whose two largest values swap order between fp32 and fp64 moves the whole max-pool gradient to another
channel.  That is a condition on the inputs, not a tolerance: every case without a planted tie asserts on its fp64 run that
(top1 - top2) / max|row| >= 1e-4 for all 17 rows of every sample (about 100x the fp32 error of y).

The kernel-level cases call the C entry points directly: every operand that is read sits inside NaN moats, every output -
pre-filled with NaN (0xFF bytes for the int32 argmax) - inside 0xFF moats (tests/moat.py), and the guards must be unchanged.
Shapes: B in {1, 3}; S = 5 and C = 512 are fixed by the head, so one sample and an odd count that is no power of two are the
smallest shapes at which the indexing can go wrong."""
import functools

import pytest
import torch

from tests import mamba_ref as mr
from tests import moat
from tests import time_mamba_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
F64 = torch.float64
MOAT = moat.MIN_MOAT
C, S, R = tr.C, tr.S, tr.ROWS
TOKENS = 7                     # the strided cases read gps as rows 5, 6 of a [B][7][512] buffer: sample stride 3584 > 1024


def _compare(tag, hip, r32, r64, keys=None):
    bad = []
    print()
    for k in (keys or r64):
        e32 = mr.rel_err(r32[k], r64[k])
        eh = mr.rel_err(hip[k], r64[k])
        print(f"parity {tag:<34s} {k:<26s} e_hip {eh:.3e}  e_32 {e32:.3e}  bar {mr.bar(e32):.3e}")
        if not eh <= mr.bar(e32):
            bad.append((k, eh, e32))
    assert not bad, (tag, bad)


def _dev(t):
    return t.to(DEV, F32).contiguous()


# ---- 1. the two kernels -----------------------------------------------------------------------------------------------
KINDS = ("random", "negative", "edge", "tie", "stride", "accumulate")
TIE = (1, 3, 100, 400)          # (modality, frame) of sample 0 and the two channels of the planted tie
SEED_SHIFT = {("negative", 3): 900}     # seeds picked on the CPU for an argmax margin >= 1e-3 (README_timemamba.md)


@functools.lru_cache(maxsize=None)
def _head_case(kind, B):
    g = torch.Generator().manual_seed(400 + 10 * KINDS.index(kind) + B + SEED_SHIFT.get((kind, B), 0))
    y = torch.randn(3 * B, S, C, generator=g, dtype=F64)
    gps = torch.randn(B, 2, C, generator=g, dtype=F64)
    dout = torch.randn(B, C, generator=g, dtype=F64)
    pre = torch.randn(36, generator=g, dtype=F64) if kind == "accumulate" else None
    if kind == "negative":                                   # every row all negative: a running maximum that starts at 0 fails
        y, gps = y * 0.25 - 2.0, gps * 0.25 - 2.0         # scores near -1.2: the softmaxes stay unsaturated
        assert float(y.max()) < -0.5 and float(gps.max()) < -0.5
    if kind == "edge":                                       # the maximum at the first / the last channel, alternating by row
        yv, gv = y.view(-1, C), gps.view(-1, C)
        yv[0::2, 0] = 6.0
        yv[1::2, C - 1] = 6.0
        gv[0::2, C - 1] = 6.0
        gv[1::2, 0] = 6.0
    if kind == "tie":
        m, t, c0, c1 = TIE
        y[m * B, t, c0] = y[m * B, t, c1] = 7.0
    p = tr.make_head_params(seed=B)
    r64, margin = tr.head_run(p, y, gps, dout, F64)
    r32, _ = tr.head_run(p, y, gps, dout, F32)
    if pre is not None:
        off = 0
        for k in tr.HEAD_NAMES:
            n = r64[k].numel()
            r64[k] = r64[k] + pre[off:off + n].view_as(r64[k])
            r32[k] = r32[k] + pre[off:off + n].view_as(r32[k]).float()
            off += n
    return p, y, gps, dout, pre, r64, r32, margin


def _read(t, name):
    return moat.embed(_dev(t), MOAT, MOAT, "nan", name)


def _written(shape, dtype, name):
    return moat.embed(moat.nan_like(torch.empty(shape, dtype=dtype, device=DEV)), MOAT, MOAT, 0xFF, name)


def _run_head(kind, B):
    from deepsense6g_tii_amd import _lib, ops
    L = _lib.lib()
    p, y, gps, dout, pre, r64, r32, margin = _head_case(kind, B)
    guards = []

    def rd(t, name):
        v, gd = _read(t, name)
        guards.append(gd)
        return v

    def wr(shape, dtype, name):
        v, gd = _written(shape, dtype, name)
        guards.append(gd)
        return v

    yd, doutd = rd(y.view(-1, C), "y"), rd(dout, "dout")
    w5, b5, w2, b2 = (rd(p[k], k) for k in tr.HEAD_NAMES)
    if kind == "stride":
        big = torch.full((B, TOKENS, C), float("nan"), dtype=F64)
        big[:, TOKENS - 2:] = gps
        gbuf = rd(big, "gps buffer")
        gptr, ld = gbuf[0, TOKENS - 2].data_ptr(), TOKENS * C
        dgbuf = wr((B, TOKENS, C), F32, "dgps buffer")
        dgptr, dgps = dgbuf[0, TOKENS - 2].data_ptr(), dgbuf[:, TOKENS - 2:]
    else:
        gbuf = rd(gps, "gps")
        gptr, ld = gbuf.data_ptr(), 2 * C
        dgbuf = dgps = wr((B, 2, C), F32, "dgps")
        dgptr = dgbuf.data_ptr()
    out, attn, score = wr((B, C), F32, "out"), wr((B, R), F32, "attn"), wr((B, R), F32, "score")
    argmax = wr((B, R), torch.int32, "argmax")
    st = ops._stream()
    L.time_attn_fwd(yd.data_ptr(), gptr, ld, w5.data_ptr(), b5.data_ptr(), w2.data_ptr(), b2.data_ptr(), out.data_ptr(),
                    attn.data_ptr(), score.data_ptr(), argmax.data_ptr(), B, S, C, st)
    # the backward reads the saved tensors out of moats of their own
    attn_r, score_r = rd(attn.clone(), "attn (saved)"), rd(score.clone(), "score (saved)")
    argmax_r, gd = moat.embed(argmax.clone(), MOAT, MOAT, 0xFF, "argmax (saved)")
    guards.append(gd)
    dy, part = wr((3 * B * S, C), F32, "dy"), wr((B, 36), F32, "dparam_part")
    if pre is None:
        dparams = wr((36,), F32, "dparams")
    else:
        dparams, gd = moat.embed(_dev(pre), MOAT, MOAT, 0xFF, "dparams")
        guards.append(gd)
    L.time_attn_bwd(doutd.data_ptr(), yd.data_ptr(), gptr, ld, attn_r.data_ptr(), score_r.data_ptr(), argmax_r.data_ptr(),
                    w5.data_ptr(), w2.data_ptr(), dy.data_ptr(), dgptr, ld, part.data_ptr(), B, S, C, st)
    L.batch_sum(part.data_ptr(), dparams.data_ptr(), 36, B, 36, int(pre is not None), st)
    torch.cuda.synchronize()
    for gd in guards:
        gd()
    if kind == "stride":                                     # the token rows in front of the gps rows were not written
        assert torch.isnan(dgbuf[:, :TOKENS - 2]).all()
    hip = {"out": out, "attn": attn, "score": score, "argmax": argmax, "dy": dy, "dgps": dgps, "mlp.0.weight": dparams[:25],
           "mlp.0.bias": dparams[25:30], "mlp_gps.0.weight": dparams[30:34], "mlp_gps.0.bias": dparams[34:36]}
    hip = {k: v.reshape(r64[k].shape) for k, v in hip.items()}
    return hip, r64, r32, margin


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_head_kernels(kind, B):
    hip, r64, r32, margin = _run_head(kind, B)
    if kind == "tie":
        assert margin == 0.0
    else:
        assert margin >= tr.MARGIN_MIN, margin
    assert torch.equal(hip["argmax"].cpu(), r64["argmax"]) and torch.equal(r32["argmax"], r64["argmax"])
    _compare(f"head {kind} B={B}", hip, r32, r64, keys=[k for k in r64 if k != "argmax"])
    if kind == "edge":
        assert set(r64["argmax"].flatten().tolist()) == {0, C - 1}
    if kind == "tie":
        # the whole max-pool gradient ds of the tied row lands on the LOWER channel, as in torch's fp32 CPU run
        m, t, c0, c1 = TIE
        row = (m * B) * S + t
        assert int(hip["argmax"][0, m * S + t]) == c0
        a, d64, scale = float(r64["attn"][0, m * S + t]), r64["dy"], float(r64["dy"].abs().max())
        ds = float(d64[row, c0] - d64[row, c1]) - a * float(_head_case(kind, B)[3][0, c0] - _head_case(kind, B)[3][0, c1])
        assert abs(ds) >= 1e-3 * scale, (ds, scale)          # a gradient on the wrong channel would be visible
        tol = mr.bar(mr.rel_err(r32["dy"], r64["dy"])) * scale
        for c in (c0, c1):
            assert abs(float(hip["dy"][row, c]) - float(r32["dy"][row, c])) <= 2 * tol, c


def test_head_kernels_are_deterministic():
    a = _run_head("random", 3)[0]
    b = _run_head("random", 3)[0]
    for k in a:
        assert torch.equal(moat.bits(a[k]), moat.bits(b[k])), k


# ---- 2. the module ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _module_case(case):
    B, pseed, iseed = case
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = tr.make_params(pseed)
    ins, dout = tr.make_inputs(B, iseed)
    r64, margin = tr.time_run(p, ins, dout, F64)
    r32, _ = tr.time_run(p, ins, dout, F32)
    return p, ins, dout, r64, r32, margin


def _module(p):
    from deepsense6g_tii_amd.time_mamba import TimeMamba
    m = TimeMamba(device=DEV)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    return m


def _hip_module(m, ins, dout, make_input=_dev):
    m.train()
    m.zero_grad(set_to_none=True)
    xs = {k: make_input(v).requires_grad_(True) for k, v in ins.items()}
    out = m(*(xs[k] for k in tr.IN_KEYS))
    out.backward(_dev(dout))
    res = {"out": out.detach()}
    res.update({"d" + k: xs[k].grad for k in tr.IN_KEYS})
    res.update({k: q.grad for k, q in m.named_parameters()})
    assert len(res) == 18 and all(v is not None for v in res.values())
    return res


@pytest.mark.parametrize("case", tr.CASES)
def test_module(case):
    p, ins, dout, r64, r32, margin = _module_case(case)
    assert margin >= tr.MARGIN_MIN, margin
    hip = _hip_module(_module(p), ins, dout)
    assert set(hip) == set(r64)
    _compare(f"module B={case[0]}", hip, r32, r64)


def test_module_is_deterministic():
    p, ins, dout, _, _, _ = _module_case(tr.CASES[1])
    m = _module(p)
    a = _hip_module(m, ins, dout)
    b = _hip_module(m, ins, dout)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 3. the autograd boundary -----------------------------------------------------------------------------------------
def _strided(t):
    """the same values behind a non-contiguous view"""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=F32, device=DEV)
    wide[..., ::2] = t.to(DEV, F32)
    v = wide[..., ::2]
    assert not v.is_contiguous()
    return v.detach()


def test_non_contiguous_inputs():
    p, ins, dout, _, _, _ = _module_case(tr.CASES[1])
    m = _module(p)
    a = _hip_module(m, ins, dout)
    b = _hip_module(m, ins, dout, make_input=_strided)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_only_some_inputs_require_grad():
    p, ins, dout, _, _, _ = _module_case(tr.CASES[1])
    m = _module(p)
    full = _hip_module(m, ins, dout)
    m.zero_grad(set_to_none=True)
    for q in m.parameters():
        q.requires_grad_(False)
    xs = {k: _dev(v) for k, v in ins.items()}
    xs["lidar"].requires_grad_(True)
    xs["gps"].requires_grad_(True)
    out = m(*(xs[k] for k in tr.IN_KEYS))
    assert out.requires_grad
    out.backward(_dev(dout))
    assert torch.equal(out.detach(), full["out"])
    assert torch.equal(xs["lidar"].grad, full["dlidar"]) and torch.equal(xs["gps"].grad, full["dgps"])
    assert xs["image"].grad is None and xs["radar"].grad is None and all(q.grad is None for q in m.parameters())
    out = m(*(_dev(ins[k]) for k in tr.IN_KEYS))             # nothing requires a gradient: no tape
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out, full["out"])


def test_eval_and_no_grad_keep_no_tape():
    p, ins, dout, _, _, _ = _module_case(tr.CASES[0])
    m = _module(p)
    full = _hip_module(m, ins, dout)
    xs = [_dev(ins[k]).requires_grad_(True) for k in tr.IN_KEYS]
    with torch.no_grad():
        quiet = m(*xs)
    m.eval()
    ev = m(*xs)
    for o in (quiet, ev):
        assert not o.requires_grad and o.grad_fn is None and torch.equal(o, full["out"])
    with pytest.raises(RuntimeError):
        m(*[x.detach().cpu() for x in xs])
    with pytest.raises(ValueError):
        m(xs[0][:, :4], xs[1][:, :4], xs[2][:, :4], xs[3])   # 4 frames
    with pytest.raises(ValueError):
        m(xs[0].double(), xs[1], xs[2], xs[3])


def test_functional_pair_reproduces_the_node():
    from deepsense6g_tii_amd import time_mamba as tm
    p, ins, dout, _, _, _ = _module_case(tr.CASES[1])
    B = tr.CASES[1][0]
    m = _module(p)
    full = _hip_module(m, ins, dout)
    ws = m.mamba._workspace(torch.device(DEV), 3 * B, S)
    rows = torch.cat([_dev(ins[k]) for k in tr.IN_KEYS[:3]], 0).view(3 * B * S, C)
    # the gps rows as the last two token rows of a (B, 7, 512) buffer, addressed by sample stride
    tokens = torch.full((B, TOKENS, C), float("nan"), dtype=F32, device=DEV)
    tokens[:, TOKENS - 2:] = _dev(ins["gps"])
    gps = tokens[:, TOKENS - 2:]
    with torch.no_grad():
        out, tape = tm.time_mamba_forward(m, ws, True, rows, gps, TOKENS * C, B)
        drows, dgps, grads = tm.time_mamba_backward(m, ws, tape, _dev(dout), gps, TOKENS * C, B)
        out2, tape2 = tm.time_mamba_forward(m, ws, False, rows, gps, TOKENS * C, B)
    assert tape2 is None and torch.equal(out2, out) and torch.equal(out, full["out"])
    d = drows.view(3, B, S, C)
    for i, k in enumerate(tr.IN_KEYS[:3]):
        assert torch.equal(d[i], full["d" + k]), k
    assert torch.equal(dgps, full["dgps"])
    names = [n for n, _ in m.named_parameters()]
    by_param = {id(q): n for n, q in m.named_parameters()}
    assert len(grads) == 13
    for q, g in zip(m._params(), grads):
        assert by_param[id(q)] in names and torch.equal(g, full[by_param[id(q)]]), by_param[id(q)]
