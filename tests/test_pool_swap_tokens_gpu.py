"""GPU tests of the NHWC token pack of the Mamba stage (ds6g_pool_swap_tokens_fwd / _bwd, csrc/mamba_fusion.hip).

Reference: a torch composition in fp64, built here: adaptive_avg_pool2d of the three maps, the channel swap written as slice
assignments, pos_emb.  Yardstick: the same composition in fp32 on the CPU.  The bar is the project's rule
    e_hip <= max(10 * e_32, 1e-5),   e = max|x - ref64| / max|ref64|   (tests/mamba_ref.rel_err / bar),
with e_32 computed in the test.  Every operand sits in NaN moats and every output in 0xFF moats (tests/moat.py).

The one-hot probes are exact: a single 1.0 in one map must produce exactly one non-zero token element, 1 / (H/8)^2 (a power
of two), in the predicted row and channel, and the backward must return a one-hot token gradient to exactly the window it
came from.  The probed channels sit on both sides of the two segment cuts (C//3 and 2 (C//3), never multiples of 4 here), so
the float4 groups that straddle a cut are all covered."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import mamba_ref as mr
from tests import moat

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
F64 = torch.float64
MOAT = moat.MIN_MOAT
SHAPES = [(64, 64, 1, 2), (128, 32, 2, 1), (256, 16, 5, 1), (512, 8, 1, 3)]     # (C, H, S, B)


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


def _in(t):
    """operand on the device inside NaN moats -> (view, guard)"""
    return moat.embed(t.to(DEV, F32).contiguous(), MOAT, MOAT, "nan")


def _out(*shape):
    """NaN-filled output on the device inside 0xFF moats -> (view, guard)"""
    return moat.embed(torch.full(shape, float("nan"), dtype=F32, device=DEV), MOAT, MOAT, 0xFF)


def _seg_bounds(C):
    s1 = C // 3
    return [(0, s1), (s1, 2 * s1), (2 * s1, C)]


def _pack_ref(maps, gemb, pos, S):
    """maps: three [B*S, H, H, C] (NHWC), gemb [B, 2, C], pos [T, C] -> tokens [B, T, C], in the operands' dtype"""
    N, H, _, C = maps[0].shape
    B = N // S
    pooled = [F.adaptive_avg_pool2d(m.permute(0, 3, 1, 2), 8).permute(0, 2, 3, 1).reshape(B, S * 64, C) for m in maps]
    body = []
    for m in range(3):
        t = torch.empty_like(pooled[0])
        for j, (lo, hi) in enumerate(_seg_bounds(C)):
            t[:, :, lo:hi] = pooled[(m + j) % 3][:, :, lo:hi]
        body.append(t)
    return torch.cat(body + [gemb], 1) + pos


@functools.lru_cache(maxsize=None)
def _case(C, H, S, B):
    """seeded operands (fp64) and the fp64 / fp32 forward + backward references, computed once per shape"""
    g = torch.Generator().manual_seed(1000 + C + H + S + B)
    T = 192 * S + 2
    x = {"map0": torch.randn(B * S, H, H, C, generator=g, dtype=F64), "map1": torch.randn(B * S, H, H, C, generator=g, dtype=F64),
         "map2": torch.randn(B * S, H, H, C, generator=g, dtype=F64), "gemb": torch.randn(B, 2, C, generator=g, dtype=F64),
         "pos": torch.randn(T, C, generator=g, dtype=F64)}
    dtok = torch.randn(B, T, C, generator=g, dtype=F64)
    din = [torch.randn(B * S, H, H, C, generator=g, dtype=F64) for _ in range(3)]
    dpos0 = torch.randn(T, C, generator=g, dtype=F64)
    refs = []
    for dt in (F64, F32):
        v = {k: t.to(dt).clone().requires_grad_(True) for k, t in x.items()}
        tok = _pack_ref([v["map0"], v["map1"], v["map2"]], v["gemb"], v["pos"], S)
        (tok * dtok.to(dt)).sum().backward()
        r = {"tokens": tok.detach(), "dgemb": v["gemb"].grad, "dpos_emb": v["pos"].grad + dpos0.to(dt)}
        for q in range(3):
            r[f"dfeat{q}"] = v[f"map{q}"].grad + din[q].to(dt)
        refs.append(r)
    for k, t in refs[0].items():
        assert t.abs().max() > 0, k
    return x, dtok, din, dpos0, refs[0], refs[1]


def _compare(tag, hip, r32, r64):
    bad = []
    print()
    for k in r64:
        e32, eh = mr.rel_err(r32[k], r64[k]), mr.rel_err(hip[k], r64[k])
        print(f"parity {tag:<28s} {k:<10s} e_hip {eh:.3e}  e_32 {e32:.3e}  bar {mr.bar(e32):.3e}")
        if not eh <= mr.bar(e32):
            bad.append((k, eh, e32))
    assert not bad, (tag, bad)


def _fwd(x, S, drop=(0.0, 0, 0)):
    """-> (tokens, guards) of one forward on moated operands"""
    ops = _ops()
    B, _, C = x["gemb"].shape
    ins = {k: _in(t) for k, t in x.items()}
    tok, gt = _out(B, 192 * S + 2, C)
    ops.pool_swap_tokens_fwd([ins[f"map{q}"][0] for q in range(3)], ins["gemb"][0], ins["pos"][0].data_ptr(), tok, S, *drop)
    return tok, [gt] + [g for _, g in ins.values()]


def _bwd(dtok, din, dpos0, S, H, drop=(0.0, 0, 0), inplace=False):
    """-> ({dfeat0..2, dgemb, dpos_emb}, guards); din None: fresh map gradients; dpos0 None: dpos_emb written, else added to"""
    ops = _ops()
    B, T, C = dtok.shape
    d, gd = _in(dtok)
    guards = [gd]
    outs, ins = [], []
    for q in range(3):
        if din is not None and inplace:
            o, go = moat.embed(din[q].to(DEV, F32).contiguous(), MOAT, MOAT, 0xFF)
            i = o
        else:
            o, go = _out(B * S, H, H, C)
            i = None
            if din is not None:
                i, gi = _in(din[q])
                guards.append(gi)
        outs.append(o)
        ins.append(i)
        guards.append(go)
    dg, gg = _out(B, 2, C)
    if dpos0 is None:
        dp, gp = _out(T, C)
    else:
        dp, gp = moat.embed(dpos0.to(DEV, F32).contiguous(), MOAT, MOAT, 0xFF)
    ops.pool_swap_tokens_bwd(d, ins if din is not None else None, outs, dg, dp.data_ptr(), dpos0 is not None, S, *drop)
    res = {f"dfeat{q}": outs[q] for q in range(3)}
    res.update(dgemb=dg, dpos_emb=dp)
    return res, guards + [gg, gp]


@pytest.mark.parametrize("C,H,S,B", SHAPES)
def test_parity_and_determinism(C, H, S, B):
    x, dtok, din, dpos0, r64, r32 = _case(C, H, S, B)
    tok, guards = _fwd(x, S)
    res, g2 = _bwd(dtok, din, dpos0, S, H)                 # dfeat_in given, dpos_emb accumulated onto a non-zero destination
    hip = dict(res, tokens=tok)
    for g in guards + g2:
        g()
    _compare(f"C={C} H={H} S={S} B={B}", hip, r32, r64)
    tok2, _ = _fwd(x, S)                                    # no atomics, fixed order: two runs are bit-identical
    res2, _ = _bwd(dtok, din, dpos0, S, H)
    assert torch.equal(moat.bits(tok), moat.bits(tok2))
    for k in res:
        assert torch.equal(moat.bits(res[k]), moat.bits(res2[k])), k
    # in == out gives the same bits as separate buffers; no dfeat_in and a written dpos_emb = the result minus the addends
    res3, g3 = _bwd(dtok, din, dpos0, S, H, inplace=True)
    for k in res:
        assert torch.equal(moat.bits(res[k]), moat.bits(res3[k])), k
    res4, g4 = _bwd(dtok, None, None, S, H)
    for g in g3 + g4:
        g()
    fresh = {k: (r64[k] - (dpos0 if k == "dpos_emb" else din[int(k[-1])])) for k in r64 if k.startswith("dfeat") or k == "dpos_emb"}
    for k, ref in fresh.items():
        assert mr.rel_err(res4[k], ref) <= 1e-5, k
    assert torch.equal(moat.bits(res4["dgemb"]), moat.bits(res["dgemb"]))


@pytest.mark.parametrize("C,H,S,B", SHAPES)
def test_dropout_is_ops_dropout_of_the_plain_result(C, H, S, B):
    ops = _ops()
    x, dtok, din, dpos0, _, _ = _case(C, H, S, B)
    drop = (0.1, 0x5DEECE66D, (1 << 33) + 12345)            # a counter offset past 2^32
    plain, _ = _fwd(x, S)
    tok, guards = _fwd(x, S, drop)
    for g in guards:
        g()
    want = ops.dropout(plain.contiguous(), *drop)
    assert torch.equal(moat.bits(tok), moat.bits(want))
    kept = (tok != 0).float().mean().item()
    assert 0.85 < kept < 0.95, kept
    # the backward zeroes and scales the same elements: it equals the plain backward of the dropped token gradient
    got, g2 = _bwd(dtok, din, dpos0, S, H, drop)
    for g in g2:
        g()
    want, _ = _bwd(ops.dropout(dtok.to(DEV, F32).contiguous(), *drop).cpu(), din, dpos0, S, H)
    for k in got:
        assert torch.equal(moat.bits(got[k]), moat.bits(want[k])), k


def _probe_points(C, H):
    k = H // 8
    s1 = C // 3
    chans = [s1 - 1, s1, 2 * s1 - 1, 2 * s1, C - 1]
    pix = sorted({(p * k + d, p * k + d) for p in (0, 7) for d in (0, k - 1)})   # first / last pixel of window (0,0) and (7,7)
    return chans, pix


@pytest.mark.parametrize("C,H,S,B", SHAPES)
def test_one_hot_probes_land_exactly(C, H, S, B):
    """forward: one 1.0 in map q -> exactly one token element, 1 / k^2, at the predicted place; backward: the adjoint"""
    ops = _ops()
    k, T = H // 8, 192 * S + 2
    s1 = C // 3
    chans, pix = _probe_points(C, H)
    maps = [torch.zeros(B * S, H, H, C, dtype=F32, device=DEV) for _ in range(3)]
    gemb = torch.zeros(B, 2, C, dtype=F32, device=DEV)
    pos = torch.zeros(T, C, dtype=F32, device=DEV)
    tok = torch.empty(B, T, C, dtype=F32, device=DEV)
    dtok = torch.zeros(B, T, C, dtype=F32, device=DEV)
    dmaps = [torch.empty(B * S, H, H, C, dtype=F32, device=DEV) for _ in range(3)]
    dgemb = torch.empty(B, 2, C, dtype=F32, device=DEV)
    dpos = torch.empty(T, C, dtype=F32, device=DEV)
    n = 0
    for q in range(3):
        for ci, c in enumerate(chans):
            for pi, (h, w) in enumerate(pix):
                b, f = (B - 1, S - 1) if (ci + pi + q) % 2 else (0, 0)
                seg = 0 if c < s1 else (1 if c < 2 * s1 else 2)
                row = (((q - seg) % 3) * S + f) * 64 + (h // k) * 8 + w // k
                maps[q][b * S + f, h, w, c] = 1.0
                ops.pool_swap_tokens_fwd(maps, gemb, pos.data_ptr(), tok, S)
                maps[q][b * S + f, h, w, c] = 0.0
                nz = tok.nonzero().tolist()
                assert nz == [[b, row, c]], (q, c, h, w, nz)
                assert tok[b, row, c].item() == 1.0 / (k * k)
                dtok[b, row, c] = 1.0
                ops.pool_swap_tokens_bwd(dtok, None, dmaps, dgemb, dpos.data_ptr(), False, S)
                dtok[b, row, c] = 0.0
                for m in range(3):
                    nz = dmaps[m].nonzero().tolist()
                    if m != q:
                        assert nz == [], (q, m, c, h, w, nz[:4])
                        continue
                    h0, w0 = h // k * k, w // k * k
                    want = [[b * S + f, hh, ww, c] for hh in range(h0, h0 + k) for ww in range(w0, w0 + k)]
                    assert nz == want, (q, c, h, w, nz[:4])
                    assert bool((dmaps[q][b * S + f, h0:h0 + k, w0:w0 + k, c] == 1.0 / (k * k)).all())
                assert dpos.nonzero().tolist() == [[row, c]] and dpos[row, c].item() == 1.0
                assert not bool(dgemb.any())
                n += 1
    assert n == 3 * 5 * len(pix)


def test_gps_rows_one_hot():
    ops = _ops()
    C, H, S, B = 64, 8, 2, 2
    T = 192 * S + 2
    maps = [torch.zeros(B * S, H, H, C, dtype=F32, device=DEV) for _ in range(3)]
    gemb = torch.zeros(B, 2, C, dtype=F32, device=DEV)
    pos = torch.zeros(T, C, dtype=F32, device=DEV)
    tok = torch.empty(B, T, C, dtype=F32, device=DEV)
    dmaps = [torch.empty(B * S, H, H, C, dtype=F32, device=DEV) for _ in range(3)]
    dgemb = torch.empty(B, 2, C, dtype=F32, device=DEV)
    dpos = torch.empty(T, C, dtype=F32, device=DEV)
    for b, j, c in ((0, 0, 0), (1, 1, C - 1), (1, 0, C // 3)):
        gemb.zero_()
        gemb[b, j, c] = 1.0
        ops.pool_swap_tokens_fwd(maps, gemb, pos.data_ptr(), tok, S)
        assert tok.nonzero().tolist() == [[b, T - 2 + j, c]]
        ops.pool_swap_tokens_bwd(tok, None, dmaps, dgemb, dpos.data_ptr(), False, S)
        assert dgemb.nonzero().tolist() == [[b, j, c]] and not any(bool(d.any()) for d in dmaps)


def test_wrapper_refuses_what_the_kernel_does_not_take():
    ops = _ops()
    from deepsense6g_tii_amd._lib import Ds6gError, lib
    C, H, S, B = 64, 8, 1, 1
    T = 192 * S + 2
    maps = [torch.zeros(B * S, H, H, C, dtype=F32, device=DEV) for _ in range(3)]
    gemb = torch.zeros(B, 2, C, dtype=F32, device=DEV)
    pos = torch.zeros(T, C, dtype=F32, device=DEV)
    tok = torch.empty(B, T, C, dtype=F32, device=DEV)
    with pytest.raises(AssertionError):
        ops.pool_swap_tokens_fwd([m.bfloat16() for m in maps], gemb, pos.data_ptr(), tok, S)
    with pytest.raises(AssertionError):
        ops.pool_swap_tokens_fwd(maps, gemb, pos.data_ptr(), tok[:, :-1].contiguous(), S)
    descs, _, _ = ops._pool_swap_descs(maps, None, S, C)
    descs[1].mod_off = 0                                     # not the layout (m * S * 64) the kernel assumes
    import ctypes
    with pytest.raises(Ds6gError):
        lib().pool_swap_tokens_fwd(ctypes.addressof(descs), gemb.data_ptr(), pos.data_ptr(), tok.data_ptr(), B, S, H, C, 0.0,
                                   0, 0, 0)
