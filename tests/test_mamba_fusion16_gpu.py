"""GPU parity of the Mamba fusion block and walk-form stage on bf16 / f16 storage (ds6g_h16_sample_layernorm_* /
ds6g_h16_bimamba_gate_* / ds6g_h16_pool_swap_tokens_* of csrc/mamba_fusion.hip, the 16-bit branch of
deepsense6g_tii_amd/mamba_fusion.py).  Rules and helpers are tests/test_mamba16_gpu.py's:

  kernels   inputs are rounded to the type the kernel reads, the reference is fp64 on those; a 16-bit output holds
            |hip - ref| <= u16 |ref| + bar32 max|ref| elementwise, an fp32 output max|hip - ref| / max|ref| <= bar32 =
            max(10 e_32, 1e-5).  Operands sit in NaN moats, outputs in 0xFF moats.
  block,    e_hip <= 3 e_round + bar32 per tensor (max norm), e_round = the error of tests/mamba_fusion16_ref.py's rounded
  stage     restatement against the unrounded fp64 run.  Conditions (asserted; the seeds were picked on the CPU): LeakyReLU
            margin >= KINK_MIN on the rounded restatement's pre-store f2 in every block, every compared reference tensor
            non-zero, e_round > 0 (but for the stage's ln_f.bias gradient, which no 16-bit tensor reaches: e_round == 0 there).
The table is printed (pytest -s); the committed copy is profiles/mamba_stage16_parity.txt."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from tests import mamba16_ref as m16
from tests import mamba_fusion16_ref as f16r
from tests import mamba_fusion_ref as fr
from tests import mamba_ref as mr
from tests import moat
from tests import test_mamba16_gpu as t16
from tests.test_mamba_stage_walk_gpu import _stage_ref

pytestmark = pytest.mark.gpu

DEV, F32, F64 = t16.DEV, t16.F32, t16.F64
DTYPES, U16, ST = t16.DTYPES, t16.U16, t16.ST
_rd, _in, _out, _name = t16._rd, t16._in, t16._out, t16._name


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


def _lib():
    from deepsense6g_tii_amd._lib import lib
    return lib()


def _st():
    return _ops()._stream()


# ---- 1. the sample LayerNorm alone ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sln_case(dtype, B, T, C, offset):
    g = torch.Generator().manual_seed(B * 1000 + T + C + int(offset))
    n = T * C
    x = _rd(offset + torch.randn(B, n, generator=g, dtype=F64), dtype)
    gam, bet = _rd(1 + mr._uniform(g, (n,), 0.5), F32), _rd(mr._uniform(g, (n,), 0.5), F32)
    dy = _rd(torch.randn(B, n, generator=g, dtype=F64), dtype)

    def run(dt):
        xs, gs, bs = (t.to(dt).clone().requires_grad_(True) for t in (x, gam, bet))
        y = F.layer_norm(xs, (n,), gs, bs, 1e-5)
        (y * dy.to(dt)).sum().backward()
        mean = xs.detach().mean(1)
        return {"y": y.detach(), "dx": xs.grad, "dgamma": gs.grad, "dbeta": bs.grad, "mean": mean,
                "rstd": (xs.detach().var(1, unbiased=False) + 1e-5).rsqrt()}
    return x, gam, bet, dy, run(F64), run(F32)


@pytest.mark.parametrize("B,T,C,offset", [(2, 3, 64, 0.0), (3, 194, 64, 0.0), (2, 10, 512, 0.0), (2, 194, 64, 30.0)])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_sample_layernorm_kernel(dtype, B, T, C, offset):
    ops, lib = _ops(), _lib()
    x64, gam, bet, dy64, r64, r32 = _sln_case(dtype, B, T, C, offset)
    n = T * C
    if offset:      # the variance must not cancel: it is O(1) beside a mean of 30
        assert float(r64["rstd"].min()) > 0.5 and float(r64["mean"].abs().min()) > 29
    x, g_x = _in(x64, dtype, "x")
    ga, g_ga = _in(gam, F32, "gamma")
    be, g_be = _in(bet, F32, "beta")
    dy, g_dy = _in(dy64, dtype, "dy")
    y, g_y = _out((B, n), dtype, "y")
    dx, g_dx = _out((B, n), dtype, "dx")
    mean, g_m = _out((B,), F32, "mean")
    rstd, g_r = _out((B,), F32, "rstd")
    dg, g_dg = _out((n,), F32, "dgamma")
    db, g_db = _out((n,), F32, "dbeta")
    gen = torch.Generator().manual_seed(3)
    pre = [torch.randn(n, generator=gen) for _ in range(2)]
    dg2, g_dg2 = moat.embed(pre[0].to(DEV), t16.MOAT, t16.MOAT, 0xFF, "dgamma (accumulate)")
    db2, g_db2 = moat.embed(pre[1].to(DEV), t16.MOAT, t16.MOAT, 0xFF, "dbeta (accumulate)")
    ws = moat.moat_workspace(ops, int(lib.sample_layernorm_workspace_bytes(B, n)), 0xFF, DEV)
    lib.h16_sample_layernorm_fwd(ST[dtype], x.data_ptr(), ga.data_ptr(), be.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                 rstd.data_ptr(), B, n, 1e-5, ws.ptr, ws.nbytes, _st())
    # the backward reads the statistics out of NaN moats of their own
    mean_r, g_mr = moat.embed(mean.clone(), t16.MOAT, t16.MOAT, "nan", "mean (read)")
    rstd_r, g_rr = moat.embed(rstd.clone(), t16.MOAT, t16.MOAT, "nan", "rstd (read)")
    for acc, (a, b) in ((0, (dg, db)), (1, (dg2, db2))):
        lib.h16_sample_layernorm_bwd(ST[dtype], dy.data_ptr(), x.data_ptr(), mean_r.data_ptr(), rstd_r.data_ptr(),
                                     ga.data_ptr(), dx.data_ptr(), a.data_ptr(), b.data_ptr(), B, n, acc, ws.ptr, ws.nbytes,
                                     _st())
    torch.cuda.synchronize()
    for g in (g_x, g_ga, g_be, g_dy, g_y, g_dx, g_m, g_r, g_dg, g_db, g_dg2, g_db2, g_mr, g_rr, ws.guard):
        g()
    tag = f"sample-LN {_name(dtype)} B={B} T={T} C={C} off={offset:g}"
    hip = {"y": y, "dx": dx, "dgamma": dg, "dbeta": db, "mean": mean, "rstd": rstd}
    t16._gate(tag, hip, r32, r64, dtype, out16=("y", "dx"))
    acc64 = {"dgamma": r64["dgamma"] + pre[0].double(), "dbeta": r64["dbeta"] + pre[1].double()}
    acc32 = {"dgamma": r32["dgamma"] + pre[0], "dbeta": r32["dbeta"] + pre[1]}
    t16._gate(tag + " accumulate", {"dgamma": dg2, "dbeta": db2}, acc32, acc64, dtype, out16=())


# ---- 2. the gate alone ------------------------------------------------------------------------------------------------
def _halfc(t, dtype, right, name, out=False):
    """`t` [M, C] as one column half of a [M, 2 C] buffer (NaN inside NaN moats, or an output inside 0xFF moats) ->
    (the half's view, the buffer, guard)"""
    M, C = t.shape
    if out:
        buf, g = _out((M, 2 * C), dtype, name)
    else:
        full = torch.full((M, 2 * C), float("nan"), dtype=F64)
        (full[:, C:] if right else full[:, :C]).copy_(t)
        buf, g = _in(full, dtype, name)
    return (buf[:, C:] if right else buf[:, :C]), buf, g


def _gate_ref(t, B, L, C):
    fm, bm, f2 = (t[k].reshape(B, L, C) for k in ("fm", "bm", "f2"))
    return (bm.flip(1) * F.leaky_relu(f2.flip(1), 0.2) + fm * bm.flip(1)).reshape(B * L, C)


@functools.lru_cache(maxsize=None)
def _gate_case(dtype, L, C):
    B = 2
    g = torch.Generator().manual_seed(40 + L + C)
    inputs = {k: _rd(torch.randn(B * L, C, generator=g, dtype=F64), dtype) for k in ("fm", "bm", "f2")}
    dout = _rd(torch.randn(B * L, C, generator=g, dtype=F64), dtype)
    fn = lambda t: _gate_ref(t, B, L, C)                          # noqa: E731
    return inputs, dout, t16._grads(fn, inputs, dout, F64), t16._grads(fn, inputs, dout, F32)


def _run_gate(lib, dtype, B, L, C, inputs, dout):
    M = B * L
    ops_in = {k: _halfc(inputs[k], dtype, i % 2 == 1, k) for i, k in enumerate(("fm", "bm", "f2"))}
    do = _halfc(dout, dtype, True, "dout")
    outs = {k: _halfc(torch.empty(M, C), dtype, i % 2 == 0, k, out=True) for i, k in enumerate(("out", "dfm", "dbm", "df2"))}
    keep = {k: moat.bits(v[1][:, :C] if v[0].data_ptr() != v[1].data_ptr() else v[1][:, C:]).clone() for k, v in outs.items()}
    a = lambda k: (ops_in[k][0].data_ptr(), 2 * C)                # noqa: E731
    o = lambda k: (outs[k][0].data_ptr(), 2 * C)                  # noqa: E731
    lib.h16_bimamba_gate_fwd(ST[dtype], *a("fm"), *a("bm"), *a("f2"), *o("out"), B, L, C, _st())
    lib.h16_bimamba_gate_bwd(ST[dtype], do[0].data_ptr(), 2 * C, *a("fm"), *a("bm"), *a("f2"), *o("dfm"), *o("dbm"), *o("df2"),
                             B, L, C, _st())
    torch.cuda.synchronize()
    for v in (*ops_in.values(), do, *outs.values()):
        v[2]()
    for k, v in outs.items():                                     # the other column half is not touched
        other = v[1][:, :C] if v[0].data_ptr() != v[1].data_ptr() else v[1][:, C:]
        assert torch.equal(moat.bits(other), keep[k]), k
    return {"y": outs["out"][0], "dfm": outs["dfm"][0], "dbm": outs["dbm"][0], "df2": outs["df2"][0]}


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gate_kernel(dtype, L, C):
    lib = _lib()
    B = 2
    inputs, dout, r64, r32 = _gate_case(dtype, L, C)
    f2 = inputs["f2"].abs()
    assert float(f2.min()) >= fr.KINK_MIN * float(f2.max())       # the kink is a condition on the drawn input
    hip = _run_gate(lib, dtype, B, L, C, inputs, dout)
    t16._gate(f"gate {_name(dtype)} L={L} C={C}", hip, r32, r64, dtype, out16=("y", "dfm", "dbm", "df2"))
    # a one-hot dout at (b, t) lands in dfm row t and in dbm / df2 row L - 1 - t only
    for b, t in ((0, 0), (1, L - 1), (1, L // 2)):
        hot = torch.zeros(B * L, C, dtype=F64)
        hot[b * L + t] = 1.0
        h = _run_gate(lib, dtype, B, L, C, inputs, hot)
        for k, row in (("dfm", b * L + t), ("dbm", b * L + L - 1 - t), ("df2", b * L + L - 1 - t)):
            nz = (h[k].float() != 0).any(1).nonzero().flatten().tolist()
            assert nz == [row], (k, b, t, nz)


# ---- 3. the pool-swap pack and its backward ---------------------------------------------------------------------------------
POOL_CASES = [(64, 64, 1, 2), (128, 32, 2, 1), (256, 16, 5, 1), (512, 8, 1, 3)]     # (C, H, S, B)


def _pack_ref(feats, gemb, pos, S, mask=None):
    pooled = [F.adaptive_avg_pool2d(f.permute(0, 3, 1, 2), 8) for f in feats]
    tok = pos + fr.swap_pack_ref(*pooled, gemb, S)
    return tok if mask is None else tok * mask


@functools.lru_cache(maxsize=None)
def _pool_case(dtype, C, H, S, B):
    g = torch.Generator().manual_seed(60 + C + H + S)
    T = 192 * S + 2
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)       # noqa: E731
    x = {f"feat{m}": _rd(rn(B * S, H, H, C), dtype) for m in range(3)}
    x["gemb"], x["pos"] = _rd(rn(B, 2, C), F32), _rd(rn(T, C), F32)
    dtok = _rd(rn(B, T, C), dtype)
    din = [_rd(rn(B * S, H, H, C), dtype) for _ in range(3)]
    return x, dtok, din


def _pool_ref(x, dtok, S, dt, mask=None):
    xs = {k: v.to(dt).clone().requires_grad_(True) for k, v in x.items()}
    tok = _pack_ref([xs[f"feat{m}"] for m in range(3)], xs["gemb"], xs["pos"], S, None if mask is None else mask.to(dt))
    (tok * dtok.to(dt)).sum().backward()
    res = {"tokens": tok.detach(), "dgemb": xs["gemb"].grad, "dpos": xs["pos"].grad}
    res.update({f"dfeat{m}": xs[f"feat{m}"].grad for m in range(3)})
    return res


def _run_pool(dtype, x, dtok, S, B, C, H, din=None, alias=False, drop=(0.0, 0, 0), dpos_pre=None):
    """-> (hip results, guards) of one forward and one backward through the wrappers on moated operands"""
    ops = _ops()
    T = 192 * S + 2
    guards = []

    def rd(t, dt, name):
        v, g = _in(t, dt, name)
        guards.append(g)
        return v

    def wr(shape, dt, name):
        v, g = _out(shape, dt, name)
        guards.append(g)
        return v
    feats = [rd(x[f"feat{m}"], dtype, f"feat{m}") for m in range(3)]
    gemb, pos = rd(x["gemb"], F32, "gemb"), rd(x["pos"], F32, "pos_emb")
    tok = wr((B, T, C), dtype, "tokens")
    ops.pool_swap_tokens_fwd(feats, gemb, pos.data_ptr(), tok, S, *drop)
    d = rd(dtok, dtype, "dtokens")
    dgemb = wr((B, 2, C), F32, "dgemb")
    if dpos_pre is None:
        dpos = wr((T, C), F32, "dpos")
    else:
        dpos, g = moat.embed(dpos_pre.to(DEV, F32), t16.MOAT, t16.MOAT, 0xFF, "dpos (accumulate)")
        guards.append(g)
    if din is None:
        dins, douts = None, [wr((B * S, H, H, C), dtype, f"dfeat{m}") for m in range(3)]
    elif alias:
        douts = []
        for m in range(3):
            v, g = moat.embed(din[m].to(dtype).to(DEV), t16.MOAT, t16.MOAT, 0xFF, f"dfeat{m} (in place)")
            guards.append(g)
            douts.append(v)
        dins = douts
    else:
        dins = [rd(din[m], dtype, f"dfeat_in{m}") for m in range(3)]
        douts = [wr((B * S, H, H, C), dtype, f"dfeat{m}") for m in range(3)]
    ops.pool_swap_tokens_bwd(d, dins, douts, dgemb, dpos.data_ptr(), dpos_pre is not None, S, *drop)
    torch.cuda.synchronize()
    for g in guards:
        g()
    res = {"tokens": tok, "dgemb": dgemb, "dpos": dpos}
    res.update({f"dfeat{m}": douts[m] for m in range(3)})
    return res


@pytest.mark.parametrize("C,H,S,B", POOL_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_pool_swap_pair(dtype, C, H, S, B):
    x, dtok, din = _pool_case(dtype, C, H, S, B)
    r64, r32 = _pool_ref(x, dtok, S, F64), _pool_ref(x, dtok, S, F32)
    out16 = ("tokens", "dfeat0", "dfeat1", "dfeat2")
    tag = f"pool-swap {_name(dtype)} C={C} H={H} S={S} B={B}"
    gen = torch.Generator().manual_seed(9)
    pre = torch.randn(192 * S + 2, C, generator=gen)
    hip = _run_pool(dtype, x, dtok, S, B, C, H, dpos_pre=pre)     # dfeat_in null, dpos_emb accumulating onto non-zero
    acc = lambda r, p: {**r, "dpos": r["dpos"] + p}                # noqa: E731
    t16._gate(tag + " in=null", hip, acc(r32, pre), acc(r64, pre.double()), dtype, out16)
    add = lambda r, dt: {**r, **{f"dfeat{m}": r[f"dfeat{m}"] + din[m].to(dt) for m in range(3)}}   # noqa: E731
    a = _run_pool(dtype, x, dtok, S, B, C, H, din=din)
    t16._gate(tag + " in=distinct", a, add(r32, F32), add(r64, F64), dtype, out16)
    b = _run_pool(dtype, x, dtok, S, B, C, H, din=din, alias=True)
    for k in a:
        assert torch.equal(moat.bits(a[k]), moat.bits(b[k])), k   # in place == out of place, to the bit


def _seg(c, C):
    return 0 if c < C // 3 else (1 if c < C // 3 * 2 else 2)


@pytest.mark.parametrize("C,H,S,B", POOL_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_pool_swap_one_hot_probes_land_exactly(dtype, C, H, S, B):
    """ones at the channels around the two cuts and their 8-group neighbours, at the first and last pixel of the first and last
    window of each map: each lands as exactly 1 / k^2 (a power of two) in the token row of its segment, and back"""
    T, k = 192 * S + 2, H // 8
    s1, s2 = C // 3, C // 3 * 2
    chans = {s1 - 1, s1, s2 - 1, s2, C - 1, 0}
    for cut in (s1, s2):
        g8 = cut // 8 * 8
        chans |= {g8 - 1, g8, g8 + 7, g8 + 8}
    chans = sorted(c for c in chans if 0 <= c < C)
    pix = sorted({(0, 0), (k - 1, k - 1), (H - k, H - k), (H - 1, H - 1)})
    z = lambda *s: torch.zeros(*s, dtype=F64)                      # noqa: E731
    x = {f"feat{m}": z(B * S, H, H, C) for m in range(3)}
    x["gemb"], x["pos"] = z(B, 2, C), z(T, C)
    want_tok, dtok = z(B, T, C), z(B, T, C)
    want_df = [z(B * S, H, H, C) for _ in range(3)]
    for q in range(3):
        for i, c in enumerate(chans):
            b, f = (i + q) % B, (i * 2 + q) % S
            m = (q - _seg(c, C)) % 3                               # the token modality channel c of map q goes to
            for (r, u) in pix:
                x[f"feat{q}"][b * S + f, r, u, c] = 1.0
                row = (m * S + f) * 64 + (r // k) * 8 + u // k
                want_tok[b, row, c] += 1.0 / (k * k)
            # backward: a one at that token row's first and last window comes back over the k x k pixels of map q
            for hw in (0, 63):
                dtok[b, (m * S + f) * 64 + hw, c] = 1.0
                r0, u0 = hw // 8 * k, hw % 8 * k
                want_df[q][b * S + f, r0:r0 + k, u0:u0 + k, c] += 1.0 / (k * k)
    hip = _run_pool(dtype, x, dtok, S, B, C, H)
    assert torch.equal(hip["tokens"].double().cpu(), want_tok)
    for q in range(3):
        assert torch.equal(hip[f"dfeat{q}"].double().cpu(), want_df[q]), q
    assert float(hip["dgemb"].abs().max()) == 0.0
    assert torch.equal(hip["dpos"].double().cpu(), dtok.sum(0))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_pool_swap_dropout_pattern_and_backward(dtype):
    ops = _ops()
    C, H, S, B = POOL_CASES[1]
    T, p, seed, off = 192 * S + 2, 0.1, 1234, (1 << 32) + 12345
    x, dtok, _ = _pool_case(dtype, C, H, S, B)
    ones = torch.ones(B, T, C, dtype=F32, device=DEV)
    keep = (ops.dropout(ones, p, seed, off) != 0).cpu()           # the mask of ops.dropout on the same shape and counter
    assert 0.85 < keep.float().mean() < 0.95
    scale = 1.0 / (1.0 - float(torch.tensor(p, dtype=F32)))
    mask = keep.double() * scale
    hip = _run_pool(dtype, x, dtok, S, B, C, H, drop=(p, seed, off))
    assert torch.equal((hip["tokens"].float() != 0).cpu(), keep)  # no kept element is exactly zero on this input
    r64, r32 = _pool_ref(x, dtok, S, F64, mask), _pool_ref(x, dtok, S, F32, mask)
    t16._gate(f"pool-swap {_name(dtype)} dropout p={p}", hip, r32, r64, dtype, ("tokens", "dfeat0", "dfeat1", "dfeat2"))
    # (r64 carries the mask through autograd: its dfeat / dgemb / dpos ARE the plain backward of the masked, scaled gradient)


# ---- 4. the block -----------------------------------------------------------------------------------------------------
BLOCK16_CASES = [(64, 194, 2, 1), (512, 10, 2, 1)]               # (C, T, B, seed)


@functools.lru_cache(maxsize=None)
def _block_case(dtype, C, T, B, seed):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: _rd(v, F32) for k, v in fr.make_block_params(C, T, seed=seed).items()}
    x, dout = (_rd(t, dtype) for t in fr.make_block_input(C, B, T, seed=seed))
    r64, _ = fr.block_run(p, x, dout, F64)
    r32, _ = fr.block_run(p, x, dout, F32)
    rr, margin = f16r.block_run16(p, x, dout, m16.rounder(dtype))
    return p, x, dout, r64, r32, rr, margin


def _block(p, C, T):
    from deepsense6g_tii_amd.mamba_fusion import MambaBlock
    blk = MambaBlock(C, (T, C), 16, 4, 2, device=DEV)
    blk.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    return blk.train()


def _hip_block(blk, x, dout, dtype):
    for q in blk.parameters():
        q.grad = None
    xd, g_x = _in(x, dtype, "x")
    dd, g_d = _in(dout, dtype, "dout")
    xd.requires_grad_(True)
    out = blk(xd)
    out.backward(dd)
    torch.cuda.synchronize()
    g_x()
    g_d()
    assert out.dtype == dtype and xd.grad.dtype == dtype
    res = {"out": out.detach(), "input": xd.grad}
    res.update({k: q.grad for k, q in blk.named_parameters()})
    assert len(res) == 26 and all(v.dtype == F32 for k, v in res.items() if k not in ("out", "input"))
    return res


def _compare16(tag, hip, r64, r32, rr):
    bad = []
    print()
    for k in r64:
        assert r64[k].abs().max() > 0, k
        e_hip, e_round, b32 = mr.rel_err(hip[k], r64[k]), mr.rel_err(rr[k], r64[k]), mr.bar(mr.rel_err(r32[k], r64[k]))
        # ln_f.bias' gradient is the column sum of dxo, which depends on no 16-bit tensor but the given output gradients:
        # the rounded restatement has it exactly, and the bar is the fp32 bar alone
        assert (e_round > 0) != (k == "ln_f.bias"), (k, e_round)
        bar = 3 * e_round + b32
        print(f"parity16 {tag:<38s} {k:<48s} e_hip {e_hip:.3e}  e_round {e_round:.3e}  ratio {e_hip / e_round if e_round else float('nan'):5.2f}  "
              f"bar {bar:.3e}")
        if not e_hip <= bar:
            bad.append((k, e_hip, e_round))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("C,T,B,seed", BLOCK16_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_block(dtype, C, T, B, seed):
    from deepsense6g_tii_amd.mamba_fusion import block_backward, block_forward, block_weight_copies16
    p, x, dout, r64, r32, rr, margin = _block_case(dtype, C, T, B, seed)
    assert margin >= fr.KINK_MIN, margin
    blk = _block(p, C, T)
    xf = x.float().to(DEV)
    with torch.no_grad():
        before = blk(xf).clone()                                  # the fp32 path, before any 16-bit call
    hip = _hip_block(blk, x, dout, dtype)
    assert set(hip) == set(r64)
    _compare16(f"block {_name(dtype)} C={C} T={T} B={B}", hip, r64, r32, rr)
    again = _hip_block(blk, x, dout, dtype)                       # two runs are bit-identical
    for k in hip:
        assert torch.equal(moat.bits(hip[k]), moat.bits(again[k])), k
    # the plain functions: returned gradients == the module's; gdst flag 0 the same bits, flag 1 accumulates; w16= the same bits
    params = [q.detach() for q in blk._params()]
    name = {id(q): k for k, q in blk.named_parameters()}
    order = [name[id(q)] for q in blk._params()]
    ws = blk._workspace(torch.device(DEV), B, T)
    x2, d2 = x.to(dtype).reshape(B, T * C).to(DEV), dout.to(dtype).reshape(B * T, C).to(DEV)
    out, tape = block_forward(blk, ws, True, x2, B, T, params)
    dx0, g0 = block_backward(blk, ws, tape, d2, B, T, params)
    assert torch.equal(moat.bits(out.view(B, T, C)), moat.bits(hip["out"])) and \
        torch.equal(moat.bits(dx0.view(B, T, C)), moat.bits(hip["input"]))
    for k, g in zip(order, g0):
        assert g.dtype == F32 and torch.equal(g, hip[k]), k
    gen = torch.Generator().manual_seed(5)
    for acc in (0, 1):
        pre = [torch.randn(g.shape, generator=gen).to(DEV) for g in g0]
        dst = [t.clone() if acc else torch.full_like(t, float("nan")) for t in pre]
        dx, none = block_backward(blk, ws, tape, d2, B, T, params, gdst=[(t.data_ptr(), acc) for t in dst])
        assert none is None and torch.equal(moat.bits(dx), moat.bits(dx0))
        for k, t, g, s in zip(order, dst, g0, pre):
            if not acc:
                assert torch.equal(t, g), k
            else:
                assert mr.rel_err(t, s.double().cpu() + g.double().cpu()) <= 1e-5, k
    w16, alive = block_weight_copies16(blk, params, dtype)
    out_w, tape_w = block_forward(blk, ws, True, x2, B, T, params, w16=w16)
    dx_w, g_w = block_backward(blk, ws, tape_w, d2, B, T, params, w16=w16)
    assert torch.equal(moat.bits(out_w), moat.bits(out)) and torch.equal(moat.bits(dx_w), moat.bits(dx0))
    for k, a, b in zip(order, g_w, g0):
        assert torch.equal(a, b), k
    with torch.no_grad():
        after = blk(xf)
    assert torch.equal(moat.bits(after), moat.bits(before))       # the fp32 call returns its earlier bits


# ---- 5. the stage -----------------------------------------------------------------------------------------------------
# (C, H, S, B, n_layer, (seed on bf16, seed on f16)): picked on the CPU so that the rounded restatement of that storage meets
# the LeakyReLU margin (about one seed in twenty does at C = 512, where a block draws 2 x 194 x 512 pre-activations)
STAGE16_CASES = [(64, 64, 1, 2, 2, (2, 2)), (512, 8, 1, 2, 2, (5, 47))]


@functools.lru_cache(maxsize=None)
def _stage_case(dtype, C, H, S, B, n_layer, seed):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: _rd(v, F32) for k, v in fr.make_fusion_params(C, S, n_layer, seed=seed, spread=True).items()}
    g = torch.Generator().manual_seed(9700 + seed + C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    x = {f"feat{m}": _rd(rn(B * S, H, H, C), dtype) for m in range(3)}
    x["gemb"] = _rd(rn(B, 2, C), F32)
    d = {f"out{m}": _rd(rn(B * S, H, H, C), dtype) for m in range(3)}
    d["gps_out"] = _rd(rn(B, 2, C), F32)
    r64, _ = _stage_ref(p, x, d, n_layer, S, F64)
    r32, _ = _stage_ref(p, x, d, n_layer, S, F32)
    rr, margin = f16r.stage_run16(p, x, d, n_layer, S, m16.rounder(dtype))
    return p, x, d, r64, r32, rr, margin


def _fusion(C, S, n_layer, p):
    from deepsense6g_tii_amd.mamba_fusion import MambaFusion
    m = MambaFusion(n_embd=C, ln_size=(192 * S + 2, C), d_state=16, d_conv=4, expand=2, n_layer=n_layer, vert_anchors=8,
                    horz_anchors=8, seq_len=S, embd_pdrop=0.0, config=types.SimpleNamespace(n_views=1), device=DEV)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    return m


def _hip_stage(m, x, d, B, dtype, pre=None, ws=None):
    from deepsense6g_tii_amd import mamba_fusion as mf
    ops = _ops()
    S, C, T = m.seq_len, m.n_embd, m.n_tokens
    ws = ws or ops.Workspace(torch.device(DEV), mf.stage_workspace_bytes(m, B))
    dev = lambda t, dt: t.to(dt).contiguous().to(DEV)              # noqa: E731
    feats = [dev(x[f"feat{q}"], dtype) for q in range(3)]
    gemb = dev(x["gemb"], F32)
    outs = [torch.full_like(f, float("nan")) for f in feats]
    xo, tape = mf.stage_forward(m, ws, True, feats, gemb, outs, B)
    assert xo.dtype == F32 and all(o.dtype == dtype for o in outs)
    grads = {k: (dev(pre[k], F32) if pre is not None else torch.full_like(q, float("nan"))) for k, q in m.named_parameters()}
    slot = {id(q): (grads[k].data_ptr(), int(pre is not None)) for k, q in m.named_parameters()}
    douts = [dev(d[f"out{q}"], dtype) for q in range(3)]
    dfeats = [torch.full_like(f, float("nan")) for f in feats]
    dgemb = torch.full_like(gemb, float("nan"))
    mf.stage_backward(m, ws, tape, douts, (dev(d["gps_out"], F32), False), dfeats, dgemb, B, lambda q: slot[id(q)])
    torch.cuda.synchronize()
    res = {f"out{q}": outs[q] for q in range(3)}
    res["gps_out"] = xo.view(B, T, C)[:, T - 2:]
    res.update({f"dfeat{q}": dfeats[q] for q in range(3)})
    res["dgemb"] = dgemb
    res.update(grads)
    return res


@pytest.mark.parametrize("C,H,S,B,n_layer,seeds", STAGE16_CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_stage(dtype, C, H, S, B, n_layer, seeds):
    from deepsense6g_tii_amd import mamba_fusion as mf
    seed = seeds[DTYPES.index(dtype)]
    p, x, d, r64, r32, rr, margin = _stage_case(dtype, C, H, S, B, n_layer, seed)
    assert margin >= fr.KINK_MIN, margin
    m = _fusion(C, S, n_layer, p)
    before = _hip_stage(m, x, d, B, F32)                          # the fp32 stage on the same objects, before any 16-bit call
    hip = _hip_stage(m, x, d, B, dtype)
    assert set(hip) == set(r64) and len(hip) == 8 + 3 + 24 * n_layer
    _compare16(f"stage {_name(dtype)} C={C} H={H} L={n_layer}", hip, r64, r32, rr)
    again = _hip_stage(m, x, d, B, dtype)
    for k in hip:
        assert torch.equal(moat.bits(hip[k]), moat.bits(again[k])), k
    after = _hip_stage(m, x, d, B, F32)
    for k in before:
        assert torch.equal(moat.bits(before[k]), moat.bits(after[k])), k
    if C == 64:                                                   # gradients accumulate onto existing ones; a short workspace
        g = torch.Generator().manual_seed(5)
        pre = {k: torch.randn(v.shape, generator=g, dtype=F64) for k, v in p.items()}
        acc = _hip_stage(m, x, d, B, dtype, pre=pre)
        names = list(p)
        _compare16("stage accumulate " + _name(dtype), {k: acc[k] for k in names}, {k: r64[k] + pre[k] for k in names},
                   {k: r32[k] + pre[k].float() for k in names}, {k: rr[k] + pre[k] for k in names})
        short = _ops().Workspace(torch.device(DEV), mf.stage_workspace_bytes(m, B) - 1)
        feats = [x[f"feat{q}"].to(dtype).to(DEV) for q in range(3)]
        with pytest.raises(ValueError, match="workspace"):
            mf.stage_forward(m, short, False, feats, x["gemb"].float().to(DEV), [torch.empty_like(f) for f in feats], B)
