"""The launches taken off the GPT stages' serial chain compute what the launches they replace computed.

Deferred LayerNorm parameter gradients, the single slab sum of the attention backward and the grouped per-modality stage glue
are compared bit for bit (torch.equal) with the per-layer / two-launch / per-map forms on the same operands; the small_linear
kernels (LDS-staged forward, four-lane data gradient) are held to the fp32 dot-product bound that holds for ANY summation order
against an fp64 CPU reference.  Every operand lives inside moats (tests/moat.py): NaN around what is read,
0xFF around what is written.
"""
import zlib

import pytest
import torch

from tests import moat

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DEV = "cuda"
MOAT = moat.MIN_MOAT


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


def _lib():
    from deepsense6g_tii_amd._lib import lib
    return lib()


def _gen(*key):
    g = torch.Generator(device="cpu")
    g.manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()))
    return g


def rnd(g, *shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


class Moats:
    """operands of one case: read() puts a tensor between NaN moats, written() an output (NaN payload unless given) between
    0xFF moats; check() asserts every moat is intact"""

    def __init__(self):
        self.guards = []

    def read(self, t, name="in"):
        v, g = moat.embed(t.to(DEV).contiguous(), MOAT, MOAT, "nan", name)
        self.guards.append(g)
        return v

    def written(self, t, name="out", keep=False):
        t = t.to(DEV).contiguous()
        v, g = moat.embed(t if keep else moat.nan_like(t), MOAT, MOAT, 0xFF, name)
        self.guards.append(g)
        return v

    def check(self):
        torch.cuda.synchronize()
        for g in self.guards:
            g()


# ---- A. deferred LayerNorm parameter gradients ---------------------------------------------------------------------------
LN_M = 37   # three row blocks of 16, ragged tail


def _ln_case(g, C, kind):
    """one LayerNorm backward's operands; kind: 'fresh' | 'acc' (pre-filled dgamma / dbeta) | 'drop' (dx_drop output)"""
    x, dy, add = rnd(g, LN_M, C), rnd(g, LN_M, C), rnd(g, LN_M, C)
    gamma = rnd(g, C) + 1.0
    mean = x.mean(1)
    rstd = (x.var(1, unbiased=False) + 1e-5).rsqrt()
    pre = (rnd(g, C), rnd(g, C)) if kind == "acc" else None
    return dict(x=x, dy=dy, add=add, gamma=gamma, mean=mean, rstd=rstd, pre=pre, drop=(0.1, 77, 1000) if kind == "drop" else None)


def _ln_run(ops, mo, cases, deferred):
    """-> [(dx, dxd or None, dgamma, dbeta)] per case; deferred: partial buffers + ONE batched finalize"""
    outs, items, held = [], [], []
    for c in cases:
        C = c["x"].shape[1]
        x, dy, add = mo.read(c["x"]), mo.read(c["dy"]), mo.read(c["add"])
        gamma, mean, rstd = mo.read(c["gamma"]), mo.read(c["mean"]), mo.read(c["rstd"])
        acc = c["pre"] is not None
        dg = mo.written(c["pre"][0] if acc else torch.empty(C), "dgamma", keep=acc)
        db = mo.written(c["pre"][1] if acc else torch.empty(C), "dbeta", keep=acc)
        dx = mo.written(torch.empty(LN_M, C), "dx")
        kw = dict(add=add, out=dx, drop=c["drop"])
        if deferred:
            nb = ops.layernorm_partial_bytes(LN_M, C)
            assert nb == int(_lib().layernorm_bwd_workspace_bytes(LN_M, C))
            part = moat.moat_workspace(ops, nb, 0xFF)
            held.append(part)
            mo.guards.append(part.guard)
            r = ops.layernorm_bwd(dy, x, mean, rstd, gamma.data_ptr(), 0, 0, None, partial=(part.ptr, nb), **kw)
            items.append((part.ptr, LN_M, C, dg.data_ptr(), db.data_ptr(), acc))
        else:
            ws = moat.moat_workspace(ops, ops.layernorm_partial_bytes(LN_M, C), 0xFF)
            mo.guards.append(ws.guard)
            r = ops.layernorm_bwd(dy, x, mean, rstd, gamma.data_ptr(), dg.data_ptr(), db.data_ptr(), ws, accumulate=acc, **kw)
        dxd = r[1] if c["drop"] is not None else None
        outs.append((dx, dxd, dg, db))
    if deferred:
        ops.layernorm_finalize_batched(items)
    mo.check()
    return outs


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("kinds", [("fresh", "acc", "drop"), ("acc",), ("fresh", "drop", "acc") * 8],
                         ids=["batch3", "batch1", "batch24"])
def test_layernorm_deferred_finalize_is_bit_identical(C, kinds):
    ops = _ops()
    g = _gen("ln", C, len(kinds))
    # a mixed-width batch: the grid is as wide as the widest LayerNorm, narrower ones leave early
    widths = [C if i % 5 else (576 - C) for i in range(len(kinds))] if len(kinds) > 1 else [C]
    cases = [_ln_case(g, w, k) for w, k in zip(widths, kinds)]
    ref = _ln_run(ops, Moats(), cases, deferred=False)
    got = _ln_run(ops, Moats(), cases, deferred=True)
    for i, (r, o) in enumerate(zip(ref, got)):
        for name, a, b in zip(("dx", "dx_drop", "dgamma", "dbeta"), r, o):
            if a is None:
                assert b is None
                continue
            assert not torch.isnan(b).any(), (i, name)
            assert torch.equal(a, b), (i, kinds[i], name, (a - b).abs().max().item())
        if cases[i]["drop"] is not None:
            assert not torch.equal(o[0], o[1])   # the dropout copy really is one


def test_layernorm_deferred_16bit_storage_is_bit_identical():
    """the 16-bit entry point shares the launcher: bf16 dy, bf16 dropout copy"""
    ops = _ops()
    C = 128
    g = _gen("ln16")
    c = _ln_case(g, C, "drop")
    res = []
    for deferred in (False, True):
        mo = Moats()
        x, dy, add = mo.read(c["x"]), mo.read(c["dy"].to(BF16)), mo.read(c["add"])
        gamma, mean, rstd = mo.read(c["gamma"]), mo.read(c["mean"]), mo.read(c["rstd"])
        dg, db = mo.written(torch.empty(C)), mo.written(torch.empty(C))
        nb = ops.layernorm_partial_bytes(LN_M, C)
        ws = moat.moat_workspace(ops, nb, 0xFF)
        mo.guards.append(ws.guard)
        kw = dict(add=add, drop=c["drop"], dtype=BF16)
        if deferred:
            dx, dxd = ops.layernorm_bwd_bf16(dy, x, mean, rstd, gamma.data_ptr(), 0, 0, None, partial=(ws.ptr, nb), **kw)
            ops.layernorm_finalize_batched([(ws.ptr, LN_M, C, dg.data_ptr(), db.data_ptr(), False)])
        else:
            dx, dxd = ops.layernorm_bwd_bf16(dy, x, mean, rstd, gamma.data_ptr(), dg.data_ptr(), db.data_ptr(), ws, **kw)
        mo.check()
        res.append((dx, dxd, dg, db))
    for a, b in zip(*res):
        assert not torch.isnan(b.float()).any() and torch.equal(a, b)


def test_layernorm_deferred_refuses_a_short_partial_buffer():
    from deepsense6g_tii_amd._lib import Ds6gError
    ops = _ops()
    C = 64
    c = _ln_case(_gen("lnshort"), C, "fresh")
    mo = Moats()
    x, dy = mo.read(c["x"]), mo.read(c["dy"])
    gamma, mean, rstd = mo.read(c["gamma"]), mo.read(c["mean"]), mo.read(c["rstd"])
    dx = mo.written(torch.empty(LN_M, C))
    nb = ops.layernorm_partial_bytes(LN_M, C) - 4          # one float short
    part = moat.moat_workspace(ops, nb, 0xFF)
    mo.guards.append(part.guard)
    with pytest.raises(Ds6gError, match="code 3"):
        ops.layernorm_bwd(dy, x, mean, rstd, gamma.data_ptr(), 0, 0, None, out=dx, partial=(part.ptr, nb))
    mo.check()
    assert torch.isnan(dx).all()                                         # nothing was written
    assert bool((part.buf == 0xFF).all())


# ---- B. one slab sum per attention backward ------------------------------------------------------------------------------
MERGED_SUM_OFF = 0x08000000   # ds6g_set_debug_flags: dK/dV and dQ slabs reduced by two launches


def _attn_bwd(ops, B, T, nh, hd, kind, flags):
    """kind: 'f32' | 'bf16out' (fp32 q / k / v / dO, bf16 o and gradients) | 'bf16' / 'f16' (every operand 16-bit)
    -> (dq, dk, dv), slab-sum launches the backward made"""
    L = _lib()
    C, M = nh * hd, B * T
    tin = {"f32": F32, "bf16out": F32, "bf16": BF16, "f16": F16}[kind]
    tout = {"f32": F32, "bf16out": BF16, "bf16": BF16, "f16": F16}[kind]
    fwd, bwd = {"f32": (ops.attention_fwd, ops.attention_bwd), "bf16out": (ops.attention_fwd_bf16out, ops.attention_bwd_bf16),
                "bf16": (ops.attention_fwd_bf16, ops.attention_bwd_bf16io), "f16": (ops.attention_fwd_bf16, ops.attention_bwd_bf16io)}[kind]
    g = _gen("attn", B, T, nh, hd, kind)
    mo = Moats()
    q, k, v, d_o = (mo.read(rnd(g, M, C, dtype=tin, scale=0.5)) for _ in range(4))
    need = int(L.attention_workspace_bytes(B, T, nh, hd, C))
    ws = moat.moat_workspace(ops, need, 0xFF)                # exactly the queried size
    mo.guards.append(ws.guard)
    o, lse = fwd(q, k, v, B, T, nh, ws, 0.1, 5, 0)
    out = tuple(mo.written(torch.empty(M, C, dtype=tout), n) for n in ("dq", "dk", "dv"))
    L.set_debug_flags(flags)
    try:
        bwd(q, k, v, o, d_o, lse, B, T, nh, ws, 0.1, 5, 0, out=out)
        sums = int(L.last_attention_bwd_slab_sums())
        # the planner, asked without a launch (under the same flags), predicts what the call then did
        from tests.test_attention_plan_cpu import KIND_OF, query_plan
        rc, plan = query_plan(1, KIND_OF[kind], B, T, nh, hd, need)
        assert rc == 0 and plan.slab_sums == sums, (rc, plan and plan.slab_sums, sums)
        mo.check()
    finally:
        L.set_debug_flags(0)
    return out, sums


# B, T, nh, hd, kind, slab-sum launches (merged form, debug-flag form).  The launch counts follow from the split heuristic
# (pick_splits: 16 workgroups per split on 256 CUs, so cost = tiles per split + penalty x splits, penalty 0.35 for fp32
# operands and 4 for 16-bit ones) and from the workspace query's 16 slabs; they pin which branch each case takes, so that a
# change of the heuristic cannot turn the comparison into one of a path with itself unnoticed.
ATTN_SUM_CASES = [
    (2, 130, 4, 16, "f32", 1, 2), (2, 130, 4, 128, "f32", 1, 2),      # 5 key tiles: 5 + 5 + 5 slabs fit -> merged
    (2, 250, 4, 16, "f32", 1, 2), (2, 250, 4, 128, "f32", 1, 2),      # 8 key tiles cost 3.8 as 8 splits, 3.4 as 4: 12 slabs fit
    (2, 512, 4, 16, "f32", 2, 2), (2, 512, 4, 128, "f32", 2, 2),      # 16 tiles: 8 splits (4.8), 8 + 8 + 8 slabs do NOT fit
    (2, 130, 4, 64, "bf16out", 1, 2),                                 # fp32 operands (5 splits), bf16 sums out of pair 2
    (2, 512, 4, 64, "bf16", 1, 2), (2, 512, 4, 64, "f16", 1, 2),      # 16-bit operands: 16 tiles cost 20 / 16 / 18 -> 2 splits
    (2, 130, 4, 64, "bf16", 0, 0),                                    # 16-bit operands, 5 tiles: 9 < 11, nothing is split
]


@pytest.mark.parametrize("B,T,nh,hd,kind,n_one,n_two", ATTN_SUM_CASES)
def test_attention_bwd_single_slab_sum_is_bit_identical(B, T, nh, hd, kind, n_one, n_two):
    ops = _ops()
    two, sums_two = _attn_bwd(ops, B, T, nh, hd, kind, MERGED_SUM_OFF)
    one, sums_one = _attn_bwd(ops, B, T, nh, hd, kind, 0)
    assert (sums_one, sums_two) == (n_one, n_two)
    for name, a, b in zip(("dq", "dk", "dv"), two, one):
        assert not torch.isnan(b.float()).any(), name
        assert b.float().abs().max() > 0, name
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())


# ---- C. grouped per-modality stage glue ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [8, 32])
def test_grouped_stage_glue_is_bit_identical(H, dtype):
    ops = _ops()
    B, S, C, views = 1, 2, 64, 2
    fps = (views * S, S, S)                                  # the image map holds more frames than the other two
    offs = (0, fps[0] * 64, (fps[0] + S) * 64)
    T = (views + 2) * S * 64 + 2
    g = _gen("glue", H, dtype)
    feats_h = [rnd(g, B * f, H, H, C, dtype=dtype) for f in fps]
    dfeat_h = [rnd(g, B * f, H, H, C, dtype=dtype) for f in fps]
    pos_h, tok_h = rnd(g, T, C), rnd(g, B, T, C)
    res = []
    for grouped in (False, True):
        mo = Moats()
        feats, dfin = [mo.read(t) for t in feats_h], [mo.read(t) for t in dfeat_h]
        pos, tok = mo.read(pos_h), mo.read(tok_h)
        x0 = mo.written(torch.empty(B, T, C), "tokens")
        dtok = mo.written(torch.empty(B, T, C), "dtok")
        outs = [mo.written(torch.empty_like(t), "out") for t in feats_h]
        dfeats = [mo.written(torch.empty_like(t), "dfeat") for t in feats_h]
        if grouped:
            ops.avgpool_tokens_fwd3(feats, pos.data_ptr(), x0, fps, offs, T, 0.1, 9, 4096)
            ops.upsample_add_fwd3(feats, tok, outs, fps, offs, T)
            ops.upsample_add_bwd3(dfin, dtok, fps, offs, T)
            ops.avgpool_tokens_bwd3(tok, dfin, dfeats, fps, offs, T)
        else:
            for m in range(3):
                ops.avgpool_tokens_fwd(feats[m], pos.data_ptr(), x0, fps[m], offs[m], T, 0.1, 9, 4096)
                ops.upsample_add_fwd(feats[m], tok, outs[m], fps[m], offs[m], T)
                ops.upsample_add_bwd(dfin[m], dtok, fps[m], offs[m], T)
                ops.avgpool_tokens_bwd(tok, dfin[m], dfeats[m], fps[m], offs[m], T)
        mo.check()
        res.append([x0[:, :T - 2], dtok[:, :T - 2]] + outs + dfeats)   # the two GPS rows belong to other kernels
        assert torch.isnan(x0[:, T - 2:]).all() and torch.isnan(dtok[:, T - 2:]).all()
    for i, (a, b) in enumerate(zip(*res)):
        assert not torch.isnan(b.float()).any(), i
        assert torch.equal(a, b), i
    assert (res[1][0] == 0).float().mean().item() > 0.02     # the embedding dropout was on


# ---- D. small_linear with coalesced weight reads ---------------------------------------------------------------------------
U = 2.0 ** -24   # fp32 unit roundoff


def _dot_bound(terms_abs_sum, n):
    """(n + 2) u sum |terms| with n the reduction length: the fp32 dot-product bound for any summation order (at most n
    roundings lie on the path of any term: gamma_n < (n + 2) u).  The bias of the forward and the value an accumulating call
    adds to count among the terms of the sum - a bound on sum |x w| alone cannot hold for any kernel once |b| exceeds it,
    since the last addition rounds relative to the whole result - while the factor stays n + 2 of the reduction length:
    the fused multiply-adds round once per product, so the bias costs no rounding and the accumulate one."""
    return (n + 2) * U * terms_abs_sum


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N", [64, 512])
@pytest.mark.parametrize("K", [2, 130, 512])
@pytest.mark.parametrize("M", [4, 24])
def test_small_linear_against_fp64(M, K, N, relu):
    L = _lib()
    rpg = 2
    gstride = rpg * K + 7                                    # rows in groups of 2, the groups 7 floats apart
    G = M // rpg
    g = _gen("sl", M, K, N, relu)
    xbuf = rnd(g, G * gstride)
    w, b = rnd(g, N, K, scale=K ** -0.5), rnd(g, N)
    dy = rnd(g, M, N)
    rows = torch.tensor([(m // rpg) * gstride + (m % rpg) * K for m in range(M)])
    idx = rows[:, None] + torch.arange(K)[None, :]
    x64, w64, b64, dy64 = xbuf[idx].double(), w.double(), b.double(), dy.double()

    # forward: K products on top of the bias
    mo = Moats()
    xd, wd, bd = mo.read(xbuf), mo.read(w), mo.read(b)
    y = mo.written(torch.empty(M, N), "y")
    L.small_linear_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), M, N, K, rpg, gstride, relu, 0)
    mo.check()
    pre = x64 @ w64.T + b64
    ref = pre.clamp_min(0) if relu else pre
    bound = _dot_bound(x64.abs() @ w64.abs().T + b64.abs(), K)
    err = (y.cpu().double() - ref).abs()
    print(f"fwd M={M} K={K} N={N} relu={relu}: max err/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), (err / bound).max().item()

    # backward: ReLU mask on dy, dx accumulated into a pre-filled strided buffer, dw / db accumulated likewise
    ymask = ref.float() if relu else None
    dyeff64 = dy64 * (ref > 0) if relu else dy64
    dx0, dw0, db0 = rnd(g, G * gstride), rnd(g, N, K), rnd(g, N)
    for accumulate in (0, 1):
        mo = Moats()
        dyd, xd, wd = mo.read(dy), mo.read(xbuf), mo.read(w)
        md = mo.read(ymask) if relu else None
        dxd = mo.written(dx0, "dx", keep=True)
        dwd, dbd = mo.written(dw0, "dw", keep=True), mo.written(db0, "db", keep=True)
        L.small_linear_bwd(dyd.data_ptr(), md.data_ptr() if relu else 0, xd.data_ptr(), wd.data_ptr(), dxd.data_ptr(),
                           dwd.data_ptr(), dbd.data_ptr(), M, N, K, rpg, gstride, rpg, gstride, accumulate, accumulate, 0)
        mo.check()
        base = lambda t: t.double() if accumulate else torch.zeros_like(t).double()
        extra = lambda t: t.double().abs() if accumulate else 0.0    # what an accumulating call adds to is a term too
        # dx[m][k] = sum_n dyeff[m][n] w[n][k]: reduction length N
        ref_dx = base(dx0[idx]) + dyeff64 @ w64
        err = (dxd.cpu()[idx].double() - ref_dx).abs()
        bound = _dot_bound(dyeff64.abs() @ w64.abs() + extra(dx0[idx]), N)
        print(f"dgrad acc={accumulate}: max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all())
        gaps = torch.ones(G * gstride, dtype=torch.bool)
        gaps[idx.flatten()] = False
        assert torch.equal(dxd.cpu()[gaps], dx0[gaps])               # the floats between the row groups are not touched
        # dw[n][k] = sum_m dyeff[m][n] x[m][k], db[n] = sum_m dyeff[m][n] (the bias column): reduction length M
        ref_dw = base(dw0) + dyeff64.T @ x64
        err = (dwd.cpu().double() - ref_dw).abs()
        assert bool((err <= _dot_bound(dyeff64.abs().T @ x64.abs() + extra(dw0), M)).all())
        ref_db = base(db0) + dyeff64.sum(0)
        err = (dbd.cpu().double() - ref_db).abs()
        assert bool((err <= _dot_bound(dyeff64.abs().sum(0) + extra(db0), M)).all())


# ---- the whole step: every launch taken off the chain switched back on changes no bit -------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_train_step_is_bit_identical_with_the_chain_launches_restored(mode):
    """two training iterations (dropout 0.1, three trunk streams, weight-gradient companion stream) with the deferred
    LayerNorm finalize, the grouped stage glue and the single attention slab sum, against the per-layer / per-map / two-sum
    forms: same losses, parameters and optimizer moments, bit for bit"""
    ops = _ops()
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
    from deepsense6g_tii_amd.train import FusedAdamW, train_iteration
    from oracle import fusion_ref as fr
    kw = dict(n_layer=2)
    rcfg = fr.RefConfig(**kw)
    sd = fr.make_state(rcfg, seed=8)
    batches = [fr.make_inputs(rcfg, 2, seed=60 + i)[:5] for i in range(2)]
    dev = torch.device("cuda:0")
    ops.set_compute_mode(mode)
    try:
        runs = []
        for restored in (True, False):
            model = TransFuser(GlobalConfig(**kw), dev)
            model.load_state_dict(sd)
            model.train()
            assert model.defer_ln_finalize and model.group_stage_glue      # the defaults
            if restored:
                model.defer_ln_finalize = model.group_stage_glue = False
            _lib().set_debug_flags(MERGED_SUM_OFF if restored else 0)
            opt = FusedAdamW(model, lr=1e-3)
            losses = [float(train_iteration(model, opt, b)[0]) for b in batches]
            torch.cuda.synchronize()
            runs.append((losses, model.flat_parameters()[0].clone(), opt.m.clone(), opt.v.clone()))
        a, b = runs
        assert a[0] == b[0]
        for name, x, y in zip(("p", "m", "v"), a[1:], b[1:]):
            assert torch.equal(x, y), name
    finally:
        _lib().set_debug_flags(0)
        ops.set_compute_mode("f32")
