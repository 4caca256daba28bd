"""GPU tests of the Mamba fusion stage on a model walk's conventions (mamba_fusion.stage_forward / stage_backward,
block_forward / block_backward, mamba.layer_backward with gradient destinations).

Stage parity: NHWC maps at full resolution in, NHWC maps out, every parameter gradient written through a g(p) -> (pointer,
accumulate) lookup.  Reference: the composition of the public definitions in fp64 on the CPU - torch adaptive average pool ->
tests/mamba_fusion_ref.fusion_ref (pinned to the reference's MambaFusion by its golden generator) -> F.interpolate(bilinear,
align_corners=False) -> add.  Yardstick: the same composition in fp32.  Bar: e_hip <= max(10 * e_32, 1e-5) per tensor
(tests/mamba_ref.rel_err / bar), every compared reference tensor non-zero (the stage underflows at the reference's
initialisation, so the cases use the spread parameter set), LeakyReLU margin >= KINK_MIN on the fp64 run.

Default path: _BlockFn without destinations must give the bits of the launch sequence it had before the body moved into
block_forward / block_backward; that sequence is written out below from ops calls alone."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from tests import mamba_fusion_ref as fr
from tests import mamba_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
F64 = torch.float64
# (C, H, S, B, n_layer, seed); the seeds were picked on the CPU so that the LeakyReLU margin holds (8.6e-6 and 3.0e-6)
STAGE_CASES = [(64, 64, 1, 2, 2, 12), (512, 8, 1, 2, 2, 17)]


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


def _dev(t):
    return t.to(DEV, F32).contiguous()


def _module(C, S, n_layer, p):
    from deepsense6g_tii_amd.mamba_fusion import MambaFusion
    m = MambaFusion(n_embd=C, ln_size=(192 * S + 2, C), d_state=16, d_conv=4, expand=2, n_layer=n_layer, vert_anchors=8,
                    horz_anchors=8, seq_len=S, embd_pdrop=0.0, config=types.SimpleNamespace(n_views=1), device=DEV)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    return m


def _stage_ref(p64, x64, d64, n_layer, S, dtype):
    """-> ({out0..2, gps_out, dfeat0..2, dgemb, <parameter names>}, kink margin) of the composition in `dtype` on the CPU"""
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in p64.items()}
    x = {k: v.to(dtype).clone().requires_grad_(True) for k, v in x64.items()}
    feats = [x[f"feat{m}"] for m in range(3)]
    H = feats[0].shape[1]
    probe = []
    pooled = [F.adaptive_avg_pool2d(f.permute(0, 3, 1, 2), 8) for f in feats]
    *maps, gps_out = fr.fusion_ref(p, n_layer, S, *pooled, x["gemb"], probe=probe)
    outs = []
    for f, t in zip(feats, maps):
        up = t if H == 8 else F.interpolate(t, scale_factor=H // 8, mode="bilinear", align_corners=False)
        outs.append(f + up.permute(0, 2, 3, 1))
    loss = sum((o * d64[f"out{m}"].to(dtype)).sum() for m, o in enumerate(outs)) + (gps_out * d64["gps_out"].to(dtype)).sum()
    loss.backward()
    res = {f"out{m}": o.detach() for m, o in enumerate(outs)}
    res["gps_out"] = gps_out.detach()
    res.update({f"dfeat{m}": x[f"feat{m}"].grad for m in range(3)})
    res["dgemb"] = x["gemb"].grad
    res.update({k: p[k].grad for k in p})
    return res, fr.kink_margin(probe)


@functools.lru_cache(maxsize=None)
def _stage_case(C, H, S, B, n_layer, seed):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = fr.make_fusion_params(C, S, n_layer, seed=seed, spread=True)
    g = torch.Generator().manual_seed(9700 + seed + C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    x = {f"feat{m}": rn(B * S, H, H, C) for m in range(3)}
    x["gemb"] = rn(B, 2, C)
    d = {f"out{m}": rn(B * S, H, H, C) for m in range(3)}
    d["gps_out"] = rn(B, 2, C)
    r64, margin = _stage_ref(p, x, d, n_layer, S, F64)
    r32, _ = _stage_ref(p, x, d, n_layer, S, F32)
    return p, x, d, r64, r32, margin


def _hip_stage(m, x, d, B, pre=None):
    """one stage_forward + stage_backward -> the tensors of _stage_ref.  pre: {name: tensor} the parameter gradients are ADDED
    to (accumulate flag 1); None: NaN-filled destinations, flag 0"""
    from deepsense6g_tii_amd import mamba_fusion as mf
    ops = _ops()
    S, C, T = m.seq_len, m.n_embd, m.n_tokens
    ws = ops.Workspace(torch.device(DEV), mf.stage_workspace_bytes(m, B))
    feats = [_dev(x[f"feat{q}"]) for q in range(3)]
    gemb = _dev(x["gemb"])
    outs = [torch.full_like(f, float("nan")) for f in feats]
    xo, tape = mf.stage_forward(m, ws, True, feats, gemb, outs, B)
    grads = {k: (_dev(pre[k]) if pre is not None else torch.full_like(q, float("nan"))) for k, q in m.named_parameters()}
    slot = {id(q): (grads[k].data_ptr(), int(pre is not None)) for k, q in m.named_parameters()}
    douts = [_dev(d[f"out{q}"]) for q in range(3)]
    dfeats = [torch.full_like(f, float("nan")) for f in feats]
    dgemb = torch.full_like(gemb, float("nan"))
    mf.stage_backward(m, ws, tape, douts, (_dev(d["gps_out"]), False), dfeats, dgemb, B, lambda q: slot[id(q)])
    res = {f"out{q}": outs[q] for q in range(3)}
    res["gps_out"] = xo.view(B, T, C)[:, T - 2:]
    res.update({f"dfeat{q}": dfeats[q] for q in range(3)})
    res["dgemb"] = dgemb
    res.update(grads)
    return res


def _compare(tag, hip, r32, r64):
    bad = []
    print()
    for k in r64:
        assert r64[k].abs().max() > 0, k                       # a relative error against a zero tensor checks nothing
        e32, eh = mr.rel_err(r32[k], r64[k]), mr.rel_err(hip[k], r64[k])
        print(f"parity {tag:<32s} {k:<48s} e_hip {eh:.3e}  e_32 {e32:.3e}  bar {mr.bar(e32):.3e}")
        if not eh <= mr.bar(e32):
            bad.append((k, eh, e32))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("C,H,S,B,n_layer,seed", STAGE_CASES)
def test_stage_matches_the_composition_of_the_public_definitions(C, H, S, B, n_layer, seed):
    p, x, d, r64, r32, margin = _stage_case(C, H, S, B, n_layer, seed)
    assert margin >= fr.KINK_MIN, margin
    m = _module(C, S, n_layer, p)
    hip = _hip_stage(m, x, d, B)
    assert set(hip) == set(r64) and len(hip) == 8 + 3 + 24 * n_layer
    _compare(f"stage C={C} H={H} S={S} B={B} L={n_layer}", hip, r32, r64)
    again = _hip_stage(m, x, d, B)                             # fixed-order sums everywhere: two runs are bit-identical
    for k in hip:
        assert torch.equal(hip[k], again[k]), k


def test_stage_accumulates_onto_existing_gradients_and_refuses_a_short_workspace():
    from deepsense6g_tii_amd import mamba_fusion as mf
    ops = _ops()
    C, H, S, B, n_layer, seed = STAGE_CASES[0]
    p, x, d, r64, r32, _ = _stage_case(C, H, S, B, n_layer, seed)
    m = _module(C, S, n_layer, p)
    g = torch.Generator().manual_seed(5)
    pre = {k: torch.randn(v.shape, generator=g, dtype=F64) for k, v in p.items()}
    hip = _hip_stage(m, x, d, B, pre=pre)
    names = list(p)
    _compare("stage accumulate", {k: hip[k] for k in names}, {k: r32[k] + pre[k].float() for k in names},
             {k: r64[k] + pre[k] for k in names})
    short = ops.Workspace(torch.device(DEV), mf.stage_workspace_bytes(m, B) - 1)
    feats = [_dev(x[f"feat{q}"]) for q in range(3)]
    with pytest.raises(ValueError, match="workspace"):
        mf.stage_forward(m, short, False, feats, _dev(x["gemb"]), [torch.empty_like(f) for f in feats], B)


# ---- the default path: _BlockFn without destinations ------------------------------------------------------------------------
def _layer_backward_as_it_was(ops, mod, ws, reverse, Bsz, L, tape, params, dout2, du_out):
    u2, xz, xc, x_dbl, dt, draw, y, saved = tape
    w_in, conv_w, conv_b, w_x, w_dt, b_dt, A_log, Dp, w_out = params
    M, D, r, dm = Bsz * L, mod.d_inner, mod.dt_rank, mod.d_model
    empty = lambda *s: torch.empty(s, dtype=F32, device=dout2.device)      # noqa: E731
    g_out = empty(dm, D)
    ops.linear_wgrad(y, dout2, g_out.data_ptr(), ws)
    dy = ops.linear_dgrad(dout2, w_out.data_ptr(), D)
    dxz, dxdbl, dxc, ddraw = empty(M, 2 * D), empty(M, r + 32), empty(M, D), empty(M, D)
    g_A, g_D = ops.selective_scan_bwd(xc, draw, b_dt, A_log, x_dbl[:, r:r + 16], x_dbl[:, r + 16:], Dp, xz[:, D:], dy, saved,
                                      dxc, ddraw, dxdbl[:, r:r + 16], dxdbl[:, r + 16:], dxz[:, D:], Bsz, L, ws, reverse)
    g_dtw, g_dtb = empty(D, r), empty(D)
    ops.linear_wgrad(dt, ddraw, g_dtw.data_ptr(), ws, dbias_ptr=g_dtb.data_ptr())
    ops.copy_cols(ops.linear_dgrad(ddraw, w_dt.data_ptr(), r), dxdbl[:, :r])
    g_x = empty(r + 32, D)
    ops.linear_wgrad(xc, dxdbl, g_x.data_ptr(), ws)
    ops.linear_dgrad(dxdbl, w_x.data_ptr(), D, out=dxc, accumulate=True)
    g_cw, g_cb = ops.causal_conv1d_silu_bwd(xz[:, :D], conv_w, conv_b, dxc, dxz[:, :D], Bsz, L, ws, reverse)
    g_in = empty(2 * D, dm)
    ops.linear_wgrad(u2, dxz, g_in.data_ptr(), ws)
    ops.linear_dgrad(dxz, w_in.data_ptr(), dm, out=du_out, accumulate=True)
    return (g_in, g_cw, g_cb, g_x, g_dtw, g_dtb, g_A, g_D, g_out)


def _block_as_it_was(blk, x, dout):
    """forward + backward of one MambaBlock as the launch sequence of _BlockFn before its body became block_forward /
    block_backward -> (out, dx, the 24 gradients)"""
    from deepsense6g_tii_amd.mamba import layer_forward
    ops = _ops()
    B, T, C = x.shape
    M = B * T
    ws = blk._workspace(x.device, B, T)
    ln_w, ln_b, w1, b1, w2, b2, *mp = [q.detach() for q in blk._params()]
    x2 = x.reshape(B, T * C).contiguous()
    xl, mean, rstd = ops.sample_layernorm_fwd(x2, ln_w, ln_b, ws)
    x1 = ops.linear_fwd(xl.view(M, C), w1.data_ptr(), b1.data_ptr(), C)
    fm, tape_f = layer_forward(blk.forward_mamba, ws, False, True, x1, B, T, mp[:9])
    bm, tape_b = layer_forward(blk.backward_mamba, ws, True, True, x1, B, T, mp[9:])
    f2 = ops.linear_fwd(x1, w2.data_ptr(), b2.data_ptr(), C)
    out = ops.bimamba_gate_fwd(fm, bm, f2, B, T)
    empty = lambda *s: torch.empty(s, dtype=F32, device=x.device)          # noqa: E731
    dfm, dbm, df2 = ops.bimamba_gate_bwd(dout.reshape(M, C).contiguous(), fm, bm, f2, B, T)
    g_w2, g_b2 = empty(C, C), empty(C)
    ops.linear_wgrad(x1, df2, g_w2.data_ptr(), ws, dbias_ptr=g_b2.data_ptr())
    dx1 = ops.linear_dgrad(df2, w2.data_ptr(), C)
    g_f = _layer_backward_as_it_was(ops, blk.forward_mamba, ws, False, B, T, tape_f, mp[:9], dfm, dx1)
    g_b = _layer_backward_as_it_was(ops, blk.backward_mamba, ws, True, B, T, tape_b, mp[9:], dbm, dx1)
    g_w1, g_b1 = empty(C, C), empty(C)
    ops.linear_wgrad(xl.view(M, C), dx1, g_w1.data_ptr(), ws, dbias_ptr=g_b1.data_ptr())
    dxl = ops.linear_dgrad(dx1, w1.data_ptr(), C)
    g_lw, g_lb = empty(T, C), empty(T, C)
    dx = ops.sample_layernorm_bwd(dxl.view(B, T * C), x2, mean, rstd, ln_w, g_lw, g_lb, ws)
    return out.view(B, T, C), dx.view(B, T, C), (g_lw, g_lb, g_w1, g_b1, g_w2, g_b2, *g_f, *g_b)


def test_block_default_path_keeps_its_bits_and_destinations_change_none():
    from deepsense6g_tii_amd.mamba_fusion import MambaBlock, block_backward, block_forward
    B, L, C, wide, seed = fr.BLOCK_CASES[0]
    p = fr.make_block_params(C, L, seed=seed, wide=wide)
    x, dout = (_dev(t) for t in fr.make_block_input(C, B, L, seed=seed))
    blk = MambaBlock(C, (L, C), 16, 4, 2, device=DEV)
    blk.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    blk.train()
    was_out, was_dx, was_g = _block_as_it_was(blk, x, dout)
    xd = x.clone().requires_grad_(True)
    out = blk(xd)
    out.backward(dout)
    assert torch.equal(out.detach(), was_out) and torch.equal(xd.grad, was_dx)
    plist = blk._params()                                      # the order of the 24 gradients (not registration order)
    name = {id(q): k for k, q in blk.named_parameters()}
    for q, g in zip(plist, was_g):
        assert torch.equal(q.grad, g), name[id(q)]
    # fresh destinations (flag 0) receive the same bits in place; flag 1 adds them to what is there
    params = [q.detach() for q in blk._params()]
    ws = blk._workspace(x.device, B, L)
    _, tape = block_forward(blk, ws, True, x.reshape(B, L * C).contiguous(), B, L, params)
    for acc in (0, 1):
        dst = [torch.full_like(g, 2.0) for g in was_g]
        dx, none = block_backward(blk, ws, tape, dout.reshape(B * L, C).contiguous(), B, L, params,
                                  gdst=[(t.data_ptr(), acc) for t in dst])
        assert none is None and torch.equal(dx.view(B, L, C), was_dx)
        for q, t, g in zip(plist, dst, was_g):
            if not acc:
                assert torch.equal(t, g), name[id(q)]
            else:                                              # one fp32 add onto 2.0, whichever kernel or temporary made it
                assert mr.rel_err(t, g.double().cpu() + 2.0) <= 1e-5, name[id(q)]
    # mixed flags inside a pair (weight fresh, bias accumulated) go through temporaries and land in the right places
    dst = [torch.full_like(g, 2.0) for g in was_g]
    flags = [i % 2 for i in range(len(dst))]
    block_backward(blk, ws, tape, dout.reshape(B * L, C).contiguous(), B, L, params,
                   gdst=[(t.data_ptr(), a) for t, a in zip(dst, flags)])
    for q, t, g, a in zip(plist, dst, was_g, flags):
        assert mr.rel_err(t, g.double().cpu() + 2.0 * a) <= 1e-5, (name[id(q)], a)
