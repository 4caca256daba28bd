"""CPU-side checks of the Mamba fusion block and stage on 16-bit storage: the hooked restatement (tests/mamba_fusion16_ref.py)
with the identity hook IS tests/mamba_fusion_ref.py, the six ds6g_h16_* entry points of csrc/mamba_fusion.hip are declared and
exported, each refuses bad arguments on the host before any launch, and the ops wrappers pick the entry point by storage
dtype and refuse mixed operands (the entry points replaced by recording stubs: nothing is launched)."""
import ctypes

import pytest
import torch

from deepsense6g_tii_amd import _lib, ops
from tests import mamba16_ref as m16
from tests import mamba_fusion16_ref as f16r
from tests import mamba_fusion_ref as fr

F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
NEW = ("sample_layernorm_fwd", "sample_layernorm_bwd", "bimamba_gate_fwd", "bimamba_gate_bwd", "pool_swap_tokens_fwd",
       "pool_swap_tokens_bwd")


def test_identity_hook_block_is_the_fp32_restatement_to_the_bit():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, L, C, wide, seed = fr.BLOCK_CASES[0]
    p = fr.make_block_params(C, L, seed=seed, wide=wide)
    x, dout = fr.make_block_input(C, B, L, seed=seed)
    for dt in (F64, F32):
        want, margin = fr.block_run(p, x, dout, dt)
        got, margin16 = f16r.block_run16(p, x, dout, m16.rounder(None), dt)
        assert margin == margin16 and set(got) == set(want) and len(got) == 26
        for k in want:
            assert torch.equal(got[k], want[k]), (dt, k)


def test_identity_hook_stage_is_the_composition_to_the_bit():
    from tests.test_mamba_stage_walk_gpu import _stage_ref
    torch.set_num_threads(min(16, torch.get_num_threads()))
    C, H, S, B, n_layer, seed = 64, 16, 1, 2, 2, 12
    p = fr.make_fusion_params(C, S, n_layer, seed=seed, spread=True)
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    x = {f"feat{m}": rn(B * S, H, H, C) for m in range(3)}
    x["gemb"] = rn(B, 2, C)
    d = {f"out{m}": rn(B * S, H, H, C) for m in range(3)}
    d["gps_out"] = rn(B, 2, C)
    want, margin = _stage_ref(p, x, d, n_layer, S, F64)
    got, margin16 = f16r.stage_run16(p, x, d, n_layer, S, m16.rounder(None))
    assert margin == margin16 and set(got) == set(want) and len(got) == 8 + 3 + 24 * n_layer
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_rounding_hook_rounds_what_the_storage_map_says():
    """the block's output and input gradient are representable in the storage type, the parameter gradients are not rounded"""
    B, L, C, wide, seed = fr.BLOCK_CASES[0]
    p = fr.make_block_params(C, L, seed=seed, wide=wide)
    x, dout = fr.make_block_input(C, B, L, seed=seed)
    for dt in (BF16, F16):
        got, _ = f16r.block_run16(p, x, dout, m16.rounder(dt))
        for k in ("out", "input"):
            assert torch.equal(got[k], got[k].to(dt).to(F64)), k
        assert not torch.equal(got["fc1.weight"], got["fc1.weight"].to(dt).to(F64))


def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    L = _lib.lib()
    for e in NEW:
        name = "ds6g_h16_" + e
        assert name in protos and hasattr(L._dll, name) and callable(getattr(L, "h16_" + e)), name
        f32 = protos["ds6g_" + e][1]
        assert protos[name][1] == [ctypes.c_int] + f32, name        # the storage code, then the fp32 entry's arguments


P = 0x1000   # a non-NULL, 16-byte aligned stand-in: every call below must be refused before anything is launched
BIG = 1 << 24


def _sln_fwd(L, st=1, ptrs=(P,) * 6, B=2, n=4096, ws=P, ws_bytes=BIG):
    x, g, b, y, mean, rstd = ptrs
    return L.h16_sample_layernorm_fwd(st, x, g, b, y, mean, rstd, B, n, 1e-5, ws, ws_bytes, 0)


def _sln_bwd(L, st=1, ptrs=(P,) * 8, B=2, n=4096, ws=P, ws_bytes=BIG):
    dy, x, mean, rstd, g, dx, dg, db = ptrs
    return L.h16_sample_layernorm_bwd(st, dy, x, mean, rstd, g, dx, dg, db, B, n, 0, ws, ws_bytes, 0)


def _gate_fwd(L, st=1, ptrs=(P,) * 4, lds=(64,) * 4, C=64):
    fm, bm, f2, out = ptrs
    return L.h16_bimamba_gate_fwd(st, fm, lds[0], bm, lds[1], f2, lds[2], out, lds[3], 2, 5, C, 0)


def _gate_bwd(L, st=1, ptrs=(P,) * 7, lds=(64,) * 7, C=64):
    do, fm, bm, f2, dfm, dbm, df2 = ptrs
    return L.h16_bimamba_gate_bwd(st, do, lds[0], fm, lds[1], bm, lds[2], f2, lds[3], dfm, lds[4], dbm, lds[5], df2, lds[6], 2, 5,
                                  C, 0)


def _descs(ins=(P,) * 3, outs=(P,) * 3, S=1):
    d = (ops._MapDesc * 3)()
    for m in range(3):
        d[m].inp, d[m].out, d[m].frames_per_sample, d[m].mod_off = ins[m], outs[m], S, m * S * 64
    return d


def _pool_fwd(L, st=1, descs=None, ptrs=(P,) * 3, C=64):
    d = descs or _descs()
    return L.h16_pool_swap_tokens_fwd(st, ctypes.addressof(d), *ptrs, 2, 1, 16, C, 0.0, 0, 0, 0)


def _pool_bwd(L, st=1, descs=None, ptrs=(P,) * 3, C=64):
    d = descs or _descs()
    dtok, dgemb, dpos = ptrs
    return L.h16_pool_swap_tokens_bwd(st, ctypes.addressof(d), dtok, dgemb, dpos, 0, 2, 1, 16, C, 0.0, 0, 0, 0)


def test_new_entry_points_reject_bad_arguments_without_launching():
    L = _lib.lib()
    E = _lib.Ds6gError

    def refused(fn, **bad):
        with pytest.raises(E, match="code 1$"):                   # DS6G_ERR_ARG
            fn(L, **bad)

    for fn in (_sln_fwd, _sln_bwd, _gate_fwd, _gate_bwd, _pool_fwd, _pool_bwd):
        for st in (0, 3, -1):                                     # 0 is fp32: it has entry points of its own
            refused(fn, st=st)
    need = int(L.sample_layernorm_workspace_bytes(2, 4096))
    for fn, nptr, scalar in ((_sln_fwd, 6, (4, 5)), (_sln_bwd, 8, (2, 3))):   # mean / rstd: scalars per sample
        for st in (1, 2):
            for i in range(nptr):
                refused(fn, st=st, ptrs=tuple(0 if j == i else P for j in range(nptr)))
                if i not in scalar:
                    refused(fn, st=st, ptrs=tuple(P + 8 if j == i else P for j in range(nptr)))
            refused(fn, st=st, n=4100)                            # a whole number of float4, not of 8-element pieces
            refused(fn, st=st, ws=P + 8)
            for short in (need - 1, 0):
                with pytest.raises(E, match="code 3$"):           # DS6G_ERR_WORKSPACE
                    fn(L, st=st, ws_bytes=short)
    for fn, nptr in ((_gate_fwd, 4), (_gate_bwd, 7)):
        for st in (1, 2):
            for i in range(nptr):
                refused(fn, st=st, ptrs=tuple(0 if j == i else P for j in range(nptr)))
                refused(fn, st=st, ptrs=tuple(P + 8 if j == i else P for j in range(nptr)))
                refused(fn, st=st, lds=tuple(68 if j == i else 64 for j in range(nptr)))    # % 4 but not % 8
                refused(fn, st=st, lds=tuple(56 if j == i else 64 for j in range(nptr)))    # shorter than a row
            refused(fn, st=st, C=68)
    for fn in (_pool_fwd, _pool_bwd):
        for st in (1, 2):
            for i in range(3):
                refused(fn, st=st, ptrs=tuple(0 if j == i else P for j in range(3)))
                refused(fn, st=st, ptrs=tuple(P + 8 if j == i else P for j in range(3)))
            refused(fn, st=st, C=68)                              # fp32 takes C % 4, a 16-bit piece is 8 channels
            refused(fn, st=st, C=520)
    for m in range(3):
        bad = tuple(P + 8 if j == m else P for j in range(3))
        refused(_pool_fwd, descs=_descs(ins=bad))
        refused(_pool_bwd, descs=_descs(outs=bad))
        refused(_pool_bwd, descs=_descs(ins=bad))


class _OnDevice(torch.Tensor):
    """a host tensor that says it is on the device: the wrappers' operand checks pass, and nothing is launched"""
    is_cuda = property(lambda self: True)


def _z(*shape, dt=F32):
    return torch.zeros(shape, dtype=dt).as_subclass(_OnDevice)


def test_wrappers_pick_entry_by_storage_and_refuse_mixed_operands(monkeypatch):
    L = _lib.lib()
    calls = []
    for e in NEW:
        for name in (e, "h16_" + e):
            monkeypatch.setattr(L, name, lambda *a, _n=name: calls.append((_n, a)))
    monkeypatch.setattr(ops, "_stream", lambda: 77)
    ws = ops.Workspace.__new__(ops.Workspace)
    ws.buf, ws.nbytes = torch.zeros(1 << 16, dtype=torch.uint8), 1 << 16
    B, Lq, C, S, H = 2, 3, 64, 1, 8
    M, n, T = B * Lq, Lq * C, 194
    gamma, beta, mean, rstd = _z(Lq, C), _z(Lq, C), _z(B), _z(B)
    gemb, dgemb, pos = _z(B, 2, C), _z(B, 2, C), _z(T, C)
    ST = {BF16: 1, F16: 2}

    def one(fn, *a, **k):
        del calls[:]
        ret = fn(*a, **k)
        assert len(calls) == 1 and calls[0][1][-1] == 77, calls
        return calls[0][0], calls[0][1][:-1], ret

    ops_t = {}
    for dt in (F32, BF16, F16):
        def entry(want, name, args):
            if dt == F32:
                assert name == want, (name, dt)
                return args
            assert name == "h16_" + want and args[0] == ST[dt], (name, args[0], dt)
            return args[1:]

        x, dy = _z(B, n, dt=dt), _z(B, n, dt=dt)
        name, args, (y, mu, rs) = one(ops.sample_layernorm_fwd, x, gamma, beta, ws)
        a = entry("sample_layernorm_fwd", name, args)
        assert y.dtype == dt and mu.dtype == F32 and rs.dtype == F32
        assert a[:3] == (x.data_ptr(), gamma.data_ptr(), beta.data_ptr()) and a[3] == y.data_ptr() and a[6:8] == (B, n)
        name, args, dx = one(ops.sample_layernorm_bwd, dy, x, mean, rstd, gamma, _z(Lq, C), _z(Lq, C), ws, accumulate=True)
        a = entry("sample_layernorm_bwd", name, args)
        assert dx.dtype == dt and a[:2] == (dy.data_ptr(), x.data_ptr()) and a[5] == dx.data_ptr() and a[8:11] == (B, n, 1)

        wide = _z(M, 2 * C, dt=dt)                                # operands that are column halves keep their row stride
        fm, bm, f2, out = wide[:, :C], wide[:, C:], _z(M, C, dt=dt), _z(M, C, dt=dt)
        name, args, o = one(ops.bimamba_gate_fwd, fm, bm, f2, B, Lq, out=out)
        a = entry("bimamba_gate_fwd", name, args)
        assert a == (fm.data_ptr(), 2 * C, bm.data_ptr(), 2 * C, f2.data_ptr(), C, out.data_ptr(), C, B, Lq, C)
        dst = tuple(_z(M, C, dt=dt) for _ in range(3))
        name, args, _ = one(ops.bimamba_gate_bwd, out, fm, bm, f2, B, Lq, out=dst)
        a = entry("bimamba_gate_bwd", name, args)
        assert a == (out.data_ptr(), C, fm.data_ptr(), 2 * C, bm.data_ptr(), 2 * C, f2.data_ptr(), C, dst[0].data_ptr(), C,
                     dst[1].data_ptr(), C, dst[2].data_ptr(), C, B, Lq, C)

        maps = [_z(B * S, H, H, C, dt=dt) for _ in range(3)]
        tok = _z(B, T, C, dt=dt)
        name, args, _ = one(ops.pool_swap_tokens_fwd, maps, gemb, pos.data_ptr(), tok, S, 0.1, 5, 9)
        a = entry("pool_swap_tokens_fwd", name, args)
        assert a[1:] == (gemb.data_ptr(), pos.data_ptr(), tok.data_ptr(), B, S, H, C, pytest.approx(0.1), 5, 9)
        name, args, _ = one(ops.pool_swap_tokens_bwd, tok, None, maps, dgemb, pos.data_ptr(), True, S)
        a = entry("pool_swap_tokens_bwd", name, args)
        assert a[1:] == (tok.data_ptr(), dgemb.data_ptr(), pos.data_ptr(), 1, B, S, H, C, 0.0, 0, 0)
        ops_t[dt] = dict(x=x, dy=dy, fm=fm, bm=bm, f2=f2, out=out, dst=dst, maps=maps, tok=tok)

    f, b, h = ops_t[F32], ops_t[BF16], ops_t[F16]
    mixed = {
        "ln fwd: bf16 x, bf16 gamma": lambda: ops.sample_layernorm_fwd(b["x"], _z(Lq, C, dt=BF16), beta, ws),
        "ln bwd: bf16 dy, fp32 x": lambda: ops.sample_layernorm_bwd(b["dy"], f["x"], mean, rstd, gamma, _z(Lq, C), _z(Lq, C), ws),
        "ln bwd: fp32 dy, f16 x": lambda: ops.sample_layernorm_bwd(f["dy"], h["x"], mean, rstd, gamma, _z(Lq, C), _z(Lq, C), ws),
        "gate fwd: bf16 fm, f16 bm": lambda: ops.bimamba_gate_fwd(b["fm"], h["bm"], b["f2"], B, Lq, out=b["out"]),
        "gate fwd: bf16 operands, fp32 out": lambda: ops.bimamba_gate_fwd(b["fm"], b["bm"], b["f2"], B, Lq, out=f["out"]),
        "gate bwd: f16 dout, fp32 f2": lambda: ops.bimamba_gate_bwd(h["out"], h["fm"], h["bm"], f["f2"], B, Lq, out=h["dst"]),
        "gate bwd: fp32 operands, bf16 df2": lambda: ops.bimamba_gate_bwd(f["out"], f["fm"], f["bm"], f["f2"], B, Lq,
                                                                          out=(f["dst"][0], f["dst"][1], b["dst"][2])),
        "pack fwd: bf16 maps, fp32 tokens": lambda: ops.pool_swap_tokens_fwd(b["maps"], gemb, pos.data_ptr(), f["tok"], S),
        "pack fwd: bf16 maps, one f16": lambda: ops.pool_swap_tokens_fwd([b["maps"][0], h["maps"][1], b["maps"][2]], gemb,
                                                                         pos.data_ptr(), b["tok"], S),
        "pack fwd: bf16 maps, bf16 gemb": lambda: ops.pool_swap_tokens_fwd(b["maps"], _z(B, 2, C, dt=BF16), pos.data_ptr(),
                                                                           b["tok"], S),
        "pack bwd: f16 dtokens, fp32 maps": lambda: ops.pool_swap_tokens_bwd(h["tok"], None, f["maps"], dgemb, pos.data_ptr(),
                                                                             False, S),
        "pack bwd: fp32 dtokens, bf16 dfeat_in": lambda: ops.pool_swap_tokens_bwd(f["tok"], b["maps"], f["maps"], dgemb,
                                                                                  pos.data_ptr(), False, S),
    }
    for what, call in mixed.items():
        del calls[:]
        with pytest.raises(AssertionError):
            call()
        assert not calls, (what, calls)
