"""GPU parity of the Mamba layer's 16-bit-storage path (ds6g_h16_causal_conv1d_* / ds6g_h16_selective_scan_* of
csrc/mamba.hip, the bf16 / f16 branch of deepsense6g_tii_amd/mamba.py) against tests/mamba_ref.py in fp64.

Inputs are drawn, then rounded to the type the kernel reads them in (16-bit activations, fp32 for the rest), so the fp64
reference sees exactly what the kernel sees.  Yardstick for fp32-accuracy claims: the same restatement in fp32 on the CPU,
e_32, bar32 = max(10 e_32, 1e-5) as in tests/test_mamba_gpu.py.  u16 = 2^-8 (bf16) / 2^-11 (f16), one store's unit roundoff.

  kernels   a 16-bit output is fp32 arithmetic plus ONE output rounding: |hip - ref| <= u16 |ref| + bar32 max|ref| elementwise;
            an fp32 output: max|hip - ref| / max|ref| <= bar32.  The entry points are called directly: what is read sits inside
            NaN moats, what is written (pre-filled with NaN) inside 0xFF moats (tests/moat.py).
  layer     several roundings compound, so the bar is measured: tests/mamba16_ref.py rounds exactly the tensors the storage map
            keeps 16-bit; its error against the unrounded fp64 run is e_round (computed here), and every tensor must hold
            e_hip <= 3 e_round + bar32 (3: the HIP GEMMs accumulate in fp32, so a value near a rounding boundary may land one
            ulp the other way).  The table is printed (pytest -s); the committed copy is profiles/mamba16_parity.txt."""
import functools

import pytest
import torch

from tests import mamba16_ref as m16
from tests import mamba_ref as mr
from tests import moat

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
F64 = torch.float64
MOAT = moat.MIN_MOAT
DTYPES = [torch.bfloat16, torch.float16]
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ST = {torch.bfloat16: 1, torch.float16: 2}
B, D, R = 2, 128, 4     # the kernel-level cases: d_model 64's inner width and dt_rank


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


def _lib():
    from deepsense6g_tii_amd._lib import lib
    return lib()


def _st():
    return _ops()._stream()


def _rd(t, dtype):
    """fp64 -> the value a `dtype` copy holds, as fp64"""
    return t.to(dtype).to(F64)


def _in(t, dtype, name):
    """a read operand: `t` (fp64, already representable) as `dtype` on the device, inside NaN moats"""
    return moat.embed(t.to(dtype).contiguous().to(DEV), MOAT, MOAT, "nan", name)


def _out(shape, dtype, name):
    """a written operand: NaN payload inside 0xFF moats"""
    return moat.embed(moat.nan_like(torch.empty(shape, dtype=dtype, device=DEV)), MOAT, MOAT, 0xFF, name)


def _half(t, dtype, right, name):
    """`t` [M, D] as one column half of a NaN [M, 2 D] buffer inside NaN moats -> (the half's view, the buffer, guard)"""
    M = t.shape[0]
    full = torch.full((M, 2 * D), float("nan"), dtype=F64)
    (full[:, D:] if right else full[:, :D]).copy_(t)
    buf, g = _in(full, dtype, name)
    return (buf[:, D:] if right else buf[:, :D]), buf, g


def _grads(fn, inputs, dout, dtype):
    xs = {k: v.to(dtype).clone().requires_grad_(True) for k, v in inputs.items()}
    y = fn(xs)
    (y * dout.to(dtype)).sum().backward()
    res = {"y": y.detach()}
    res.update({"d" + k: v.grad for k, v in xs.items()})
    return res


def _gate(tag, hip, r32, r64, dtype, out16):
    """out16: the keys stored in `dtype`; the others are fp32 outputs"""
    bad = []
    print()
    for k in r64:
        ref = r64[k].double()
        got = hip[k].double().cpu().reshape(ref.shape)
        assert torch.isfinite(got).all(), (tag, k)
        b32 = mr.bar(mr.rel_err(r32[k], ref))
        mx = ref.abs().max().item()
        err = (got - ref).abs()
        if k in out16:
            tol = U16[dtype] * ref.abs() + b32 * mx
            worst = (err / tol.clamp(min=1e-300)).max().item() if mx > 0 else float(err.max() > 0)
            print(f"parity16 {tag:<46s} {k:<12s} 16-bit  max err/tol {worst:.3f}  bar32 {b32:.3e}")
            ok = worst <= 1.0
        else:
            e = mr.rel_err(got, ref)
            print(f"parity16 {tag:<46s} {k:<12s} fp32    e_hip {e:.3e}  bar32 {b32:.3e}")
            ok = e <= b32
        if not ok:
            bad.append(k)
    assert not bad, (tag, bad)


def _name(dtype):
    return {torch.bfloat16: "bf16", torch.float16: "f16"}[dtype]


# ---- 1. the conv kernel alone ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(dtype, L, reverse):
    g = torch.Generator().manual_seed(10 + L)
    inputs = {"x": _rd(torch.randn(B, L, D, generator=g, dtype=F64), dtype),
              "w": _rd(mr._uniform(g, (D, 1, 4), 0.5), F32), "b": _rd(mr._uniform(g, (D,), 0.5), F32)}
    dout = _rd(torch.randn(B, L, D, generator=g, dtype=F64), dtype)
    fn = lambda t: mr.conv_ref(t["x"], t["w"], t["b"], reverse)
    return inputs, dout, _grads(fn, inputs, dout, F64), _grads(fn, inputs, dout, F32)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("L", [1, 3, 4, 131])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_conv_kernel(dtype, L, reverse):
    ops, lib = _ops(), _lib()
    inputs, dout, r64, r32 = _conv_case(dtype, L, reverse)
    M = B * L
    x, xz, g_xz = _half(inputs["x"].reshape(M, D), dtype, False, "xz")      # x: the left column half, as in the layer
    w, g_w = _in(inputs["w"], F32, "w")
    b, g_b = _in(inputs["b"], F32, "bias")
    dy, g_dy = _in(dout.reshape(M, D), dtype, "dy")
    y, g_y = _out((M, D), dtype, "y")
    dxz, g_dxz = _out((M, 2 * D), dtype, "dxz")
    dw, g_dw = _out((D, 1, 4), F32, "dw")
    db, g_db = _out((D,), F32, "db")
    ws = moat.moat_workspace(ops, int(lib.causal_conv1d_workspace_bytes(B, L, D)), 0xFF, DEV)
    before = moat.bits(dxz[:, D:]).clone()
    lib.h16_causal_conv1d_silu_fwd(ST[dtype], x.data_ptr(), 2 * D, w.data_ptr(), b.data_ptr(), y.data_ptr(), D, B, L, D,
                                   int(reverse), _st())
    lib.h16_causal_conv1d_silu_bwd(ST[dtype], x.data_ptr(), 2 * D, w.data_ptr(), b.data_ptr(), dy.data_ptr(), D,
                                   dxz.data_ptr(), 2 * D, dw.data_ptr(), db.data_ptr(), B, L, D, int(reverse), ws.ptr, ws.nbytes,
                                   _st())
    torch.cuda.synchronize()
    for g in (g_xz, g_w, g_b, g_dy, g_y, g_dxz, g_dw, g_db, ws.guard):
        g()
    assert torch.equal(moat.bits(dxz[:, D:]), before)                       # the other half is not touched
    hip = {"y": y, "dx": dxz[:, :D], "dw": dw, "db": db}
    _gate(f"conv {_name(dtype)} L={L} rev={int(reverse)}", hip, r32, r64, dtype, out16=("y", "dx"))


# ---- 2. the scan kernel alone ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scan_case(dtype, L, reverse, wide):
    g = torch.Generator().manual_seed(20 + L)
    s = 2.0 if wide else 1.0
    p = mr.make_params(64, seed=7, wide=wide)
    st = {"u": dtype, "delta_raw": F32, "Bm": F32, "Cm": F32, "z": dtype}
    inputs = {k: _rd(s * torch.randn(B, L, n, generator=g, dtype=F64), st[k])
              for k, n in (("u", D), ("delta_raw", D), ("Bm", 16), ("Cm", 16), ("z", D))}
    inputs["A_log"], inputs["D"] = _rd(p["A_log"], F32), _rd(p["D"], F32)
    dt_bias = _rd(p["dt_proj.bias"], F32)
    dout = _rd(torch.randn(B, L, D, generator=g, dtype=F64), dtype)

    def run(dt):
        return _grads(lambda t: mr.scan_ref(t["u"], t["delta_raw"], dt_bias.to(dt), t["A_log"], t["Bm"], t["Cm"], t["D"],
                                            t["z"], reverse), inputs, dout, dt)
    return inputs, dt_bias, dout, run(F64), run(F32)


def _scan_lengths():
    c = int(_lib().selective_scan_chunk())
    return sorted({1, 5, c - 1, c, c + 1, 2 * c + 3})


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_scan_kernel(dtype, reverse, wide):
    ops, lib = _ops(), _lib()
    st16 = ST[dtype]
    for L in _scan_lengths():
        inputs, dt_bias, dout, r64, r32 = _scan_case(dtype, L, reverse, wide)
        M = B * L
        flat = lambda k: inputs[k].reshape(M, -1)
        z, xz, g_xz = _half(flat("z"), dtype, True, "xz")                    # z: the right column half
        xd = torch.full((M, R + 32), float("nan"), dtype=F64)                # Bm / Cm: slices of an x_dbl-shaped fp32 buffer
        xd[:, R:R + 16], xd[:, R + 16:] = flat("Bm"), flat("Cm")
        x_dbl, g_xd = _in(xd, F32, "x_dbl")
        u, g_u = _in(flat("u"), dtype, "u")
        raw, g_raw = _in(flat("delta_raw"), F32, "delta_raw")
        A_log, g_A = _in(inputs["A_log"], F32, "A_log")
        Dp, g_D = _in(inputs["D"], F32, "D")
        bias, g_bias = _in(dt_bias, F32, "dt_bias")
        dy, g_dy = _in(dout.reshape(M, D), dtype, "dy")
        nsaved = int(lib.selective_scan_saved_floats(B, L, D))
        y, g_y = _out((M, D), dtype, "y")
        y2, g_y2 = _out((M, D), dtype, "y (no tape)")
        saved, g_saved = _out((nsaved,), F32, "saved")
        ws = moat.moat_workspace(ops, int(lib.selective_scan_workspace_bytes(B, L, D)), 0xFF, DEV)
        Bm, Cm = x_dbl[:, R:R + 16], x_dbl[:, R + 16:]
        fwd = lambda yy, sv: lib.h16_selective_scan_fwd(
            st16, u.data_ptr(), D, raw.data_ptr(), D, bias.data_ptr(), A_log.data_ptr(), Bm.data_ptr(), R + 32, Cm.data_ptr(),
            R + 32, Dp.data_ptr(), z.data_ptr(), 2 * D, yy.data_ptr(), D, sv, B, L, D, int(reverse), ws.ptr, ws.nbytes, _st())
        fwd(y, saved.data_ptr())
        fwd(y2, 0)
        assert torch.equal(moat.bits(y), moat.bits(y2))
        # the backward reads the checkpoints out of NaN moats of their own
        saved_r, g_sr = moat.embed(saved.clone(), MOAT, MOAT, "nan", "saved (read)")
        dxz, g_dxz = _out((M, 2 * D), dtype, "dxz")
        dxdbl, g_dxd = _out((M, R + 32), F32, "dxdbl")
        du, g_du = _out((M, D), F32, "du")
        dd, g_dd = _out((M, D), F32, "ddelta")
        dA, g_dA = _out((D, 16), F32, "dA_log")
        dD, g_dD = _out((D,), F32, "dD")
        keep_xz, keep_xd = moat.bits(dxz[:, :D]).clone(), moat.bits(dxdbl[:, :R]).clone()
        lib.h16_selective_scan_bwd(
            st16, u.data_ptr(), D, raw.data_ptr(), D, bias.data_ptr(), A_log.data_ptr(), Bm.data_ptr(), R + 32, Cm.data_ptr(),
            R + 32, Dp.data_ptr(), z.data_ptr(), 2 * D, dy.data_ptr(), D, saved_r.data_ptr(), du.data_ptr(), D, dd.data_ptr(), D,
            dxdbl[:, R:R + 16].data_ptr(), R + 32, dxdbl[:, R + 16:].data_ptr(), R + 32, dxz[:, D:].data_ptr(), 2 * D,
            dA.data_ptr(), dD.data_ptr(), B, L, D, int(reverse), ws.ptr, ws.nbytes, _st())
        torch.cuda.synchronize()
        for g in (g_xz, g_xd, g_u, g_raw, g_A, g_D, g_bias, g_dy, g_y, g_y2, g_saved, g_sr, g_dxz, g_dxd, g_du, g_dd, g_dA,
                  g_dD, ws.guard):
            g()
        assert torch.equal(moat.bits(dxz[:, :D]), keep_xz) and torch.equal(moat.bits(dxdbl[:, :R]), keep_xd)
        hip = {"y": y, "du": du, "ddelta_raw": dd, "dBm": dxdbl[:, R:R + 16], "dCm": dxdbl[:, R + 16:], "dz": dxz[:, D:],
               "dA_log": dA, "dD": dD}
        _gate(f"scan {_name(dtype)} L={L} rev={int(reverse)} {'wide' if wide else 'default'}", hip, r32, r64, dtype,
              out16=("y", "dz"))


# ---- 3. the whole layer ---------------------------------------------------------------------------------------------
def _layer_len():
    return 2 * int(_lib().selective_scan_chunk()) + 3


@functools.lru_cache(maxsize=None)
def _layer_case(dtype, d_model, reverse):
    """-> params (fp32-representable), u, dout (`dtype`-representable), the fp64 / fp32 / rounded-fp64 runs"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    L = _layer_len()
    p = {k: _rd(v, F32) for k, v in mr.make_params(d_model, seed=d_model).items()}
    u, dout = (_rd(t, dtype) for t in mr.make_input(d_model, B, L, seed=d_model))
    return (p, u, dout, mr.layer_run(p, u, dout, reverse, F64), mr.layer_run(p, u, dout, reverse, F32),
            m16.layer_run16(p, u, dout, reverse, m16.rounder(dtype)))


def _module(p, d_model):
    from deepsense6g_tii_amd.mamba import Mamba
    m = Mamba(d_model, device=DEV)
    m.load_state_dict({k: v.float() for k, v in p.items()}, strict=True)
    return m.train()


def _hip_layer(m, u, dout, dtype, reverse):
    for q in m.parameters():
        q.grad = None
    ud, g_u = _in(u, dtype, "u")
    dd, g_d = _in(dout, dtype, "dout")
    ud.requires_grad_(True)
    out = m(ud, reverse=reverse)
    out.backward(dd)
    torch.cuda.synchronize()
    g_u()
    g_d()
    assert out.dtype == dtype and ud.grad.dtype == dtype
    res = {"out": out.detach(), "input": ud.grad}
    res.update({k: q.grad for k, q in m.named_parameters()})
    assert set(res) == {"out", "input", *mr.NAMES} and all(res[k].dtype == F32 for k in mr.NAMES)
    return res


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d_model", [64, 512])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_layer(dtype, d_model, reverse):
    p, u, dout, r64, r32, rr = _layer_case(dtype, d_model, reverse)
    hip = _hip_layer(_module(p, d_model), u, dout, dtype, reverse)
    tag = f"layer {_name(dtype)} d={d_model} B={B} L={_layer_len()} rev={int(reverse)}"
    bad = []
    print()
    for k in r64:
        e_hip, e_round, b32 = mr.rel_err(hip[k], r64[k]), mr.rel_err(rr[k], r64[k]), mr.bar(mr.rel_err(r32[k], r64[k]))
        bar = 3 * e_round + b32
        print(f"parity16 {tag:<40s} {k:<16s} e_hip {e_hip:.3e}  e_round {e_round:.3e}  ratio {e_hip / e_round if e_round else float('nan'):5.2f}  "
              f"bar {bar:.3e}")
        if not e_hip <= bar:
            bad.append((k, e_hip, e_round))
    assert not bad, (tag, bad)


# ---- 4. direction, determinism ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_reverse_is_flip_forward_flip(dtype):
    p, u, dout, *_ = _layer_case(dtype, 64, False)
    m = _module(p, 64)
    a = _hip_layer(m, u, dout, dtype, True)
    b = _hip_layer(m, u.flip(1), dout.flip(1), dtype, False)
    assert torch.equal(moat.bits(a["out"]), moat.bits(b["out"].flip(1)))
    assert torch.equal(moat.bits(a["input"]), moat.bits(b["input"].flip(1)))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_layer_is_deterministic(dtype):
    p, u, dout, *_ = _layer_case(dtype, 64, False)
    a = _hip_layer(_module(p, 64), u, dout, dtype, False)
    b = _hip_layer(_module(p, 64), u, dout, dtype, False)
    for k in a:
        assert torch.equal(moat.bits(a[k]), moat.bits(b[k])), k


# ---- 5. gradient destinations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gradient_destinations(dtype):
    from deepsense6g_tii_amd.mamba import layer_backward, layer_forward
    p, u, dout, *_ = _layer_case(dtype, 64, True)
    m = _module(p, 64)
    L = _layer_len()
    params = [q.detach() for q in m._params()]
    ws = m._workspace(torch.device(DEV), B, L)
    u2 = u.to(dtype).reshape(B * L, 64).to(DEV)
    d2 = dout.to(dtype).reshape(B * L, 64).to(DEV)
    out, tape = layer_forward(m, ws, True, True, u2, B, L, params)
    du0, g0 = layer_backward(m, ws, True, B, L, tape, params, d2)
    assert out.dtype == dtype and du0.dtype == dtype and all(g.dtype == F32 for g in g0)
    gen = torch.Generator().manual_seed(5)
    for acc in (0, 1):
        pre = [torch.randn(g.shape, generator=gen).to(DEV) for g in g0]
        dst = [t.clone() if acc else torch.full_like(t, float("nan")) for t in pre]
        du, none = layer_backward(m, ws, True, B, L, tape, params, d2, gdst=[(t.data_ptr(), acc) for t in dst])
        assert none is None and torch.equal(moat.bits(du), moat.bits(du0))
        for k, t, g, s in zip(mr.NAMES, dst, g0, pre):
            if not acc:
                assert torch.equal(t, g), k                    # flag 0: the returned-gradient form bit for bit
            else:                                              # flag 1: one fp32 add onto the seed
                assert mr.rel_err(t, s.double().cpu() + g.double().cpu()) <= 1e-5, k
    # du_out: the input gradient is added to an existing one, 16-bit (one rounding of the sum) or fp32
    for dt in (dtype, F32):
        seed = torch.randn(B * L, 64, generator=gen).to(dt).to(DEV)
        acc_to = seed.clone()
        du, _ = layer_backward(m, ws, True, B, L, tape, params, d2, du_out=acc_to)
        assert du.data_ptr() == acc_to.data_ptr()
        want = seed.double().cpu() + du0.double().cpu()
        # 16-bit: round(seed + du0) exactly; fp32: seed + the unrounded du, which du0 is one 16-bit rounding away from
        tol = (U16[dtype] if dt == dtype else 2.0 ** -22) * want.abs() + 1.01 * U16[dtype] * du0.double().cpu().abs()
        assert ((acc_to.double().cpu() - want).abs() <= tol + 1e-30).all(), dt


# ---- 6. the module surface --------------------------------------------------------------------------------------------
def test_module_runs_bf16_and_keeps_its_fp32_bits():
    from deepsense6g_tii_amd.mamba import Mamba
    torch.manual_seed(0)
    m = Mamba(64).to("cuda")
    m.train()
    u = torch.randn(2, 70, 64, device="cuda")
    with torch.no_grad():
        before = m(u).clone()
    ub = u.bfloat16().requires_grad_(True)
    out = m(ub)
    assert out.dtype == torch.bfloat16 and out.shape == u.shape and out.requires_grad
    out.float().square().mean().backward()
    assert ub.grad.dtype == torch.bfloat16 and torch.isfinite(ub.grad.float()).all() and ub.grad.float().abs().max() > 0
    for k, q in m.named_parameters():
        assert q.dtype == F32 and q.grad.dtype == F32 and torch.isfinite(q.grad).all(), k
        assert q.grad.abs().max() > 0, k
    with torch.no_grad():
        assert mr.rel_err(out.detach().float(), before.double().cpu()) < 0.05
        q = m(ub.detach())
        assert q.dtype == torch.bfloat16 and torch.equal(moat.bits(q), moat.bits(out.detach()))
        assert m(u.half()).dtype == torch.float16
        after = m(u)
    assert torch.equal(moat.bits(after), moat.bits(before))   # workspace and weight copies do not leak between the paths


# ---- 7. the wrappers pick the entry point and type every operand ------------------------------------------------------
_ENTRIES = ("causal_conv1d_silu_fwd", "causal_conv1d_silu_bwd", "selective_scan_fwd", "selective_scan_bwd")


def test_wrappers_pick_entry_by_storage_and_refuse_mixed_operands(monkeypatch):
    """ops.causal_conv1d_silu_* / ops.selective_scan_* on fp32, bf16 and f16: which of the eight entry points is called, with
    which storage code and row strides, and that an operand of the wrong dtype is refused before anything is called.  The
    entry points are replaced by recording stubs for the test: no kernel runs, so none reads mistyped memory."""
    ops, lib = _ops(), _lib()
    calls = []
    for e in _ENTRIES:
        for name in (e, "h16_" + e):
            monkeypatch.setattr(lib, name, lambda *a, _n=name: calls.append((_n, a)))
    Bq, L, M, X = 1, 4, 4, R + 32
    ws = ops.Workspace(torch.device(DEV), max(int(lib.selective_scan_workspace_bytes(Bq, L, D)),
                                              int(lib.causal_conv1d_workspace_bytes(Bq, L, D))))
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=DEV)
    w, bias, dtb, A_log, Dp = z(D, 1, 4), z(D), z(D), z(D, 16), z(D)
    draw, du, dd, x_dbl, dxdbl = z(M, D), z(M, D), z(M, D), z(M, X), z(M, X)
    saved = z(int(lib.selective_scan_saved_floats(Bq, L, D)))
    Bm, Cm, dBm, dCm = x_dbl[:, R:R + 16], x_dbl[:, R + 16:], dxdbl[:, R:R + 16], dxdbl[:, R + 16:]
    wide = {dt: (z(M, 2 * D, dt=dt), z(M, 2 * D, dt=dt), z(M, D, dt=dt)) for dt in (F32, *DTYPES)}   # xz, dxz, dy

    def one(fn, *a, **k):
        """-> (entry name, its arguments without the stream, what the wrapper returned) of the ONE call fn makes"""
        del calls[:]
        ret = fn(*a, **k)
        assert len(calls) == 1, calls
        return calls[0][0], calls[0][1][:-1], ret

    for dt in (F32, *DTYPES):
        xz, dxz, dy = wide[dt]
        x, zz, dx, dz = xz[:, :D], xz[:, D:], dxz[:, :D], dxz[:, D:]

        def entry(name, args):
            """the entry point of this storage was called; -> its arguments after the storage code"""
            if dt == F32:
                assert name == entry.want, (name, dt)
                return args
            assert name == "h16_" + entry.want and args[0] == ST[dt], (name, args[0], dt)
            return args[1:]

        entry.want = "causal_conv1d_silu_fwd"
        name, args, y = one(ops.causal_conv1d_silu_fwd, x, w, bias, Bq, L)
        a = entry(name, args)
        assert y.dtype == dt and tuple(y.shape) == (M, D)
        assert a == (x.data_ptr(), 2 * D, w.data_ptr(), bias.data_ptr(), y.data_ptr(), D, Bq, L, D, 0)

        entry.want = "causal_conv1d_silu_bwd"
        dwb = (z(D, 1, 4), z(D))
        name, args, _ = one(ops.causal_conv1d_silu_bwd, x, w, bias, dy, dx, Bq, L, ws, out=dwb)
        a = entry(name, args)
        assert a == (x.data_ptr(), 2 * D, w.data_ptr(), bias.data_ptr(), dy.data_ptr(), D, dx.data_ptr(), 2 * D,
                     dwb[0].data_ptr(), dwb[1].data_ptr(), Bq, L, D, 0, ws.ptr, ws.nbytes)

        entry.want = "selective_scan_fwd"
        name, args, (y, sv) = one(ops.selective_scan_fwd, x, draw, dtb, A_log, Bm, Cm, Dp, zz, Bq, L, ws, save=True)
        a = entry(name, args)
        assert y.dtype == dt and tuple(y.shape) == (M, D) and sv.dtype == F32
        assert a == (x.data_ptr(), 2 * D, draw.data_ptr(), D, dtb.data_ptr(), A_log.data_ptr(), Bm.data_ptr(), X, Cm.data_ptr(),
                     X, Dp.data_ptr(), zz.data_ptr(), 2 * D, y.data_ptr(), D, sv.data_ptr(), Bq, L, D, 0, ws.ptr, ws.nbytes)

        entry.want = "selective_scan_bwd"
        dAD = (z(D, 16), z(D))
        name, args, _ = one(ops.selective_scan_bwd, x, draw, dtb, A_log, Bm, Cm, Dp, zz, dy, saved, du, dd, dBm, dCm, dz, Bq, L,
                            ws, out=dAD)
        a = entry(name, args)
        assert a == (x.data_ptr(), 2 * D, draw.data_ptr(), D, dtb.data_ptr(), A_log.data_ptr(), Bm.data_ptr(), X, Cm.data_ptr(),
                     X, Dp.data_ptr(), zz.data_ptr(), 2 * D, dy.data_ptr(), D, saved.data_ptr(), du.data_ptr(), D,
                     dd.data_ptr(), D, dBm.data_ptr(), X, dCm.data_ptr(), X, dz.data_ptr(), 2 * D, dAD[0].data_ptr(),
                     dAD[1].data_ptr(), Bq, L, D, 0, ws.ptr, ws.nbytes)

    bf, hf = torch.bfloat16, torch.float16
    (xz32, dxz32, dy32), (xzb, dxzb, dyb), (xzh, dxzh, dyh) = wide[F32], wide[bf], wide[hf]
    scan_f = lambda u, raw, zz: ops.selective_scan_fwd(u, raw, dtb, A_log, Bm, Cm, Dp, zz, Bq, L, ws)
    scan_b = lambda u, zz, dy, du_, dz: ops.selective_scan_bwd(u, draw, dtb, A_log, Bm, Cm, Dp, zz, dy, saved, du_, dd, dBm,
                                                              dCm, dz, Bq, L, ws)
    mixed = {
        "conv bwd: fp32 x, bf16 dy": lambda: ops.causal_conv1d_silu_bwd(xz32[:, :D], w, bias, dyb, dxz32[:, :D], Bq, L, ws),
        "conv bwd: bf16 x, f16 dx": lambda: ops.causal_conv1d_silu_bwd(xzb[:, :D], w, bias, dyb, dxzh[:, :D], Bq, L, ws),
        "scan fwd: bf16 u, f16 z": lambda: scan_f(xzb[:, :D], draw, xzh[:, D:]),
        "scan fwd: bf16 u, bf16 delta_raw": lambda: scan_f(xzb[:, :D], z(M, D, dt=bf), xzb[:, D:]),
        "scan bwd: f16 u, fp32 dz": lambda: scan_b(xzh[:, :D], xzh[:, D:], dyh, du, dxz32[:, D:]),
        "scan bwd: fp32 u, bf16 du": lambda: scan_b(xz32[:, :D], xz32[:, D:], dy32, z(M, D, dt=bf), dxz32[:, D:]),
    }
    for what, call in mixed.items():
        del calls[:]
        with pytest.raises(AssertionError):
            call()
        assert not calls, (what, calls)
