"""What ran is what was planned: one conv / linear call per case, every pointer inside the moats of tests/moat.py, bracketed by
ds6g_profile_begin / _end.  The single profile record carries the variant of ds6g_gemm_plan's plan for that call and the flops
of the formula (2 Mg Ng Kg; 2 Mg Ng R S K over the parity classes of the fp32 stride-2 dgrad), the guards are intact, and the
result matches torch in fp64 at the tolerance of the op's own test (tests/test_ops_gpu.py: 2e-5 fwd / dgrad, 1e-4 wgrad;
tests/test_bgemm_gpu.py and tests/test_f16_gpu.py: one rounding of a 16-bit output, 3e-5 / 2e-5 of the largest fp32 one)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import moat
from tests.test_gemm_plan_cpu import (ACCUMULATE, BIAS_ACT, BNSTATS, CONV_DGRAD, CONV_FWD, CONV_WGRAD, DBIAS, EPILOGUE, F32, H16,
                                      LIN_DGRAD, LIN_FWD, LIN_WGRAD, OUT16, cdiv, conv, linear, query)
from tests.test_moat_gpu import IO, ST, WS, I, O, Run, _gen, _lib, _ops, rnd
from tests.test_ops_gpu import close

pytestmark = pytest.mark.gpu
F64 = torch.float64


def planned(name, args, family, op, shape, flags, ws_bytes=0, flops=None):
    """runs entry point `name` once with moated arguments and a moated workspace of exactly ws_bytes (the WS pair) inside a
    profile bracket -> (outputs in argument order, a copy of the plan's int fields)"""
    L = _lib()
    rc, p = query(family, op, shape, flags, ws_bytes)
    assert rc == 0, (name, shape, rc)
    plan = {n: getattr(p, n) for n, _ in p._fields_}
    ws = moat.moat_workspace(_ops(), max(ws_bytes, 4), 0xFF) if any(a is WS for a in args) else None
    r = Run(args, True, ws, ws_bytes=ws_bytes)
    L.profile_begin(8)
    try:
        r.call(getattr(L, name))
    finally:
        variants, fl, ms = (ctypes.c_int * 8)(), (ctypes.c_double * 8)(), (ctypes.c_float * 8)()
        n = L.profile_end(variants, fl, ms, 8)
    assert n == 1 and variants[0] == plan["variant"], (name, shape, n, list(variants[:n]), plan)
    if family == F32:
        assert L.last_igemm_variant() == plan["variant"]
    want = 2.0 * plan["Mg"] * plan["Ng"] * plan["Kg"] if flops is None else flops
    assert fl[0] == want, (name, shape, fl[0], want)
    r.check_guards()
    for out in r.outs:
        assert not bool(torch.isnan(out).any()), (name, shape, "NaN in an output")
    return r.outs, plan


def conv_ref(x, w, dy, stride, pad):
    """NHWC / OHWI device tensors -> y, dx, dw in fp64 on the CPU, in the kernels' layouts"""
    xd = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wd = w.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.conv2d(xd, wd, None, stride, pad)
    y.backward(dy.double().cpu().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xd.grad.permute(0, 2, 3, 1), wd.grad.permute(0, 2, 3, 1)


# ---- fp32 storage -----------------------------------------------------------------------------------------------------------
def test_fp32_conv_runs_its_plans(dev):
    N, HW, C, K, R = 2, 8, 64, 64, 3
    shape = conv(N, HW, C, K, R, 1)
    g = _gen("plan-conv", *shape)
    sh = (HW + 1) * 64
    x, w, dy = rnd(g, N, HW, HW, C), rnd(g, K, R, R, C, scale=1 / math.sqrt(C * R * R)), rnd(g, N, HW, HW, K)
    y_ref, dx_ref, dw_ref = conv_ref(x, w, dy, 1, 1)
    (y,), p = planned("conv2d_fwd", [I(x, sh), I(w, sh), O(N, HW, HW, K), *shape], F32, CONV_FWD, shape, 0)
    close(y, y_ref, 2e-5, 2e-5)
    assert (p["walk"], p["epilogue"], p["nclass"]) == (1, 0, 0)
    (dx,), p = planned("conv2d_dgrad", [I(dy, sh), I(w, sh), O(N, HW, HW, C), *shape, 0], F32, CONV_DGRAD, shape, 0)
    close(dx, dx_ref, 2e-5, 2e-5)
    slab = K * R * R * C * 4
    # on a roomy workspace, on exactly 4 slabs while accumulating, and with no workspace at all (the direct launch)
    (dw,), p = planned("conv2d_wgrad", [I(x, sh), I(dy, sh), O(K, R, R, C), *shape, 0, WS], F32, CONV_WGRAD, shape, 0, 1 << 20)
    close(dw, dw_ref, 1e-4, 1e-4)
    assert p["splits"] == 2 and p["reduce"] == 1 and p["wg_rows"] == 2                         # 128 pixels, >= 64 per split
    base = rnd(g, K, R, R, C)
    (dw,), p = planned("conv2d_wgrad", [I(x, sh), I(dy, sh), IO(base), *shape, 1, WS], F32, CONV_WGRAD, shape, ACCUMULATE, 4 * slab)
    close(dw, dw_ref + base.double().cpu(), 1e-4, 1e-4)
    assert p["reduce"] == 1 and p["ws_bytes_used"] <= 4 * slab
    (dw,), p = planned("conv2d_wgrad", [I(x, sh), I(dy, sh), O(K, R, R, C), *shape, 0, 0, 0], F32, CONV_WGRAD, shape, 0, 0)
    close(dw, dw_ref, 1e-4, 1e-4)
    assert (p["splits"], p["reduce"]) == (1, 0)


def test_fp32_stride2_dgrad_runs_its_parity_classes(dev):
    N, HW, C, K, R = 2, 8, 64, 64, 3
    shape = conv(N, HW, C, K, R, 2)
    g = _gen("plan-s2", *shape)
    x, w, dy = rnd(g, N, HW, HW, C), rnd(g, K, R, R, C, scale=1 / math.sqrt(C * R * R)), rnd(g, N, HW // 2, HW // 2, K)
    _, dx_ref, _ = conv_ref(x, w, dy, 2, 1)
    (dx,), p = planned("conv2d_dgrad", [I(dy, 640), I(w, 640), O(N, HW, HW, C), *shape, 0], F32, CONV_DGRAD, shape, 0,
                       flops=2.0 * (N * 4 * 4) * C * (R * R) * K)
    close(dx, dx_ref, 2e-5, 2e-5)
    assert (p["nclass"], p["grid_y"], p["epilogue"], p["Kg"]) == (4, 4, 1, 4 * K)


def test_fp32_stem_like_conv_runs_the_general_walk(dev):
    shape = (1, 16, 16, 4, 64, 7, 7, 2, 3)
    g = _gen("plan-stem", *shape)
    x, w = rnd(g, 1, 16, 16, 4), rnd(g, 64, 7, 7, 4, scale=1 / 14)
    y_ref, _, _ = conv_ref(x, w, torch.zeros(1, 8, 8, 64), 2, 3)
    (y,), p = planned("conv2d_fwd", [I(x, 256), I(w, 256), O(1, 8, 8, 64), *shape], F32, CONV_FWD, shape, 0)
    close(y, y_ref, 2e-5, 2e-5)
    assert (p["walk"], p["bk"], p["variant"]) == (0, 16, 2)


def test_fp32_linear_runs_its_plans(dev):
    M, N, K = 130, 72, 64
    shape = linear(M, N, K)
    g = _gen("plan-lin", M, N, K)
    x, w, b, res = rnd(g, M, K), rnd(g, N, K, scale=1 / 8), rnd(g, N), rnd(g, M, N)
    dy, msk = rnd(g, M, N), rnd(g, M, K)
    xd, wd, dyd = x.double().cpu(), w.double().cpu(), dy.double().cpu()
    (y,), p = planned("linear_fwd", [I(x), I(w), I(b), O(M, N), M, N, K, 1, I(res), 0.0, 0, 0], F32, LIN_FWD, shape, EPILOGUE)
    close(y, torch.relu(xd @ wd.t() + b.double().cpu()) + res.double().cpu(), 2e-5, 2e-5)
    assert p["epilogue"] == 1
    (dx,), p = planned("linear_dgrad", [I(dy), I(w), O(M, K), M, N, K, I(msk), 0], F32, LIN_DGRAD, shape, EPILOGUE)
    close(dx, (dyd @ wd) * (msk.cpu() > 0), 2e-5, 2e-5)
    (dw, db), p = planned("linear_wgrad", [I(x), I(dy), O(N, K), O(N), M, N, K, 0, WS], F32, LIN_WGRAD, shape, DBIAS, 1 << 20)
    close(dw, dyd.t() @ xd, 1e-4, 1e-4)
    close(db, dyd.sum(0), 1e-4, 1e-4)
    assert p["reduce"] == 1 and p["want_colsum"] == 1 and p["slab_elems"] == N * K + N


# ---- 16-bit storage ---------------------------------------------------------------------------------------------------------
def one_rounding(st16, got, ref, roundings=1):
    """a 16-bit output: tests/test_bgemm_gpu.py close16 (bf16), tests/test_f16_gpu.py within_one_rounding (f16)"""
    got, ref = got.double().cpu(), ref.double().cpu()
    u, slack = (2.0 ** -8, 3e-5) if st16 == 1 else (2.0 ** -11, 2e-5)
    bound = ref.abs() * u * roundings + slack * ref.abs().max()
    assert bool(((got - ref).abs() <= bound).all()), ((got - ref).abs() - bound).max().item()


def close32(st16, got, ref):
    """an fp32 weight gradient: 3e-5 (test_bgemm_gpu) / 2e-5 (test_f16_gpu) of the largest entry"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert (got - ref).abs().max().item() <= (3e-5 if st16 == 1 else 2e-5) * ref.abs().max().item()


@pytest.mark.parametrize("st16", [1, 2], ids=["bf16", "f16"])
def test_16bit_conv_runs_its_plans(dev, st16):
    T = ST[st16]
    N, HW, C, K, R = 2, 8, 64, 64, 3
    g = _gen("plan-conv16", st16)
    w = rnd(g, K, R, R, C, dtype=T, scale=1 / math.sqrt(C * R * R))
    for stride in (1, 2):
        shape = conv(N, HW, C, K, R, stride)
        Ho = HW // stride
        sh = (HW + 1) * 64
        x, dy = rnd(g, N, HW, HW, C, dtype=T), rnd(g, N, Ho, Ho, K, dtype=T)
        y_ref, dx_ref, dw_ref = conv_ref(x, w, dy, stride, 1)
        (dx,), p = planned("h16_conv2d_dgrad", [st16, I(dy, sh), I(w, sh), O(N, HW, HW, C, dtype=T), 1, *shape, 0], H16, CONV_DGRAD,
                           shape, OUT16)
        one_rounding(st16, dx, dx_ref)
        assert p["nclass"] == (4 if stride == 2 else 0) and p["epilogue"] == 0 and p["variant"] == 30111
        if stride == 2:
            continue
        (y,), p = planned("h16_conv2d_fwd", [st16, I(x, sh), I(w, sh), O(N, Ho, Ho, K, dtype=T), 1, *shape], H16, CONV_FWD, shape, OUT16)
        one_rounding(st16, y, y_ref)
        # Wo = 8: a k-tile of 64 pixels is 8 whole output rows
        (dw,), p = planned("h16_conv2d_wgrad", [st16, I(x, sh), I(dy, sh), O(K, R, R, C), *shape, 0, WS], H16, CONV_WGRAD, shape, 0, 1 << 20)
        close32(st16, dw, dw_ref)
        assert (p["wg_rows"], p["splits"], p["reduce"], p["variant"]) == (8, 1, 0, 30021)
        # the inference conv: bias, ReLU after the 16-bit residual
        bias, res = rnd(g, K), rnd(g, N, Ho, Ho, K, dtype=T)
        (yb,), p = planned("h16_conv2d_bias_act_fwd", [st16, I(x, sh), I(w, sh), I(bias), I(res), O(N, Ho, Ho, K, dtype=T), *shape, 2],
                           H16, BIAS_ACT, shape, 0)
        one_rounding(st16, yb, torch.relu(y_ref + bias.double().cpu() + res.double().cpu()))
        assert p["variant"] == 30201
        # the conv with the BatchNorm statistics of its stored output
        need = cdiv(N * Ho * Ho, 64) * 2 * K * 8
        (y2, mean, invstd), p = planned("h16_conv2d_fwd_bnstats", [st16, I(x, sh), I(w, sh), O(N, Ho, Ho, K, dtype=T), *shape, 1e-5, 0.1,
                                                                 O(K), O(K), 0, 0, WS], H16, BNSTATS, shape, 0, need)
        assert torch.equal(moat.bits(y2), moat.bits(y)) and p["ws_bytes_used"] == need
        yd = y2.double().cpu().reshape(-1, K)
        assert (mean.double().cpu() - yd.mean(0)).abs().max() <= 1e-5 * yd.mean(0).abs().max()
        inv_ref = 1.0 / torch.sqrt(yd.var(0, unbiased=False) + 1e-5)
        assert (invstd.double().cpu() - inv_ref).abs().max() <= 1e-5 * inv_ref.abs().max()


@pytest.mark.parametrize("st16", [1, 2], ids=["bf16", "f16"])
def test_16bit_linear_runs_its_plans(dev, st16):
    T = ST[st16]
    M, N, K = 130, 72, 64
    g = _gen("plan-lin16", st16)
    x, w, dy = rnd(g, M, K, dtype=T), rnd(g, N, K, dtype=T, scale=1 / 8), rnd(g, M, N, dtype=T)
    xd, wd, dyd = x.double().cpu(), w.double().cpu(), dy.double().cpu()
    (y,), p = planned("h16_linear_fwd", [st16, I(x), I(w), 0, O(M, N, dtype=T), 1, M, N, K, 0, 0, 0.0, 0, 0], H16, LIN_FWD,
                      linear(M, N, K), OUT16)
    one_rounding(st16, y, xd @ wd.t())
    assert p["variant"] == 30101
    (dw, db), p = planned("h16_linear_wgrad", [st16, I(x), I(dy), O(N, K), O(N), M, N, K, 0, WS], H16, LIN_WGRAD, linear(M, N, K),
                          DBIAS, 1 << 20)
    close32(st16, dw, dyd.t() @ xd)
    close32(st16, db, dyd.sum(0))
    assert p["reduce"] == 1 and p["want_colsum"] == 1 and p["variant"] == 30021
    # the data gradient reduces over the 72 outputs, and the 16-bit kernels take whole 64-element k-tiles only: this layer's is
    # refused (the model keeps such a layer in fp32 storage); the 72 -> 64 layer's runs, 64 on the reduced side
    assert query(H16, LIN_DGRAD, linear(M, N, K), OUT16, 0)[0] == 1
    w2, dy2 = rnd(g, 64, N, dtype=T, scale=1 / 8), rnd(g, M, 64, dtype=T)
    (dx,), p = planned("h16_linear_dgrad", [st16, I(dy2), I(w2), O(M, N, dtype=T), 1, M, 64, N, 0, 0, 0], H16, LIN_DGRAD,
                       linear(M, 64, N), OUT16)
    one_rounding(st16, dx, dy2.double().cpu() @ w2.double().cpu())
    assert p["variant"] == 30111
