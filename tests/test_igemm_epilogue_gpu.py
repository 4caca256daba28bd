"""The fused epilogue of the implicit-GEMM kernels (csrc/igemm.hip): bias, ReLU, ReLU mask, dropout, residual, accumulate and
the strided data gradient's scatter, through the C ABI at the smallest shapes that reach every path.

Rows M in {64, 130} (at 130 the rows beyond Mg fall off the buffer descriptor), columns in {36, 64, 192} (at 36 the columns
beyond Ng inside a tile are dropped), reduction length in {16, 32, 256} (one and two k-tiles: fewer than the pipeline has
stages); the 128 x 64 and 128 x 128 tiles are planned at these sizes through the min_blocks field of ds6g_set_debug_flags and
the plan is asserted with ds6g_gemm_plan.  Everything a kernel reads sits inside NaN moats, everything it writes (pre-filled
with NaN unless it accumulates) inside 0xFF moats (tests/moat.py).

Two checks per case: against torch on the CPU at the tolerance tests/test_ops_gpu.py uses for the same entry points (2e-5),
and BITWISE against the library's own unfused composition wherever that is a chain of single IEEE operations on the same
GEMM result (same shape, so same plan and same accumulators): residual = bias-only call + one add, mask = plain data gradient
+ where(mask > 0, ., 0), accumulate = overwrite call + one add, dropout = bias-only call + ops.dropout (same seed and offset)
+ one add.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import moat
from tests.test_gemm_plan_cpu import (ACCUMULATE, CONV_DGRAD, EPILOGUE, F32, LIN_DGRAD, LIN_FWD, linear, query)

pytestmark = pytest.mark.gpu

MOAT = moat.MIN_MOAT
ROWS, COLS, REDS = (64, 130), (36, 64, 192), (16, 32, 256)
SHAPES = [(m, n, k) for m in ROWS for n in COLS for k in REDS]
TILE_SHAPES = [((130, 192, 32), (128, 128)), ((130, 36, 32), (128, 64))]      # planned tile under min_blocks = 1
MIN_BLOCKS_1, MIN_BLOCKS_DEFAULT = 1 << 8, 2560 << 8                           # ds6g_set_debug_flags, bits 8-19
DROP_P, SEED, SEED_OFF = 0.1, 1234, 77


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


def _lib():
    from deepsense6g_tii_amd._lib import lib
    return lib()


def close(a, b, rtol=2e-5, atol=2e-5):
    a, b = a.float().cpu(), b.float().cpu()
    assert bool(b.abs().max() > 0)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"max err {err:.3e} vs ref max {ref:.3e}"


def same_bits(a, b):
    assert torch.equal(moat.bits(a), moat.bits(b)), f"{int((moat.bits(a) != moat.bits(b)).sum())} elements differ"


class Bufs:
    """moated operands of one test; check() asserts every guard"""

    def __init__(self):
        self.guards = []

    def rd(self, t, name):
        v, g = moat.embed(t.contiguous().cuda(), MOAT, MOAT, "nan", name)
        self.guards.append(g)
        return v

    def wr(self, shape, name, init=None):
        t = init.contiguous().cuda() if init is not None else moat.nan_like(torch.empty(shape, dtype=torch.float32, device="cuda"))
        v, g = moat.embed(t, MOAT, MOAT, 0xFF, name)
        self.guards.append(g)
        return v

    def check(self):
        torch.cuda.synchronize()
        for g in self.guards:
            g()


@functools.lru_cache(maxsize=None)
def _linear_case(M, N, K):
    """inputs and CPU references of y[M][N] = x[M][K] w[N][K]^T + b, computed once per shape and never modified"""
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    return x, w, b, res, F.linear(x, w, b), F.linear(x, w)


@functools.lru_cache(maxsize=None)
def _dgrad_case(M, NC, KR):
    """dx[M][NC] = dy[M][KR] w[KR][NC]: NC is the GEMM's column count, KR its reduction length"""
    g = torch.Generator().manual_seed(M * 1000003 + NC * 1009 + KR + 1)
    dy = torch.randn(M, KR, generator=g)
    w = torch.randn(KR, NC, generator=g) / math.sqrt(KR)
    mask = torch.randn(M, NC, generator=g)
    base = torch.randn(M, NC, generator=g)
    return dy, w, mask, base, dy @ w


def _plan_tile(op, shape, flags):
    rc, p = query(F32, op, shape, flags, 0)
    assert rc == 0
    return p.BM, p.BN


def _run_linear_fwd(M, N, K, tile):
    ops = _ops()
    x, w, b, res, y_ref, y0_ref = _linear_case(M, N, K)
    assert _plan_tile(LIN_FWD, linear(M, N, K), EPILOGUE) == tile and _plan_tile(LIN_FWD, linear(M, N, K), 0) == tile
    B = Bufs()
    xg, wg, bg, rg = B.rd(x, "x"), B.rd(w, "w"), B.rd(b, "bias"), B.rd(res, "residual")
    wp, bp = wg.data_ptr(), bg.data_ptr()
    out = lambda name: B.wr((M, N), name)
    y_b = ops.linear_fwd(xg, wp, bp, N, out=out("y bias"))
    y_relu = ops.linear_fwd(xg, wp, bp, N, relu=True, out=out("y bias relu"))
    y_br = ops.linear_fwd(xg, wp, bp, N, residual=rg, out=out("y bias residual"))
    y_bdr = ops.linear_fwd(xg, wp, bp, N, residual=rg, drop_p=DROP_P, seed=SEED, seed_off=SEED_OFF, out=out("y bias dropout residual"))
    y_r = ops.linear_fwd(xg, wp, 0, N, residual=rg, out=out("y residual"))
    y_0 = ops.linear_fwd(xg, wp, 0, N, out=out("y plain"))
    dropped = ops.dropout(y_b, DROP_P, SEED, SEED_OFF)
    B.check()
    # torch
    close(y_b, y_ref)
    close(y_relu, F.relu(y_ref))
    close(y_br, y_ref + res)
    close(y_r, y0_ref + res)
    close(y_0, y0_ref)
    kept = (ops.dropout(torch.ones(M, N, device="cuda"), DROP_P, SEED, SEED_OFF) != 0).cpu()
    assert 0 < int(kept.sum()) < M * N
    close(y_bdr, y_ref * kept / (1.0 - DROP_P) + res)
    # the unfused composition, bit for bit
    assert torch.equal(y_relu, torch.relu(y_b))
    same_bits(y_br, y_b + rg)
    same_bits(y_r, y_0 + rg)
    same_bits(y_bdr, dropped + rg)


def _run_linear_dgrad(M, NC, KR, tile):
    ops = _ops()
    dy, w, mask, base, dx_ref = _dgrad_case(M, NC, KR)
    shape = linear(M, KR, NC)
    for flags in (0, EPILOGUE, ACCUMULATE, EPILOGUE | ACCUMULATE):
        assert _plan_tile(LIN_DGRAD, shape, flags) == tile
    B = Bufs()
    dyg, wg, mg = B.rd(dy, "dy"), B.rd(w, "w"), B.rd(mask, "mask")
    wp = wg.data_ptr()
    d_plain = ops.linear_dgrad(dyg, wp, NC, out=B.wr((M, NC), "dx"))
    d_mask = ops.linear_dgrad(dyg, wp, NC, relu_mask_src=mg, out=B.wr((M, NC), "dx mask"))
    d_acc = ops.linear_dgrad(dyg, wp, NC, out=B.wr((M, NC), "dx accumulate", init=base), accumulate=True)
    d_macc = ops.linear_dgrad(dyg, wp, NC, relu_mask_src=mg, out=B.wr((M, NC), "dx mask accumulate", init=base), accumulate=True)
    B.check()
    on = mask > 0
    close(d_plain, dx_ref)
    close(d_mask, dx_ref * on)
    close(d_acc, dx_ref + base)
    close(d_macc, dx_ref * on + base)
    masked = torch.where(mg > 0, d_plain, torch.zeros_like(d_plain))
    baseg = base.cuda()
    same_bits(d_mask, masked)
    same_bits(d_acc, d_plain + baseg)
    same_bits(d_macc, masked + baseg)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_forward_epilogues(dev, M, N, K):
    """bias; bias + ReLU; bias + residual; bias + dropout 0.1 + residual; residual without bias; on the 64 x 64 tile"""
    _run_linear_fwd(M, N, K, (64, 64))


@pytest.mark.parametrize("M,NC,KR", SHAPES)
def test_linear_dgrad_epilogues(dev, M, NC, KR):
    """plain; ReLU mask; accumulate into a pre-filled out; mask + accumulate; on the 64 x 64 tile"""
    _run_linear_dgrad(M, NC, KR, (64, 64))


@pytest.mark.parametrize("shape,tile", TILE_SHAPES, ids=["128x128", "128x64"])
def test_epilogues_on_the_larger_tiles(dev, shape, tile):
    """the same cases with the 128 x 128 and 128 x 64 tiles planned at small size (min_blocks = 1)"""
    L = _lib()
    L.set_debug_flags(MIN_BLOCKS_1)
    try:
        _run_linear_fwd(*shape, tile)
        _run_linear_dgrad(*shape, tile)
    finally:
        L.set_debug_flags(MIN_BLOCKS_DEFAULT)    # the override is sticky: back to the default
        L.set_debug_flags(0)
    assert _plan_tile(LIN_FWD, linear(*shape), EPILOGUE) == (64, 64)


STRIDED = [(3, 1, False), (3, 1, True), (1, 0, True)]     # R, pad, accumulate


@pytest.mark.parametrize("R,pad,accumulate", STRIDED, ids=["3x3", "3x3-accumulate", "1x1-accumulate"])
def test_strided_conv_dgrad_scatter(dev, R, pad, accumulate):
    """stride-2 data gradient, run as four input-pixel parity classes whose rows scatter to full-resolution pixels: 3 x 3 with
    and without accumulate, and the 1 x 1 form with accumulate (three of its classes meet no tap and keep their pixels)"""
    ops = _ops()
    N, H, W, C, K = 2, 6, 6, 8, 8
    g = torch.Generator().manual_seed(R * 10 + accumulate)
    x = torch.randn(N, C, H, W, generator=g, requires_grad=True)
    w = torch.randn(K, C, R, R, generator=g) / math.sqrt(C * R * R)
    y = F.conv2d(x, w, None, 2, pad)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    base = torch.randn(N, H, W, C, generator=g)
    rc, p = query(F32, CONV_DGRAD, (N, H, W, C, K, R, R, 2, pad), ACCUMULATE if accumulate else 0, 0)
    assert rc == 0 and p.nclass == 4 and p.grid_y == 4
    B = Bufs()
    dyg = B.rd(dy.permute(0, 2, 3, 1), "dy")
    wg = B.rd(w.permute(0, 2, 3, 1), "w")
    dx = ops.conv2d_dgrad(dyg, wg.data_ptr(), (N, H, W, C), R, R, 2, pad, out=B.wr((N, H, W, C), "dx"))
    ref = x.grad.permute(0, 2, 3, 1)
    if accumulate:
        dxa = ops.conv2d_dgrad(dyg, wg.data_ptr(), (N, H, W, C), R, R, 2, pad, out=B.wr((N, H, W, C), "dx accumulate", init=base),
                               accumulate=True)
    B.check()
    close(dx, ref)
    if accumulate:
        close(dxa, ref + base)
        same_bits(dxa, dx + base.cuda())
