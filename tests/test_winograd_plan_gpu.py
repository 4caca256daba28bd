"""What ran is what was planned: one Winograd call per case, every pointer inside the moats of tests/moat.py, bracketed by
ds6g_profile_begin / _end.  The single profile record carries the variant and the flops of ds6g_winograd_plan's plan for that
call on this device's CU count, the guards are intact, and the result matches torch in fp64 at the tolerance of the op's own
test (tests/test_ops_gpu.py test_winograd_conv3x3, test_winograd_bias_act, test_winograd_wgrad3x3: 2e-5 of the largest value).
Each case asserts the branch it is there for from the plan; where this device's CU count makes the first candidate miss it,
the next candidate that reaches it runs."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import moat
from tests.test_moat_gpu import IO, WS, I, O, Run, _gen, _lib, _ops, rnd
from tests.test_ops_gpu import close
from tests.test_winograd_plan_cpu import BIAS_ACT, FWD, K_FWD1, K_PC, K_WGRAD, WGRAD, query

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def pick(op, candidates, n_cu, branch, ws_bytes=0, accumulate=0):
    """-> (shape, plan) of the first candidate whose plan on this device takes the branch"""
    for shape in candidates:
        rc, p = query(op, shape, accumulate, n_cu, ws_bytes)
        if rc == 0 and branch(p):
            return shape, p
    raise AssertionError(f"no candidate reaches the branch on {n_cu} CUs: {candidates}")


def planned(name, args, plan, ws_bytes=0):
    """runs entry point `name` once with moated arguments (and a moated workspace of exactly ws_bytes for the WS pair) inside a
    profile bracket; the one record is the plan's -> the outputs in argument order"""
    L = _lib()
    ws = moat.moat_workspace(_ops(), max(ws_bytes, 4), 0xFF) if any(a is WS for a in args) else None
    r = Run(args, True, ws, ws_bytes=ws_bytes)
    L.profile_begin(8)
    try:
        r.call(getattr(L, name))
    finally:
        variants, fl, ms = (ctypes.c_int * 8)(), (ctypes.c_double * 8)(), (ctypes.c_float * 8)()
        n = L.profile_end(variants, fl, ms, 8)
    assert n == 1 and variants[0] == plan["variant"] and fl[0] == plan["flops"], (name, n, list(variants[:n]), list(fl[:n]), plan)
    r.check_guards()
    for out in r.outs:
        assert not bool(torch.isnan(out).any()), (name, "NaN in an output")
    return r.outs


def conv_case(shape, seed):
    """x [N][H][W][C], w [K][3][3][C], dy [N][H][W][K] on the device; y, dx, dw of the 3x3 / stride 1 / pad 1 conv in fp64, NHWC / OHWI"""
    N, H, W, C, K = shape
    g = _gen("wino-plan", seed, *shape)
    x, w, dy = rnd(g, N, H, W, C), rnd(g, K, 3, 3, C, scale=1 / (3 * C ** 0.5)), rnd(g, N, H, W, K)
    xd = x.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    wd = w.double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.conv2d(xd, wd, None, 1, 1)
    y.backward(dy.double().cpu().permute(0, 3, 1, 2))
    return x, w, dy, y.detach().permute(0, 2, 3, 1), xd.grad.permute(0, 2, 3, 1), wd.grad.permute(0, 2, 3, 1)


def run_fwd(shape, plan):
    N, H, W, C, K = shape
    x, w, _, y_ref, _, _ = conv_case(shape, "fwd")
    u = _ops().winograd_weights(w.data_ptr(), K, C, x.device)
    (y,) = planned("conv3x3_winograd_fwd", [I(x, (W + 1) * C), I(u), O(N, H, W, K), N, H, W, C, K, 0], plan)
    close(y, y_ref, 2e-5, 2e-5)


# ---- the conv forms ---------------------------------------------------------------------------------------------------------
def test_the_32_channel_kernel_runs_its_plan(dev, n_cu):
    shape, p = pick(FWD, [(2, 8, 16, 32, 32)], n_cu, lambda p: p["kernel"] == K_FWD1)
    assert (p["variant"], p["grid_x"], p["block"]) == (20000, 2, 256)
    run_fwd(shape, p)


def test_a_single_item_runs_its_plan(dev, n_cu):
    shape, p = pick(FWD, [(2, 8, 8, 64, 64)], n_cu, lambda p: p["kernel"] == K_PC and p["items"] == 1)
    assert (p["grid_x"], p["rounds"], p["xcd"], p["variant"]) == (1, 1, 0, 20002)
    run_fwd(shape, p)


def test_a_ragged_last_round_runs_in_plain_item_order(dev, n_cu):
    ragged = lambda p: p["kernel"] == K_PC and p["rounds"] >= 2 and p["items"] % p["grid_x"] != 0 and p["xcd"] == 0
    shape, p = pick(FWD, [(N, 8, 8, 32, 512) for N in (66, 34, 130, 18, 10, 258, 6)], n_cu, ragged)
    run_fwd(shape, p)


def test_two_full_rounds_run_in_xcd_item_order(dev, n_cu):
    full = lambda p: p["kernel"] == K_PC and p["rounds"] == 2 and p["items"] == 2 * p["grid_x"] and p["xcd"] >= 1
    # 32 N tile blocks of one channel block each: N = CUs / 16 gives two rounds of one item per CU
    shape, p = pick(FWD, [(16, 64, 64, 32, 64), (max(n_cu // 16, 1), 64, 64, 32, 64), (max(n_cu // 8, 1), 32, 64, 32, 64)], n_cu, full)
    assert p["grid_x"] % 8 == 0
    run_fwd(shape, p)


def test_channel_block_groups_of_xcds_run_their_plan(dev, n_cu):
    shape, p = pick(FWD, [(4, 8, 8, 512, 512), (8, 8, 8, 512, 512), (16, 8, 8, 512, 512)], n_cu, lambda p: p["xcd"] > 1)
    run_fwd(shape, p)


def test_the_accumulating_data_gradient_runs_its_plan(dev, n_cu):
    N, H, W, C, K = 3, 6, 16, 64, 128                  # the data gradient: the same entry point on dy and the dgrad filter, C outputs
    x, w, dy, _, dx_ref, _ = conv_case((N, H, W, C, K), "dgrad")
    shape, p = pick(FWD, [(N, H, W, K, C)], n_cu, lambda p: p["kernel"] == K_PC and p["TH"] == 3, accumulate=1)
    ud = _ops().winograd_weights(w.data_ptr(), K, C, dev, dgrad=True)
    base = rnd(_gen("wino-plan-base"), N, H, W, C)
    (dx,) = planned("conv3x3_winograd_fwd", [I(dy, (W + 1) * K), I(ud), IO(base), N, H, W, K, C, 1], p)
    close(dx.double().cpu() - base.double().cpu(), dx_ref, 2e-5, 2e-5)


def test_the_inference_form_with_a_residual_runs_its_plan(dev, n_cu):
    N, H, W, C, K = 3, 10, 16, 64, 128
    x, w, _, y_ref, _, _ = conv_case((N, H, W, C, K), "bias-act")
    shape, p = pick(BIAS_ACT, [(N, H, W, C, K)], n_cu, lambda p: p["kernel"] == K_PC)
    g = _gen("wino-plan-bias")
    bias, res = rnd(g, K), rnd(g, N, H, W, K)
    u = _ops().winograd_weights(w.data_ptr(), K, C, dev)
    (y,) = planned("conv3x3_winograd_bias_act_fwd", [I(x, (W + 1) * C), I(u), I(bias), I(res), O(N, H, W, K), N, H, W, C, K, 2], p)
    close(y, torch.relu(y_ref + bias.double().cpu() + res.double().cpu()), 2e-5, 2e-5)


# ---- the weight gradient ----------------------------------------------------------------------------------------------------
SLAB = 16 * 64 * 64 * 4
WGRADS = [("one split", (2, 8, 16, 64, 64), 16 * SLAB, (1, 64)),
          ("two splits, a ragged last split and a partial last chunk", (1, 40, 42, 64, 64), 16 * SLAB, (2, 224)),
          ("four exact splits", (12, 16, 16, 64, 64), 16 * SLAB, (4, 192)),
          ("the workspace clamped to one slab", (12, 16, 16, 64, 64), SLAB, (1, 768))]


@pytest.mark.parametrize("what,shape,ws_bytes,want", WGRADS, ids=[w[0].split(",")[0].replace(" ", "-") for w in WGRADS])
def test_the_weight_gradient_runs_its_plan(dev, n_cu, what, shape, ws_bytes, want):
    N, H, W, C, K = shape
    shape, p = pick(WGRAD, [shape], n_cu, lambda p: (p["splits"], p["tiles_per_split"]) == want, ws_bytes=ws_bytes)
    assert p["kernel"] == K_WGRAD and p["ws_bytes_used"] == want[0] * SLAB <= ws_bytes and p["grid_z"] == want[0]
    assert (p["tiles_total"] % p["tiles_per_split"] != 0, p["tiles_total"] % 16 != 0) == (what.startswith("two"),) * 2
    x, _, dy, _, _, dw_ref = conv_case(shape, "wgrad")
    sh = (W + 1) * max(C, K)
    (dw,) = planned("conv3x3_winograd_wgrad", [I(x, sh), I(dy, sh), O(K, 3, 3, C), N, H, W, C, K, 0, WS], p, ws_bytes)
    close(dw, dw_ref, 2e-5, 2e-5)
