"""The attention launch plan (ds6g_attention_plan: the planner every attention entry point runs, queried without a launch).

Host integer arithmetic only.  Over a grid of shapes, storage kinds, compute modes, debug flags and workspace sizes, every
accepted plan keeps what it writes inside the workspace it was given, keeps its slabs off the hand-over tiles and off each
other, and reduces exactly the outputs it split; the refusals are the entry points' refusals; and the ten cases of
tests/test_chain_launches_gpu.py get the slab-sum counts pinned there.
"""
import ctypes
import itertools

import pytest

from deepsense6g_tii_amd import _lib
from tests.test_chain_launches_gpu import ATTN_SUM_CASES, MERGED_SUM_OFF

# ---- include/ds6g_types.h ------------------------------------------------------------------------------------------------
MAX_STEPS = 8
KIND_F32, KIND_OUT16, KIND_H16 = 0, 1, 2
(FWD, FWD_MERGE, DELTA, DQ_RECOMPUTE, DKV_RECOMPUTE, DKV_HANDOVER, DKV_FUSED128, DK_TWO_PASS, DV_FROM_P, DQ_FROM_DS,
 SLAB_SUM) = range(11)
T_O, T_ML, T_DQ, T_DK, T_DV, T_DELTA, T_HS, T_HP = range(8)
FORM_FWD, FORM_RECOMPUTE, FORM_HANDOVER, FORM_FUSED128, FORM_TWO_PASS = range(5)
REDUCTIONS = (FWD_MERGE, SLAB_SUM)
KERNELS = (FWD, DQ_RECOMPUTE, DKV_RECOMPUTE, DKV_HANDOVER, DKV_FUSED128, DK_TWO_PASS, DV_FROM_P, DQ_FROM_DS)
SLAB_TENSORS = (T_O, T_ML, T_DQ, T_DK, T_DV)      # what a split kernel leaves in slabs for a reduction step


class AttnOut(ctypes.Structure):       # ds6g_attn_out
    _fields_ = [("tensor", ctypes.c_int), ("slabs", ctypes.c_int), ("off", ctypes.c_size_t), ("bytes", ctypes.c_size_t)]


class AttnStep(ctypes.Structure):      # ds6g_attn_step
    _fields_ = [("family", ctypes.c_int), ("splits", ctypes.c_int), ("tiles_per_split", ctypes.c_int), ("nout", ctypes.c_int),
                ("out", AttnOut * 3)]


class AttnPlan(ctypes.Structure):      # ds6g_attn_plan
    _fields_ = [("form", ctypes.c_int), ("merged_sum", ctypes.c_int), ("nsteps", ctypes.c_int), ("slab_sums", ctypes.c_int),
                ("handover_bytes", ctypes.c_size_t), ("steps", AttnStep * MAX_STEPS)]


HANDOVER_OFF, FUSED128_OFF = 0x01000000, 0x04000000        # ds6g_set_debug_flags
KIND_OF = {"f32": KIND_F32, "bf16out": KIND_OUT16, "bf16": KIND_H16, "f16": KIND_H16}    # the names of ATTN_SUM_CASES


def query_plan(backward, kind, B, T, nh, hd, ws_bytes):
    """-> (0, AttnPlan) or (refusal code, None) under the process's current compute mode and debug flags; ld = nh * hd"""
    plan = AttnPlan()
    try:
        _lib.lib().attention_plan(backward, kind, B, T, nh, hd, nh * hd, ws_bytes, ctypes.addressof(plan))
    except _lib.Ds6gError as e:
        return int(str(e).rsplit("code ", 1)[1]), None
    return 0, plan


def test_plan_layout_matches_the_header():
    # {int, int, size_t, size_t}, {int x 4, out[3]}, {int x 4, size_t, steps[8]} on LP64
    assert ctypes.sizeof(AttnOut) == 24 and AttnOut.off.offset == 8 and AttnOut.bytes.offset == 16
    assert ctypes.sizeof(AttnStep) == 88 and AttnStep.nout.offset == 12 and AttnStep.out.offset == 16
    assert ctypes.sizeof(AttnPlan) == 728 and AttnPlan.handover_bytes.offset == 16 and AttnPlan.steps.offset == 24
    types = open(_lib.HEADER.replace("ds6g.h", "ds6g_types.h")).read()
    assert "#define DS6G_ATTN_MAX_STEPS 8" in types and "} ds6g_attn_plan;" in types
    # the enumerators in the order mirrored above
    names = ("DS6G_ATTN_FWD = 0, DS6G_ATTN_FWD_MERGE, DS6G_ATTN_DELTA, DS6G_ATTN_DQ_RECOMPUTE, DS6G_ATTN_DKV_RECOMPUTE, "
             "DS6G_ATTN_DKV_HANDOVER, DS6G_ATTN_DKV_FUSED128, DS6G_ATTN_DK_TWO_PASS, DS6G_ATTN_DV_FROM_P, DS6G_ATTN_DQ_FROM_DS, "
             "DS6G_ATTN_SLAB_SUM",
             "DS6G_ATTN_T_O = 0, DS6G_ATTN_T_ML, DS6G_ATTN_T_DQ, DS6G_ATTN_T_DK, DS6G_ATTN_T_DV, DS6G_ATTN_T_DELTA, DS6G_ATTN_T_HS, "
             "DS6G_ATTN_T_HP, DS6G_ATTN_T_COUNT",
             "DS6G_ATTN_FORM_FWD = 0, DS6G_ATTN_FORM_RECOMPUTE, DS6G_ATTN_FORM_HANDOVER, DS6G_ATTN_FORM_HANDOVER_FUSED128, "
             "DS6G_ATTN_FORM_HANDOVER_TWO_PASS")
    flat = " ".join(types.split())
    for n in names:
        assert n in flat, n
    assert "ds6g_attention_plan" in _lib.parse_header()


# ---- the grid ------------------------------------------------------------------------------------------------------------
SHAPES = list(itertools.product((1, 2, 12), (1, 31, 32, 33, 130, 250, 512, 642, 1922), (1, 4, 8), (16, 32, 64, 128)))


def _sizes(B, T, nh, hd):
    """-> slab, query, hand-over bytes, the workspace sizes of the grid"""
    slab = B * T * nh * hd * 4
    need = int(_lib.lib().attention_workspace_bytes(B, T, nh, hd, nh * hd))
    hand = need - 16 * slab - 64 * B * nh * T
    return slab, need, hand, (0, slab - 4, slab, 2 * slab, hand + 2 * slab - 4, hand + 2 * slab, hand + 3 * slab, need - 4, need,
                              need + 8 * slab, 1 << 30)


def _ranges(step):
    return [(o.tensor, o.slabs, o.off, o.off + o.bytes) for o in step.out[:step.nout]]


def _disjoint(ranges):
    spans = sorted((lo, hi) for _, slabs, lo, hi in ranges if slabs)
    return all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def check_plan(plan, ws_bytes, ctx):
    steps = plan.steps[:plan.nsteps]
    assert 1 <= plan.nsteps <= MAX_STEPS, ctx
    handover = plan.form in (FORM_HANDOVER, FORM_FUSED128, FORM_TWO_PASS)
    assert (plan.handover_bytes > 0) == handover, ctx
    for i, st in enumerate(steps):
        rs = _ranges(st)
        for tensor, slabs, lo, hi in rs:
            if not slabs:
                assert lo == hi == 0, ctx
                continue
            assert lo < hi <= ws_bytes, (ctx, i, "(a) a range ends behind the workspace")
            if handover and tensor in SLAB_TENSORS:
                assert lo >= plan.handover_bytes, (ctx, i, "(b) a slab on the hand-over tiles")
            if tensor in (T_HS, T_HP):
                assert hi <= plan.handover_bytes, (ctx, i, "(b) tiles behind handover_bytes")
        assert _disjoint(rs), (ctx, i, "(c) one step's ranges overlap")     # in the merged sum: dK, dV and dQ slabs
        if st.family in KERNELS:
            assert st.splits >= 1 and st.splits == -(-(-(-ctx[3] // 32)) // st.tiles_per_split), (ctx, i)
            for tensor, slabs, lo, hi in rs:
                if tensor not in SLAB_TENSORS:
                    continue
                assert slabs == (st.splits if st.splits > 1 else 0), (ctx, i)
                later = [s for s in steps[i + 1:] if s.family in REDUCTIONS and (tensor, slabs, lo, hi) in _ranges(s)]
                assert len(later) == (1 if st.splits > 1 else 0), (ctx, i, "(d) split output and reduction do not pair up")
        elif st.family in REDUCTIONS:
            assert st.splits == 0 and st.nout >= 1, (ctx, i)
            for r in rs:                                   # no reduction without the kernel step that wrote its slabs
                assert r[1] > 1 and any(s.family in KERNELS and r in _ranges(s) for s in steps[:i]), (ctx, i, "(d)")
        else:
            assert st.family == DELTA and i == 0 and handover, (ctx, i)
    sums = [s for s in steps if s.family == SLAB_SUM]
    assert plan.slab_sums == len(sums), (ctx, "(d) slab-sum count")
    assert plan.merged_sum == int(any(s.nout == 3 for s in sums)), ctx
    return steps


MODES = [(KIND_F32, 0), (KIND_F32, 1), (KIND_OUT16, 0), (KIND_OUT16, 1), (KIND_H16, 0)]     # kind, ds6g_set_compute_mode


@pytest.mark.parametrize("flags", [a | b | c for a in (0, HANDOVER_OFF) for b in (0, FUSED128_OFF) for c in (0, MERGED_SUM_OFF)],
                         ids=lambda f: f"flags{f >> 24:x}")
@pytest.mark.parametrize("kind,mode", MODES, ids=["f32", "f32-bf16mode", "out16", "out16-bf16mode", "h16"])
def test_every_plan_of_the_grid_is_sound(kind, mode, flags):
    L = _lib.lib()
    L.set_compute_mode(mode)
    L.set_debug_flags(flags)
    try:
        accepted = 0
        for B, T, nh, hd in SHAPES:
            slab, need, hand, sizes = _sizes(B, T, nh, hd)
            assert hand == B * nh * (-(-T // 128) * 4) ** 2 * 4096 * (2 if hd == 128 else 1)
            for ws in sizes:
                ctx = (kind, mode, hex(flags), T, B, nh, hd, ws)
                # the backward, and its refusals
                rc, plan = query_plan(1, kind, B, T, nh, hd, ws)
                want = 0 if kind == KIND_F32 else (3 if ws < need else (1 if flags & HANDOVER_OFF else 0))
                assert rc == want, ctx
                if plan is not None:
                    accepted += 1
                    steps = check_plan(plan, ws, ctx)
                    recompute = bool(flags & HANDOVER_OFF) or ws < hand + 2 * slab
                    assert (plan.form == FORM_RECOMPUTE) == recompute, ctx
                    if not recompute:
                        assert plan.handover_bytes == hand, ctx
                        assert (plan.form == FORM_HANDOVER) == (hd < 128), ctx
                        if hd == 128:          # fused: exact fp32 operands or 16-bit stored ones, and not switched off
                            fused = not flags & FUSED128_OFF and (kind == KIND_H16 or mode == 0)
                            assert (plan.form == FORM_FUSED128) == fused, ctx
                    if flags & MERGED_SUM_OFF or plan.form in (FORM_RECOMPUTE, FORM_TWO_PASS):
                        assert not plan.merged_sum, ctx
                    assert {t for s in steps if s.family in KERNELS for t, *_ in _ranges(s)} >= {T_DQ, T_DK, T_DV}, ctx
                # the forward takes any size
                rc, plan = query_plan(0, kind, B, T, nh, hd, ws)
                assert rc == 0 and plan.form == FORM_FWD and plan.slab_sums == 0, ctx
                steps = check_plan(plan, ws, ctx)
                assert steps[0].family == FWD and plan.nsteps == (2 if steps[0].splits > 1 else 1), ctx
                if steps[0].splits > 1:
                    assert steps[0].splits * (slab + 8 * B * nh * T) <= ws, (ctx, "(e)")
        assert accepted > 0 or kind != KIND_F32
    finally:
        L.set_debug_flags(0)
        L.set_compute_mode(0)


# ---- refusals and forms at the queried size --------------------------------------------------------------------------------
def test_refusals_and_the_forms_at_the_queried_size():
    L = _lib.lib()
    try:
        for B, T, nh, hd in SHAPES:
            _, need, _, _ = _sizes(B, T, nh, hd)
            L.set_debug_flags(0)
            assert query_plan(1, KIND_F32, B, T, nh, hd, 0)[0] == 0                       # fp32 takes any size, none included
            for kind in (KIND_F32, KIND_OUT16, KIND_H16):
                rc, plan = query_plan(1, kind, B, T, nh, hd, need)
                assert rc == 0 and plan.form in (FORM_HANDOVER, FORM_FUSED128, FORM_TWO_PASS), (kind, B, T, nh, hd)
            for kind in (KIND_OUT16, KIND_H16):
                assert query_plan(1, kind, B, T, nh, hd, need - 4)[0] == 3                # DS6G_ERR_WORKSPACE
                L.set_debug_flags(HANDOVER_OFF)
                assert query_plan(1, kind, B, T, nh, hd, need)[0] == 1                    # DS6G_ERR_ARG
                assert query_plan(1, kind, B, T, nh, hd, need - 4)[0] == 3                # the workspace refusal comes first
                L.set_debug_flags(0)
    finally:
        L.set_debug_flags(0)


def test_bad_shapes_are_refused():
    for args in ((0, 33, 2, 64), (1, 0, 2, 64), (1, 33, 0, 64), (1, 33, 2, 48), (1, 33, 2, 0)):
        for backward in (0, 1):
            assert query_plan(backward, KIND_F32, *args, 1 << 20)[0] == 1, args
    assert query_plan(1, 3, 1, 33, 2, 64, 1 << 20)[0] == 1                                # no such kind
    plan = AttnPlan()
    with pytest.raises(_lib.Ds6gError, match="code 1"):
        _lib.lib().attention_plan(1, 0, 1, 33, 2, 64, 130, 1 << 20, ctypes.addressof(plan))   # ld no multiple of 4
    with pytest.raises(_lib.Ds6gError, match="code 1"):
        _lib.lib().attention_plan(1, 0, 1, 33, 2, 64, 128, 1 << 20, 0)                          # no plan to fill


# ---- the pinned launch counts of tests/test_chain_launches_gpu.py ------------------------------------------------------------
@pytest.mark.parametrize("B,T,nh,hd,kind,n_one,n_two", ATTN_SUM_CASES)
def test_the_pinned_slab_sum_counts_at_the_queried_size(B, T, nh, hd, kind, n_one, n_two):
    L = _lib.lib()
    need = int(L.attention_workspace_bytes(B, T, nh, hd, nh * hd))
    try:
        got = []
        for flags in (0, MERGED_SUM_OFF):
            L.set_debug_flags(flags)
            rc, plan = query_plan(1, KIND_OF[kind], B, T, nh, hd, need)
            assert rc == 0
            check_plan(plan, need, (kind, 0, hex(flags), T, B, nh, hd, need))
            got.append(plan.slab_sums)
        assert tuple(got) == (n_one, n_two)
    finally:
        L.set_debug_flags(0)


def _kernels(plan):
    return [(s.family, s.splits, s.tiles_per_split) for s in plan.steps[:plan.nsteps] if s.family in KERNELS]


def test_the_plan_depends_on_the_workspace_beyond_the_queried_size():
    """B = 12, T = 642, fp32: both kernels take 7 splits, and 7 + 7 + 7 slabs do not fit the query's 16 - two slab-sum
    launches at the queried size, one (the merged form) on a 1 GiB scratch; the kernels and their splits are the same"""
    for hd in (16, 32, 64, 128):
        need = int(_lib.lib().attention_workspace_bytes(12, 642, 4, hd, 4 * hd))
        at_query, on_scratch = query_plan(1, KIND_F32, 12, 642, 4, hd, need)[1], query_plan(1, KIND_F32, 12, 642, 4, hd, 1 << 30)[1]
        assert (at_query.slab_sums, at_query.merged_sum) == (2, 0), hd
        assert (on_scratch.slab_sums, on_scratch.merged_sum) == (1, 1), hd
        assert _kernels(at_query) == _kernels(on_scratch) and [k[1] for k in _kernels(at_query)] == [7, 7], hd


# the benchmark's attention backwards: the four GPT stages (4 heads of 16 / 32 / 64 / 128) at B = 12, T = 962 (31 tiles), on
# the model's 1 GiB scratch.  hd -> form, slab-sum launches, merged, (family, splits, tiles per split) of the split kernels
BENCH_PLANS = {
    (KIND_F32, 0): {16: (FORM_HANDOVER, 1, 1, [(DKV_HANDOVER, 2, 16), (DQ_FROM_DS, 2, 16)]),
                    32: (FORM_HANDOVER, 1, 1, [(DKV_HANDOVER, 2, 16), (DQ_FROM_DS, 2, 16)]),
                    64: (FORM_HANDOVER, 1, 1, [(DKV_HANDOVER, 4, 8), (DQ_FROM_DS, 4, 8)]),
                    128: (FORM_FUSED128, 1, 1, [(DKV_FUSED128, 2, 16), (DQ_FROM_DS, 4, 8)])},
    (KIND_H16, 1): {16: (FORM_HANDOVER, 1, 1, [(DKV_HANDOVER, 2, 16), (DQ_FROM_DS, 2, 16)]),      # --dtype bf16
                    32: (FORM_HANDOVER, 1, 1, [(DKV_HANDOVER, 2, 16), (DQ_FROM_DS, 2, 16)]),
                    64: (FORM_HANDOVER, 0, 0, [(DKV_HANDOVER, 1, 31), (DQ_FROM_DS, 1, 31)]),
                    128: (FORM_FUSED128, 1, 0, [(DKV_FUSED128, 2, 16), (DQ_FROM_DS, 1, 31)])},
}


@pytest.mark.parametrize("kind,mode", sorted(BENCH_PLANS), ids=["f32", "bf16"])
def test_the_benchmark_plans_on_the_model_scratch(kind, mode):
    """... where the plan on the model's scratch is also the plan at the queried size"""
    L = _lib.lib()
    L.set_compute_mode(mode)
    try:
        for hd, (form, sums, merged, kernels) in BENCH_PLANS[kind, mode].items():
            need = int(L.attention_workspace_bytes(12, 962, 4, hd, 4 * hd))
            assert need <= 1 << 30
            for ws in (1 << 30, need):
                rc, plan = query_plan(1, kind, 12, 962, 4, hd, ws)
                assert rc == 0
                check_plan(plan, ws, (kind, mode, "0x0", 962, 12, 4, hd, ws))
                assert (plan.form, plan.slab_sums, plan.merged_sum, _kernels(plan)) == (form, sums, merged, kernels), (hd, ws)
    finally:
        L.set_compute_mode(0)
