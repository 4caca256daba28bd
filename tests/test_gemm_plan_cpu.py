"""The conv / linear GEMM launch plan (ds6g_gemm_plan: the planner of csrc/gemm_plan.h that every entry point of igemm.hip and
bgemm.hip runs, queried without a launch).

Host integer arithmetic only.  Over a grid of shapes, ops, flags, workspace sizes, debug flags and compute modes every accepted
plan covers K exactly, keeps its slabs inside the workspace it was clamped to, uses the uniform walk only where its rule holds,
names an instantiation that exists and carries the variant code of its own fields; the refusals are the entry points'
refusals; a restatement of the rules as they stood before the planner existed (two copies, one per file) agrees with it over
the whole grid; and the benchmark's layers get the plans pinned below.
"""
import ctypes
import itertools

import pytest

from deepsense6g_tii_amd import _lib
from tests.test_bench_shapes_gpu import CONV60

# ---- include/ds6g_types.h ------------------------------------------------------------------------------------------------
F32, H16 = 0, 1
CONV_FWD, CONV_DGRAD, CONV_WGRAD, LIN_FWD, LIN_DGRAD, LIN_WGRAD, BIAS_ACT, BNSTATS = range(8)
EPILOGUE, OUT16, ACCUMULATE, DBIAS = 1, 2, 4, 8
FWD, DGRAD, WGRAD = 0, 1, 2
ERR_ARG, ERR_WORKSPACE = 1, 3
LINEAR_OPS = (LIN_FWD, LIN_DGRAD, LIN_WGRAD)
INT_FIELDS = ("family mode operand_mode Mg Ng Kg BM BN bk tile walk epilogue out16 nclass grid_x grid_y grid_z tiles_n splits "
              "k_per_split wg_rows xcd_splits want_colsum reduce variant").split()


class GemmPlan(ctypes.Structure):       # struct ds6g_gemm_plan
    _fields_ = [(n, ctypes.c_int) for n in INT_FIELDS] + [("slab_elems", ctypes.c_size_t), ("ws_bytes_used", ctypes.c_size_t)]


def cdiv(a, b):
    return -(-a // b)


_PLAN = GemmPlan()


def query(family, op, shape, flags, ws_bytes):
    """-> (0, the plan) or (refusal code, None) under the process's current compute mode and debug flags.  The plan object
    is reused by the next query."""
    rc = _lib.lib()._dll.ds6g_gemm_plan(family, op, *shape, flags, ws_bytes, ctypes.addressof(_PLAN))
    return rc, (_PLAN if rc == 0 else None)


def conv(N, HW, C, K, R, stride):
    return (N, HW, HW, C, K, R, R, stride, R // 2)


def linear(M, N, K):
    """y[M][N] = x[M][K] w[N][K]^T as the 1x1 conv of one 1 x M image"""
    return (1, 1, M, K, N, 1, 1, 1, 0)


def test_plan_layout_matches_the_header():
    # 25 ints, padding to 8, two size_t on LP64
    assert ctypes.sizeof(GemmPlan) == 120 and GemmPlan.variant.offset == 96 and GemmPlan.slab_elems.offset == 104
    assert GemmPlan.ws_bytes_used.offset == 112
    types = " ".join(open(_lib.HEADER.replace("ds6g.h", "ds6g_types.h")).read().split())
    body = types[types.index("struct ds6g_gemm_plan {"):]
    body = body[:body.index("};")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == INT_FIELDS + ["slab_elems", "ws_bytes_used"]
    for n in ("DS6G_GEMM_F32 = 0,", "DS6G_GEMM_H16 = 1",
              "DS6G_GEMM_CONV_FWD = 0, DS6G_GEMM_CONV_DGRAD, DS6G_GEMM_CONV_WGRAD, DS6G_GEMM_LINEAR_FWD, DS6G_GEMM_LINEAR_DGRAD, "
              "DS6G_GEMM_LINEAR_WGRAD, DS6G_GEMM_CONV_BIAS_ACT_FWD, DS6G_GEMM_CONV_FWD_BNSTATS",
              "DS6G_GEMM_EPILOGUE = 1, DS6G_GEMM_OUT16 = 2, DS6G_GEMM_ACCUMULATE = 4, DS6G_GEMM_DBIAS = 8"):
        assert n in types, n
    ret, args = _lib.parse_header()["ds6g_gemm_plan"]
    assert ret is ctypes.c_int and args == [ctypes.c_int] * 12 + [ctypes.c_size_t, ctypes.c_void_p]


# ---- the rules as igemm.hip and bgemm.hip stated them before the planner (launch_igemm, pick_tile, fast_walk_ok, run_wgrad,
# bgemm_wgrad_walk, launch_bgemm and the entry points' checks of the commit before), restated -------------------------------
class Knobs:
    """what ds6g_set_debug_flags and ds6g_set_compute_mode leave behind; the environment is at its defaults"""

    def __init__(self, mode, flags, min_blocks=2560):
        self.mode = mode
        self.general = bool(flags & 0x80)
        self.wgrad_tile = 2 if flags & 0x40 else 1
        self.bf16_bk32 = 0 if flags & 0x10000000 else 1
        self.f32_bk32 = 1 if flags & 0x20000000 else (0 if flags & 0x40000000 else 2)
        self.min_blocks = (flags >> 8) & 0xfff or min_blocks


def walk_rows(N, Ho, Wo, bk):
    if Wo % bk == 0 or N * Ho == 1:
        return 0
    if bk % Wo == 0 and Ho % (bk // Wo) == 0:
        return bk // Wo
    return None


def restate(family, op, shape, flags, ws, kn):
    """-> a refusal code, or (BM, BN, bk, walk, wg_rows, splits, k_per_split, xcd_splits, nclass, reduce, Mg, Ng, Kg)"""
    N, H, W, C, K, R, S, st, pad = shape
    h16, lin = family == H16, op in LINEAR_OPS
    mode = FWD if op in (BIAS_ACT, BNSTATS) else op % 3
    if op == BNSTATS and not h16:
        return ERR_ARG
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    if h16:
        ok = {FWD: C % 64 == 0 and K % 8 == 0 and N > 0, DGRAD: K % 64 == 0 and C % 8 == 0 and (st == 1 or (st == 2 and H % 2 == 0
              and W % 2 == 0)), WGRAD: C % 8 == 0 and K % 8 == 0}[mode]
    else:
        ok = C % 4 == 0 and (N > 0 if mode == FWD else K % 4 == 0)
    es = 2 if h16 else 4
    if not ok or max(N * H * W * C, N * Ho * Wo * K, K * R * S * C) * es >= 1 << 31:
        return ERR_ARG
    nclass, wg_rows, splits, xcd, reduce = 0, 0, 1, 0, 0
    if mode == WGRAD:
        Mg, Ng, Kg = K, R * S * C, N * Ho * Wo
        bk = 64 if h16 else 16
        rows = walk_rows(N, Ho, Wo, bk)
        if h16 and rows is None:
            return ERR_ARG
        walk = int(rows is not None and (h16 or not kn.general))
        wg_rows = rows if walk else 0
        if Mg * Ng % 4 or Mg % 4:
            return ERR_ARG
        slab = Mg * Ng + (Mg if flags & DBIAS else 0)
        if h16:
            BM = BN = 128 if Mg >= 128 and Ng >= 128 else 64
            target, min_k, rnd = (512 if N * Ho == 1 else 384), 256, 64
        else:
            BM, BN = (128 if Mg >= 128 and kn.wgrad_tile == 1 else 64), 64
            target, min_k, rnd = (1024 if lin else 2048), 64, 32
        tiles = cdiv(Mg, BM) * cdiv(Ng, BN)
        splits = max(min(cdiv(target, tiles), cdiv(Kg, min_k), ws // (slab * 4)), 1)
        kps = cdiv(cdiv(Kg, splits), rnd) * rnd
        splits = cdiv(Kg, kps)
        if h16:
            pays = ((tiles * splits) % 8 == 0 and Mg * Ng >= 512 * 512) if N * Ho == 1 else tiles <= 24
            xcd = int(splits >= 2 and pays)
        else:
            xcd = int(not lin and splits >= 8 and tiles <= 12)
        reduce = int(not (splits == 1 and not flags & ACCUMULATE and not flags & DBIAS))
        if reduce and splits * slab * 4 > ws:
            return ERR_ARG
    else:
        if mode == FWD:
            Mg, Ng, Kg = N * Ho * Wo, K, R * S * C
        elif not lin and st == 2 and H % 2 == 0 and W % 2 == 0:
            nclass, Mg, Ng, Kg = 4, N * (H // 2) * (W // 2), C, ((R + 1) // 2) * ((S + 1) // 2) * K
        else:
            Mg, Ng, Kg = N * H * W, C, R * S * K
        t128 = cdiv(Mg, 128) * cdiv(Ng, 128)
        if h16:
            BM = BN = 128 if t128 * (nclass or 1) >= 200 and Mg > 64 and Ng > 64 else 64
            bk, walk = 64, 1
            if op == BNSTATS and ws < cdiv(Mg, 64) * 2 * K * 8:
                return ERR_WORKSPACE
        else:
            if Ng > 64 and Mg > 64 and t128 >= kn.min_blocks:
                BM, BN = 128, 128
            elif Mg > 64 and cdiv(Mg, 128) * cdiv(Ng, 64) >= kn.min_blocks:
                BM, BN = 128, 64
            else:
                BM, BN = 64, 64
            kch = C if mode == FWD else K
            walk = int(kch % 16 == 0 and not kn.general)
            wide = kn.bf16_bk32 != 0 if kn.mode else (kn.f32_bk32 == 1 or (kn.f32_bk32 == 2 and not lin and R * S > 1 and
                                                                             cdiv(Mg, 64) * cdiv(Ng, 64) <= 1024))
            bk = 32 if walk and kch % 32 == 0 and wide else 16
        kps = cdiv(Kg, 64 if h16 else 32) * (64 if h16 else 32)
    if Mg * Ng * 4 >= 1 << 31:
        return ERR_ARG
    return BM, BN, bk, walk, wg_rows, splits, kps, xcd, nclass, reduce, Mg, Ng, Kg


# ---- what every accepted plan satisfies -----------------------------------------------------------------------------------
def check_plan(p, family, op, shape, flags, ws, mode):
    N, H, W, C, K, R, S, st, pad = shape
    h16 = family == H16
    rnd = 64 if h16 else 32
    Ho, Wo = (H + 2 * pad - R) // st + 1, (W + 2 * pad - S) // st + 1
    acc, dbias = bool(flags & ACCUMULATE), bool(flags & DBIAS)
    assert p.family == family and p.mode == (FWD if op in (BIAS_ACT, BNSTATS) else op % 3)
    assert p.tiles_n == cdiv(p.Ng, p.BN) and p.grid_x == cdiv(p.Mg, p.BM) * p.tiles_n
    assert p.grid_y == max(p.nclass, 1) and p.grid_z == p.splits >= 1
    assert p.k_per_split % rnd == 0
    assert p.splits * p.k_per_split >= p.Kg > (p.splits - 1) * p.k_per_split          # no uncovered k, no empty split
    if p.mode == WGRAD:
        assert p.reduce == int(not (p.splits == 1 and not acc and not dbias))
        assert p.slab_elems == p.Mg * p.Ng + (p.Mg if dbias else 0) and p.want_colsum == int(dbias)
        assert p.nclass == 0
    else:
        assert p.splits == 1 and p.reduce == 0 and p.slab_elems == p.Mg * p.Ng
        assert (p.wg_rows, p.xcd_splits, p.want_colsum) == (0, 0, 0)
    if p.reduce:
        assert p.ws_bytes_used == p.splits * p.slab_elems * 4 <= ws
    elif op != BNSTATS:
        assert p.ws_bytes_used == 0
    else:
        assert p.ws_bytes_used == cdiv(p.Mg, p.BM) * 2 * K * 8 <= ws
    # the uniform walk only where its rule holds for the planned k-tile
    if p.walk:
        if p.mode == FWD:
            assert C % p.bk == 0
        elif p.mode == DGRAD:
            assert K % p.bk == 0
        else:
            assert walk_rows(N, Ho, Wo, p.bk) == p.wg_rows
    else:
        assert not h16 and p.bk == 16 and p.wg_rows == 0
    assert not (p.bk == 32 and (p.mode == WGRAD or not p.walk))
    # one of the instantiations that exist
    if h16:
        assert (p.BM, p.BN, p.tile) in ((128, 128, 0), (64, 64, 1)) and p.bk == 64 and p.walk == 1 and p.operand_mode == 0
        assert (p.epilogue, p.out16) in ((0, 0), (0, 1), (1, 0), (1, 1)) or (p.epilogue, p.out16, p.mode) == (2, 1, FWD)
        assert (p.epilogue == 2) == (op == BIAS_ACT)
        want = 30200 + p.tile if p.epilogue == 2 else 30000 + 100 * p.out16 + 10 * p.mode + p.tile
    else:
        assert (p.BM, p.BN, p.tile) in ((128, 128, 0), (128, 64, 1), (64, 64, 2)) and p.bk in (16, 32)
        assert p.epilogue in (0, 1) and p.out16 == 0 and p.operand_mode == mode
        want = 10000 * (p.bk == 32) + 1000 * p.epilogue + 100 * p.walk + 10 * p.mode + p.tile
    if p.mode == WGRAD:
        assert (p.epilogue, p.out16) == (0, 0)
    assert p.variant == want


# ---- the grid ------------------------------------------------------------------------------------------------------------
CONVS = [conv(N, HW, C, K, R, st) for N, HW, C, K, R, st in
         itertools.product((1, 2, 60), (1, 7, 8, 16, 30, 64), (4, 8, 64, 72, 128, 512), (4, 8, 64, 72, 128, 512), (1, 3, 7), (1, 2))]
LINEARS = [linear(M, N, K) for M, N, K in itertools.product((1, 24, 130, 11544), (64, 72, 256, 2048), (64, 72, 256, 2048))]
MIN_BLOCKS_384 = 384 << 8
DEBUG_FLAGS = (0, 0x40, 0x80, 0x10000000, 0x20000000, 0x40000000, MIN_BLOCKS_384)
MODES = (0, 1, 2)                        # ds6g_set_compute_mode: f32, bf16, f32x3


def _problems(family):
    """(op, shape, flags, ws_bytes): each op with the flags and workspace sizes that bear on its plan"""
    for shape in CONVS:
        for op in (CONV_FWD, CONV_DGRAD, BIAS_ACT) + ((BNSTATS,) if family == H16 else ()):
            for flags in (0, EPILOGUE) if op == BIAS_ACT else (0,):
                yield op, shape, flags | (OUT16 if family == H16 else 0), 1 << 30
        yield from _wgrads(CONV_WGRAD, shape, (0, ACCUMULATE))
    for shape in LINEARS:
        for op in (LIN_FWD, LIN_DGRAD):
            for flags in (0, EPILOGUE):
                yield op, shape, flags, 0
        yield from _wgrads(LIN_WGRAD, shape, (0, ACCUMULATE, DBIAS, ACCUMULATE | DBIAS))


def _wgrads(op, shape, flag_sets):
    N, H, W, C, K, R, S, st, pad = shape
    for flags in flag_sets:
        slab = (K * R * S * C + (K if flags & DBIAS else 0)) * 4
        for ws in (0, slab - 4, slab, 4 * slab, 256 << 20, 1 << 30):
            yield op, shape, flags, ws


def _sweep(family, mode, dbg):
    L = _lib.lib()
    L.set_compute_mode(mode)
    L.set_debug_flags(dbg)
    kn = Knobs(mode, dbg)
    accepted = refused = 0
    try:
        for op, shape, flags, ws in _problems(family):
            rc, p = query(family, op, shape, flags, ws)
            want = restate(family, op, shape, flags, ws, kn)
            if p is None:
                assert want == rc, (family, op, shape, flags, ws, rc, want)
                refused += 1
                continue
            try:
                check_plan(p, family, op, shape, flags, ws, mode)
                assert want == (p.BM, p.BN, p.bk, p.walk, p.wg_rows, p.splits, p.k_per_split, p.xcd_splits, p.nclass, p.reduce,
                                p.Mg, p.Ng, p.Kg), want
            except AssertionError as e:
                raise AssertionError((family, op, shape, flags, ws, {n: getattr(p, n) for n in INT_FIELDS})) from e
            accepted += 1
    finally:
        L.set_debug_flags(2560 << 8)     # the min_blocks override is sticky: back to the default
        L.set_debug_flags(0)
        L.set_compute_mode(0)
    assert accepted > 1000 and refused > 1000


@pytest.mark.parametrize("dbg", DEBUG_FLAGS, ids=lambda f: f"flags{f:x}")
@pytest.mark.parametrize("mode", MODES, ids=["f32", "bf16", "f32x3"])
def test_every_fp32_storage_plan_of_the_grid_is_sound_and_is_the_old_rule(mode, dbg):
    _sweep(F32, mode, dbg)


@pytest.mark.parametrize("mode,dbg", [(0, 0), (1, 0x80 | 0x40 | 0x20000000 | MIN_BLOCKS_384)], ids=["default", "every-knob"])
def test_every_16bit_storage_plan_of_the_grid_is_sound_and_is_the_old_rule(mode, dbg):
    """... and reads neither the compute mode nor a debug flag: the restatement is the same under both"""
    _sweep(H16, mode, dbg)


def test_the_16bit_family_never_plans_the_general_walk_or_a_tile_it_has_not():
    _lib.lib().set_debug_flags(0x80)
    try:
        for shape in CONVS[::7]:
            for op in (CONV_FWD, CONV_DGRAD, CONV_WGRAD):
                rc, p = query(H16, op, shape, 0, 1 << 30)
                assert p is None or (p.walk == 1 and p.BM == p.BN), shape
    finally:
        _lib.lib().set_debug_flags(0)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_are_the_entry_points():
    c = conv(2, 8, 64, 64, 3, 1)
    slab = 64 * 9 * 64 * 4
    for family in (F32, H16):
        # a needed reduction without its slabs; a direct launch needs none
        assert query(family, CONV_WGRAD, c, ACCUMULATE, 0)[0] == ERR_ARG
        assert query(family, CONV_WGRAD, c, ACCUMULATE, slab - 4)[0] == ERR_ARG
        assert query(family, LIN_WGRAD, linear(130, 64, 64), DBIAS, 0)[0] == ERR_ARG
        rc, p = query(family, CONV_WGRAD, c, 0, 0)
        assert rc == 0 and (p.splits, p.reduce, p.ws_bytes_used) == (1, 0, 0)
        rc, p = query(family, CONV_WGRAD, c, ACCUMULATE, slab)
        assert rc == 0 and (p.splits, p.reduce, p.ws_bytes_used) == (1, 1, slab)
        # the size limits: a tensor, or an fp32 output, of 2 GiB
        es = 2 if family == H16 else 4
        big = (64 * 4 // es, 128, 128, 512, 64, 1, 1, 1, 0)                  # x is 2^31 bytes
        for op in (CONV_FWD, CONV_DGRAD, CONV_WGRAD):
            assert query(family, op, big, 0, 1 << 30)[0] == ERR_ARG
        assert query(family, CONV_FWD, (big[0] - 1,) + big[1:], 0, 1 << 30)[0] == 0
        # no such family / op; a linear that is not the 1 x M image; no plan to fill
        assert query(2, CONV_FWD, c, 0, 0)[0] == ERR_ARG and query(family, 8, c, 0, 0)[0] == ERR_ARG
        assert query(family, LIN_FWD, c, 0, 0)[0] == ERR_ARG
        assert _lib.lib()._dll.ds6g_gemm_plan(family, CONV_FWD, *c, 0, 0, 0) == ERR_ARG
    assert query(H16, CONV_FWD, (64, 128, 128, 64, 512, 1, 1, 1, 0), 0, 0)[0] == ERR_ARG      # y fits in 16 bits, not as fp32 tiles
    assert query(F32, BNSTATS, c, 0, 1 << 30)[0] == ERR_ARG
    # fp32 storage: multiples of 4; the stem's 4 channels pass, with the general walk
    assert query(F32, CONV_FWD, conv(1, 16, 6, 64, 7, 2), 0, 0)[0] == ERR_ARG
    assert query(F32, CONV_DGRAD, conv(1, 16, 64, 6, 3, 1), 0, 0)[0] == ERR_ARG
    rc, p = query(F32, CONV_FWD, conv(1, 16, 4, 64, 7, 2), 0, 0)
    assert rc == 0 and (p.walk, p.bk, p.variant) == (0, 16, 2)
    # 16-bit storage: 64 on the k side, 8 on the other; stride-2 dgrad needs even H and W; a wgrad needs its walk
    assert query(H16, CONV_FWD, conv(2, 8, 72, 64, 3, 1), 0, 0)[0] == ERR_ARG
    assert query(H16, CONV_FWD, conv(2, 8, 64, 4, 3, 1), 0, 0)[0] == ERR_ARG
    assert query(H16, CONV_DGRAD, conv(2, 8, 64, 72, 3, 1), 0, 0)[0] == ERR_ARG
    assert query(H16, CONV_DGRAD, conv(2, 8, 8, 64, 3, 1), 0, 0)[0] == 0
    assert query(H16, CONV_DGRAD, conv(2, 7, 64, 64, 3, 2), 0, 0)[0] == ERR_ARG
    assert query(F32, CONV_DGRAD, conv(2, 7, 64, 64, 3, 2), 0, 0)[0] == 0                    # fp32: one class, general rows
    assert query(H16, CONV_DGRAD, (2, 8, 8, 64, 64, 3, 3, 3, 1), 0, 0)[0] == ERR_ARG
    assert query(H16, CONV_WGRAD, conv(2, 30, 64, 64, 3, 1), 0, 1 << 30)[0] == ERR_ARG       # Wo = 30: no uniform walk
    rc, p = query(F32, CONV_WGRAD, conv(2, 30, 64, 64, 3, 1), 0, 1 << 30)
    assert rc == 0 and p.walk == 0
    rc, p = query(H16, CONV_WGRAD, conv(2, 8, 64, 64, 3, 1), 0, 1 << 30)
    assert rc == 0 and p.wg_rows == 8
    # the BatchNorm partials of conv2d_fwd_bnstats: 64-row tiles, whatever tile runs
    need = cdiv(2 * 8 * 8, 64) * 2 * 64 * 8
    assert query(H16, BNSTATS, c, 0, need - 8)[0] == ERR_WORKSPACE
    rc, p = query(H16, BNSTATS, c, 0, need)
    assert rc == 0 and (p.out16, p.epilogue, p.variant, p.ws_bytes_used) == (1, 0, 30101, need)
    assert query(H16, BNSTATS, conv(2, 8, 72, 64, 3, 1), 0, 0)[0] == ERR_ARG                  # the shape refusal comes first


# ---- the benchmark's layers: N = 60 images (12 samples x 5 frames), M = 12 x 962 token rows ---------------------------------
M_TOK = 11544
# op, shape, flags -> (BM, BN, splits, k_per_split, xcd_splits) in fp32 storage, in 16-bit storage
BENCH_WGRADS = [
    (CONV_WGRAD, conv(60, 64, 64, 64, 3, 1), 0, (64, 64, 226, 1088, 1), (64, 64, 43, 5760, 1)),
    (CONV_WGRAD, conv(60, 32, 128, 128, 3, 1), 0, (128, 64, 113, 544, 0), (128, 128, 42, 1472, 1)),
    (CONV_WGRAD, conv(60, 16, 256, 256, 3, 1), 0, (128, 64, 29, 544, 0), (128, 128, 11, 1408, 0)),
    (CONV_WGRAD, conv(60, 8, 512, 512, 3, 1), 0, (128, 64, 8, 480, 0), (128, 128, 3, 1280, 0)),
    (LIN_WGRAD, linear(M_TOK, 2048, 512), DBIAS, (128, 64, 8, 1472, 0), (128, 128, 8, 1472, 1)),
    (LIN_WGRAD, linear(M_TOK, 512, 512), DBIAS, (128, 64, 31, 384, 0), (128, 128, 31, 384, 1)),
    (LIN_WGRAD, linear(M_TOK, 256, 64), DBIAS, (128, 64, 181, 64, 0), (64, 64, 46, 256, 0)),
]


def test_the_benchmark_weight_gradients_are_pinned_and_the_same_on_both_model_workspaces():
    for op, shape, flags, *want in BENCH_WGRADS:
        for family in (F32, H16):
            for ws in (256 << 20, 1 << 30):                   # the model's side and main workspace
                rc, p = query(family, op, shape, flags, ws)
                assert rc == 0
                check_plan(p, family, op, shape, flags, ws, 0)
                assert (p.BM, p.BN, p.splits, p.k_per_split, p.xcd_splits) == want[family], (op, shape, family, ws)
            slab = (shape[4] * shape[5] * shape[6] * shape[3] + (shape[4] if flags & DBIAS else 0)) * 4
            rc, p = query(family, op, shape, flags, 4 * slab)
            only3 = family == H16 and shape == conv(60, 8, 512, 512, 3, 1)      # 144 tiles: the target of 384 asks for 3 only
            assert rc == 0 and p.splits == (3 if only3 else 4) and p.ws_bytes_used == p.splits * slab, (op, shape, family)


def test_the_benchmark_forward_tiles_are_pinned():
    convs = [conv(60, 64, 64, 64, 3, 1), conv(60, 32, 128, 128, 3, 1), conv(60, 16, 256, 256, 3, 1), conv(60, 8, 512, 512, 3, 1)]
    fc, fc1 = linear(M_TOK, 512, 512), linear(M_TOK, 2048, 512)
    tile = lambda family, op, shape: (lambda p: (p.BM, p.BN))(query(family, op, shape, 0, 0)[1])
    assert [tile(F32, CONV_FWD, s) for s in convs] == [(64, 64)] * 4
    assert tile(F32, LIN_FWD, fc) == (64, 64) and tile(F32, LIN_FWD, fc1) == (128, 64)
    assert [tile(H16, CONV_FWD, s) for s in convs] == [(64, 64), (128, 128), (128, 128), (64, 64)]
    assert tile(H16, LIN_FWD, fc) == (128, 128) and tile(H16, LIN_FWD, fc1) == (128, 128)


def test_every_conv_and_linear_call_of_a_benchmark_step_plans_soundly():
    """the trunks' conv layers (tests/test_bench_shapes_gpu.py) and the linears of the four GPT stages, forward and backward,
    on the model's 1 GiB workspace, in both families and all three modes"""
    shapes = [(CONV_FWD, (N, H, W, C, K, R, R, st, pad)) for N, H, W, C, K, R, st, pad in CONV60]
    for C in (64, 128, 256, 512):
        shapes += [(LIN_FWD, linear(M_TOK, n, k)) for n, k in ((3 * C, C), (C, C), (4 * C, C), (C, 4 * C))]
    L = _lib.lib()
    try:
        for mode in MODES:
            L.set_compute_mode(mode)
            for family in (F32, H16):
                for op0, shape in shapes:
                    for op, flags in ((op0, 0), (op0, EPILOGUE), (op0 + 1, ACCUMULATE), (op0 + 2, ACCUMULATE | (DBIAS if op0 else 0))):
                        if family == H16 and shape[3] == 4:
                            assert query(family, op, shape, flags, 1 << 30)[0] == ERR_ARG       # the stems keep fp32 storage
                            continue
                        rc, p = query(family, op, shape, flags | (OUT16 if family == H16 else 0), 1 << 30)
                        assert rc == 0, (family, op, shape)
                        check_plan(p, family, op, shape, flags, 1 << 30, mode)
                        assert p.walk == (shape[3] != 4 or op % 3 != FWD), (family, op, shape)    # only the stem's forward walks generally
    finally:
        L.set_compute_mode(0)
