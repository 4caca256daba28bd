"""The Winograd launch plan (ds6g_winograd_plan: the planner of csrc/wino_plan.h that every entry point of winograd.hip runs,
queried without a launch and, with a CU count given, without a HIP call).

Host integer arithmetic only.  Over a grid of shapes, CU counts, workspace sizes and both accumulate values a restatement of
the rules as winograd.hip stated them before the planner existed agrees with it field by field, refusals included; every
accepted plan keeps the invariants the kernels rely on (rounds and grid of the persistent kernel, the conditions and the cost
minimum of its XCD item order, exact division constants, covering non-empty wgrad splits inside the workspace); the
benchmark's layers get the plans pinned below; and each environment knob, read once per process and therefore set in a child
process of its own, changes the fields it should and nothing else.
"""
import ctypes
import itertools
import json
import os
import re
import subprocess
import sys

import pytest

from deepsense6g_tii_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- include/ds6g_types.h ------------------------------------------------------------------------------------------------
FWD, BIAS_ACT, WGRAD = 0, 1, 2
K_FWD1, K_FWD2, K_PC, K_WGRAD = 0, 1, 2, 3
ERR_ARG, ERR_LAUNCH, ERR_WORKSPACE = 1, 2, 3
INT_FIELDS = ("op kernel TH TW BTW BTH rows_total row_blocks col_blocks items rounds grid_x grid_y grid_z block lds_bytes xcd "
              "btw_shift").split()
UINT_FIELDS = "th_magic x_bytes u_bytes dy_bytes".split()
INT_FIELDS2 = "tiles_total splits tiles_per_split variant".split()
FIELDS = INT_FIELDS + UINT_FIELDS + INT_FIELDS2 + ["flops", "ws_bytes_used"]
PC_LDS_BYTES = 128 << 10
MIB256 = 256 << 20


class WinoPlan(ctypes.Structure):       # struct ds6g_wino_plan
    _fields_ = ([(n, ctypes.c_int) for n in INT_FIELDS] + [(n, ctypes.c_uint) for n in UINT_FIELDS] +
                [(n, ctypes.c_int) for n in INT_FIELDS2] + [("flops", ctypes.c_double), ("ws_bytes_used", ctypes.c_size_t)])


def cdiv(a, b):
    return -(-a // b)


_PLAN = WinoPlan()


def query(op, shape, accumulate=0, n_cu=256, ws_bytes=0):
    """-> (0, the plan's fields as a dict) or (refusal code, None) under the process's debug flags and environment"""
    rc = _lib.lib()._dll.ds6g_winograd_plan(op, *shape, accumulate, n_cu, ws_bytes, ctypes.addressof(_PLAN))
    return rc, ({n: getattr(_PLAN, n) for n in FIELDS} if rc == 0 else None)


def test_plan_layout_matches_the_header():
    # 18 ints, 4 unsigned, 4 ints = 104 bytes, a double, a size_t on LP64
    assert ctypes.sizeof(WinoPlan) == 120 and WinoPlan.th_magic.offset == 72 and WinoPlan.variant.offset == 100
    assert WinoPlan.flops.offset == 104 and WinoPlan.ws_bytes_used.offset == 112
    types = " ".join(open(_lib.HEADER.replace("ds6g.h", "ds6g_types.h")).read().split())
    body = types[types.index("struct ds6g_wino_plan {"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("};")])
    assert re.findall(r"(\w+)\s*[,;]", body) == FIELDS
    for n in ("DS6G_WINO_FWD = 0,", "DS6G_WINO_BIAS_ACT = 1,", "DS6G_WINO_WGRAD = 2 }", "DS6G_WINO_K_FWD1 = 0,", "DS6G_WINO_K_FWD2 = 1,",
              "DS6G_WINO_K_PC = 2,", "DS6G_WINO_K_WGRAD = 3 }"):
        assert n in types, n
    ret, args = _lib.parse_header()["ds6g_winograd_plan"]
    assert ret is ctypes.c_int and args == [ctypes.c_int] * 8 + [ctypes.c_size_t, ctypes.c_void_p]


# ---- the rules as winograd.hip stated them before the planner (ds6g_winograd_supported, wino_fwd_launch,
# ds6g_winograd_wgrad_supported and ds6g_conv3x3_winograd_wgrad of the commit before), restated ----------------------------
class Knobs:
    """the environment's defaults and the 0x02000000 debug flag"""

    def __init__(self, pc=1, reserve=0, pc_xcd=-1, ww_xcd=1, kb64=0):
        self.pc, self.reserve, self.pc_xcd, self.ww_xcd, self.kb64 = pc, reserve, pc_xcd, ww_xcd, kb64


def fwd_supported(N, H, W, C, K):
    if H % 2 or W % 2 or C % 16 or K % 32 or N <= 0:
        return False
    TW = W // 2
    if (TW % 8 != 0) if TW >= 8 else (32 % TW != 0):
        return False
    return N * H * W * C * 4 < 0x80000000 and 16 * K * C * 4 < 0x80000000


def wgrad_supported(N, H, W, C, K):
    if H % 2 or W % 2 or C % 64 or K % 64 or N <= 0:
        return False
    return N * H * W * C * 4 + (W + 1) * C * 4 < 0x40000000 and N * H * W * K * 4 < 0x80000000


def restate(op, shape, n_cu, ws, kn):
    """-> a refusal code, or every field of the plan"""
    N, H, W, C, K = shape
    p = dict.fromkeys(FIELDS, 0)
    p.update(op=op, TH=H // 2, TW=W // 2, x_bytes=N * H * W * C * 4, flops=2.0 * N * H * W * K * 9.0 * C, grid_y=1, grid_z=1, block=256)
    if op == WGRAD:
        if not wgrad_supported(*shape):
            return ERR_ARG
        slab = 16 * K * C * 4
        if ws < slab:
            return ERR_WORKSPACE
        tiles = N * p["TH"] * p["TW"]
        base = (K // 64) * (C // 64) * 4
        chunks = cdiv(tiles, 16)
        splits = max(min(cdiv(1024, base), chunks // 12, ws // slab), 1)
        cps = cdiv(chunks, splits)
        splits = cdiv(chunks, cps)
        p.update(kernel=K_WGRAD, variant=20001, dy_bytes=N * H * W * K * 4, tiles_total=tiles, tiles_per_split=cps * 16, splits=splits,
                 grid_x=(K // 64) * (C // 64), grid_y=4, grid_z=splits, xcd=kn.ww_xcd, ws_bytes_used=splits * slab)
        return p
    if not fwd_supported(*shape):
        return ERR_ARG
    BTW = 8 if p["TW"] >= 8 else p["TW"]
    BTH = 32 // BTW
    rows_total = N * p["TH"]
    row_blocks, col_blocks = cdiv(rows_total, BTH), p["TW"] // BTW
    p.update(BTW=BTW, BTH=BTH, rows_total=rows_total, row_blocks=row_blocks, col_blocks=col_blocks, u_bytes=16 * K * C * 4, variant=20000)
    use_pc = kn.pc and K % 64 == 0 and C >= 32 and N * H * W * C * 4 + (W + 1) * C * 4 < 0x40000000
    if not use_pc:
        kb64 = K % 64 == 0 and kn.kb64
        p.update(kernel=K_FWD2 if kb64 else K_FWD1, grid_x=row_blocks * col_blocks * (K // (64 if kb64 else 32)))
        return p
    if n_cu <= 0:
        return ERR_LAUNCH
    kblocks = K // 64
    items = row_blocks * col_blocks * kblocks
    cus = max(n_cu - kn.reserve, 1)
    rounds = cdiv(items, cus)
    grid = cdiv(items, rounds)
    gk_best = 0
    if kn.pc_xcd != 0 and grid % 8 == 0 and items % grid == 0:
        ntb = items // kblocks
        best = 0
        for gk in (1, 2, 4, 8):
            gt = 8 // gk
            if kblocks % gk or ntb % gt or (kn.pc_xcd > 0 and gk != kn.pc_xcd):
                continue
            cost = p["u_bytes"] * gt + p["x_bytes"] * gk
            if not gk_best or cost < best:
                best, gk_best = cost, gk
    # th_magic keeps the (unsigned) cast: 0 for TH = 1, which the kernel never multiplies by
    p.update(kernel=K_PC, variant=20002, block=512, lds_bytes=PC_LDS_BYTES, items=items, rounds=rounds, grid_x=grid, xcd=gk_best,
             btw_shift=BTW.bit_length() - 1, th_magic=((1 << 32) + p["TH"] - 1) // p["TH"] & 0xffffffff)
    return p


# ---- what every accepted plan satisfies -----------------------------------------------------------------------------------
_DIV_CHECKED = {}     # TH -> rows whose division by multiplication has been checked


def check_plan(p, op, shape, n_cu, ws, kn):
    N, H, W, C, K = shape
    assert p["op"] == op and (p["TH"], p["TW"]) == (H // 2, W // 2) and p["flops"] == 2.0 * N * H * W * K * 9 * C
    if op == WGRAD:
        slab = 16 * K * C * 4
        assert p["kernel"] == K_WGRAD and p["variant"] == 20001 and p["tiles_total"] == N * (H // 2) * (W // 2)
        assert p["tiles_per_split"] > 0 and p["tiles_per_split"] % 16 == 0
        assert p["splits"] * p["tiles_per_split"] >= p["tiles_total"] > (p["splits"] - 1) * p["tiles_per_split"]    # no empty split
        assert p["ws_bytes_used"] == p["splits"] * slab <= ws
        assert (p["grid_x"], p["grid_y"], p["grid_z"], p["block"], p["lds_bytes"]) == ((K // 64) * (C // 64), 4, p["splits"], 256, 0)
        return
    assert p["BTW"] * p["BTH"] == 32 and p["TW"] % p["BTW"] == 0 and p["col_blocks"] * p["BTW"] == p["TW"]
    assert p["rows_total"] == N * p["TH"] and p["row_blocks"] == cdiv(p["rows_total"], p["BTH"])
    assert (p["grid_y"], p["grid_z"]) == (1, 1) and (p["splits"], p["tiles_per_split"], p["ws_bytes_used"]) == (0, 0, 0)
    blocks = p["row_blocks"] * p["col_blocks"]
    if p["kernel"] != K_PC:
        per = 64 if p["kernel"] == K_FWD2 else 32
        assert K % per == 0 and p["grid_x"] == blocks * (K // per) and (p["block"], p["lds_bytes"], p["variant"]) == (256, 0, 20000)
        assert (p["items"], p["rounds"], p["xcd"]) == (0, 0, 0)
        return
    kblocks = K // 64
    assert K % 64 == 0 and C >= 32 and p["variant"] == 20002 and (p["block"], p["lds_bytes"]) == (512, PC_LDS_BYTES)
    assert p["items"] == blocks * kblocks
    assert p["rounds"] == cdiv(p["items"], max(n_cu - kn.reserve, 1))
    assert p["grid_x"] == cdiv(p["items"], p["rounds"]) <= n_cu
    grid, items, gk = p["grid_x"], p["items"], p["xcd"]

    def allowed(g):
        return grid % 8 == 0 and items % grid == 0 and kblocks % g == 0 and (items // kblocks) % (8 // g) == 0

    def cost(g):
        return p["u_bytes"] * (8 // g) + p["x_bytes"] * g

    if gk:
        assert gk in (1, 2, 4, 8) and allowed(gk)
        if kn.pc_xcd < 0:
            assert all(cost(g) >= cost(gk) for g in (1, 2, 4, 8) if allowed(g))
    elif kn.pc_xcd < 0:
        assert not any(allowed(g) for g in (1, 2, 4, 8))
    # the kernel's / BTW, % BTW and / TH: tile 0 .. 31 of a block, tile rows 0 .. row_blocks * BTH - 1
    assert all(t >> p["btw_shift"] == t // p["BTW"] and t & (p["BTW"] - 1) == t % p["BTW"] for t in range(32))
    TH, rows = p["TH"], p["row_blocks"] * p["BTH"]
    assert p["th_magic"] == cdiv(1 << 32, TH) & 0xffffffff and rows * TH < 1 << 32
    for r in range(_DIV_CHECKED.get(TH, 0), rows):
        assert TH == 1 or (r * p["th_magic"]) >> 32 == r // TH, (TH, r)
    _DIV_CHECKED[TH] = max(_DIV_CHECKED.get(TH, 0), rows)


# ---- the grid ------------------------------------------------------------------------------------------------------------
NS = (1, 2, 5, 12, 60, 66)
HS = (2, 4, 6, 8, 16, 40, 64)
WS_ = (2, 4, 6, 8, 10, 12, 16, 24, 32, 42, 64)     # TW 1 2 3 (refused) 4 5 6 (refused) 8 12 (refused) 16 21 (refused) 32
CS = (16, 32, 48, 64, 128, 256, 512)
KS = (16, 32, 48, 64, 96, 128, 256, 512)
CUS = (1, 8, 104, 240, 256, 304)
SHAPES = list(itertools.product(NS, HS, WS_, CS, KS))


def agree(op, shape, acc, n_cu, ws, kn):
    rc, p = query(op, shape, acc, n_cu, ws)
    want = restate(op, shape, n_cu, ws, kn)
    if p is None:
        assert want == rc, (op, shape, acc, n_cu, ws, rc, want)
        return 0
    try:
        assert isinstance(want, dict), want
        assert p == want, {n: (p[n], want[n]) for n in FIELDS if p[n] != want[n]}
        check_plan(p, op, shape, n_cu, ws, kn)
    except AssertionError as e:
        raise AssertionError((op, shape, acc, n_cu, ws, p)) from e
    return 1


@pytest.mark.parametrize("n_cu", CUS)
def test_every_conv_plan_of_the_grid_is_sound_and_is_the_old_rule(n_cu):
    kn = Knobs()
    accepted = 0
    for i, shape in enumerate(SHAPES):
        accepted += agree(FWD, shape, i & 1, n_cu, 0, kn)
        if i % 5 == 0:      # the inference form plans as the forward does
            agree(BIAS_ACT, shape, 0, n_cu, 0, kn)
        supported = bool(_lib.lib().winograd_supported(*shape))
        assert supported == fwd_supported(*shape) == (query(FWD, shape, 0, n_cu, 0)[0] == 0), shape
    assert 5000 < accepted < len(SHAPES) - 5000


def test_every_wgrad_plan_of_the_grid_is_sound_and_is_the_old_rule():
    kn = Knobs()
    accepted = 0
    for i, shape in enumerate(SHAPES):
        N, H, W, C, K = shape
        slab = 16 * K * C * 4
        supported = bool(_lib.lib().winograd_wgrad_supported(*shape))
        assert supported == wgrad_supported(*shape), shape
        for j, ws in enumerate((0, slab - 1, slab, 4 * slab, MIB256)):
            ok = agree(WGRAD, shape, (i + j) & 1, 0, ws, kn)      # no CU count: a wgrad plan needs none
            assert ok == (supported and ws >= slab)
            accepted += ok
    assert accepted > 5000


def test_the_debug_flag_plans_the_64_channel_form_where_the_persistent_kernel_does_not_run():
    L = _lib.lib()
    L.set_debug_flags(0x02000000)
    try:
        kn = Knobs(kb64=1)
        for shape in SHAPES[::11]:
            agree(FWD, shape, 0, 256, 0, kn)
        assert query(FWD, (2, 8, 16, 16, 64))[1]["kernel"] == K_FWD2           # one chunk: not persistent
        assert query(FWD, (2, 8, 16, 32, 64))[1]["kernel"] == K_PC
        assert query(FWD, (2, 8, 16, 32, 96))[1]["kernel"] == K_FWD1
    finally:
        L.set_debug_flags(0)
    assert query(FWD, (2, 8, 16, 16, 64))[1]["kernel"] == K_FWD1


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_are_the_entry_points():
    s = (2, 8, 8, 64, 64)
    slab = 16 * 64 * 64 * 4
    assert query(WGRAD, s, 0, 0, slab - 1)[0] == ERR_WORKSPACE and query(WGRAD, s, 0, 0, slab)[0] == 0
    assert query(WGRAD, (2, 8, 8, 64, 96), 0, 0, 0)[0] == ERR_ARG                        # the shape refusal comes first
    assert query(3, s)[0] == ERR_ARG and query(-1, s)[0] == ERR_ARG
    assert _lib.lib()._dll.ds6g_winograd_plan(FWD, *s, 0, 256, 0, 0) == ERR_ARG          # no plan to fill
    for bad in ((0, 8, 8, 64, 64), (2, 7, 8, 64, 64), (2, 8, 9, 64, 64), (2, 8, 8, 24, 64), (2, 8, 8, 64, 48), (2, 0, 8, 64, 64),
                (2, 8, 0, 64, 64), (2, 8, 8, 0, 64), (2, 8, 8, 64, 0)):
        assert query(FWD, bad)[0] == ERR_ARG and not _lib.lib().winograd_supported(*bad), bad
        assert query(WGRAD, bad, 0, 0, MIB256)[0] == ERR_ARG and not _lib.lib().winograd_wgrad_supported(*bad), bad
    # 5 tile columns: no block of 32 tiles for the conv kernels; the weight gradient walks tiles linearly.  And its channels
    # come in 64s where the conv forms take 16 in, 32 out
    assert query(FWD, (2, 8, 10, 64, 64))[0] == ERR_ARG and query(WGRAD, (2, 8, 10, 64, 64), 0, 0, MIB256)[0] == 0
    assert query(FWD, (2, 8, 8, 16, 32))[0] == 0 and query(WGRAD, (2, 8, 8, 16, 32), 0, 0, MIB256)[0] == ERR_ARG
    # the byte bounds.  A plain buffer resource ends below 2^31: x of 2^31 bytes is refused, one image less is taken - by
    # winograd_fwd_kernel, since the shifted resource of the persistent kernel ends below 2^30
    big = (128, 64, 64, 1024, 64)
    assert 128 * 64 * 64 * 1024 * 4 == 1 << 31 and query(FWD, big)[0] == ERR_ARG
    rc, p = query(FWD, (127,) + big[1:])
    assert rc == 0 and p["kernel"] == K_FWD1
    edge = (64, 64, 64, 1024, 64)                   # x is exactly 2^30 bytes; 63 images plus the (W + 1) C lead stay below
    assert query(FWD, edge)[1]["kernel"] == K_FWD1 and query(FWD, (63,) + edge[1:])[1]["kernel"] == K_PC
    assert query(WGRAD, edge, 0, 0, MIB256)[0] == ERR_ARG and query(WGRAD, (63,) + edge[1:], 0, 0, MIB256)[0] == 0
    assert query(FWD, (1, 8, 8, 8192, 4096))[0] == ERR_ARG                              # U of 2^31 bytes
    # a persistent plan needs a CU count; on this path n_cu <= 0 asks the device, so only the planner's answer is stated here:
    # every other kernel plans without one
    assert restate(FWD, (2, 8, 16, 64, 64), 0, 0, Knobs()) == ERR_LAUNCH
    assert query(FWD, (2, 8, 16, 32, 32), 0, 0, 0)[1]["kernel"] == K_FWD1 and query(WGRAD, s, 0, 0, slab)[0] == 0


# ---- the benchmark's layers: N = 60 images (12 samples x 5 frames), 256 CUs, the environment at its defaults ----------------
# H, C -> (items, rounds, grid, xcd gk) of the persistent kernel, (wgrad grid, tiles_per_split) on a 256 MiB workspace
BENCH = [((60, 64, 64, 64, 64), (1920, 8, 240, 1), None),
         ((60, 32, 32, 128, 128), (960, 4, 240, 1), ((4, 4, 64), 240)),
         ((60, 16, 16, 256, 256), (480, 2, 240, 2), ((16, 4, 16), 240)),
         ((60, 8, 8, 512, 512), (240, 1, 240, 4), ((64, 4, 4), 240))]
OTHERS = [(2, 8, 16, 32, 32), (2, 8, 8, 64, 64), (12, 64, 64, 64, 64), (16, 64, 64, 64, 64), (66, 8, 8, 32, 512), (4, 8, 8, 512, 512)]


def test_the_benchmark_layers_are_pinned():
    for shape, fwd, wgrad in BENCH:
        for op, acc in ((FWD, 0), (FWD, 1), (BIAS_ACT, 0)):            # forward, accumulating data gradient (C = K), inference
            rc, p = query(op, shape, acc, 256, 0)
            assert rc == 0 and p["kernel"] == K_PC and p["variant"] == 20002, shape
            assert (p["items"], p["rounds"], p["grid_x"], p["xcd"]) == fwd, shape
            check_plan(p, op, shape, 256, 0, Knobs())
        if wgrad:           # the model keeps the 64-channel layers' weight gradient on the direct kernel
            rc, p = query(WGRAD, shape, 1, 256, MIB256)
            assert rc == 0 and ((p["grid_x"], p["grid_y"], p["grid_z"]), p["tiles_per_split"]) == wgrad and p["xcd"] == 1, shape
            check_plan(p, WGRAD, shape, 256, MIB256, Knobs())


def test_small_and_ragged_plans_are_pinned():
    p = query(FWD, (2, 8, 16, 32, 32))[1]
    assert (p["kernel"], p["variant"], p["grid_x"], p["block"]) == (K_FWD1, 20000, 2, 256)
    p = query(FWD, (2, 8, 8, 64, 64))[1]
    assert (p["kernel"], p["items"], p["rounds"], p["grid_x"], p["xcd"]) == (K_PC, 1, 1, 1, 0)
    p = query(FWD, (12, 64, 64, 64, 64))[1]
    assert (p["items"], p["rounds"], p["grid_x"]) == (384, 2, 192)
    p = query(FWD, (66, 8, 8, 32, 512))[1]
    assert (p["items"], p["rounds"], p["grid_x"], p["xcd"]) == (264, 2, 132, 0)       # a ragged last round: plain order
    p = query(FWD, (16, 64, 64, 64, 64))[1]
    assert (p["items"], p["rounds"], p["grid_x"], p["xcd"]) == (512, 2, 256, 1)
    p = query(FWD, (4, 8, 8, 512, 512))[1]
    assert (p["items"], p["rounds"], p["grid_x"], p["xcd"]) == (16, 1, 16, 8)
    p = query(WGRAD, (1, 40, 42, 64, 64), 0, 0, MIB256)[1]                            # 420 tiles = 27 chunks, the last of 4 tiles
    assert (p["tiles_total"], p["splits"], p["tiles_per_split"]) == (420, 2, 224)
    p = query(WGRAD, (12, 16, 16, 64, 64), 0, 0, MIB256)[1]
    assert (p["tiles_total"], p["splits"], p["tiles_per_split"]) == (768, 4, 192)
    p = query(WGRAD, (12, 16, 16, 64, 64), 0, 0, 16 * 64 * 64 * 4)[1]                 # clamped to one slab
    assert (p["splits"], p["tiles_per_split"], p["ws_bytes_used"]) == (1, 768, 16 * 64 * 64 * 4)


# ---- the environment knobs: read once per process, so one fresh child process each ------------------------------------------
KNOB_CASES = ([(FWD, s, 256, 0) for s, _, _ in BENCH] + [(FWD, s, 256, 0) for s in OTHERS] +
              [(WGRAD, s, 256, MIB256) for s, _, w in BENCH if w] + [(WGRAD, (1, 40, 42, 64, 64), 256, MIB256)])
KNOB_VARS = ("DS6G_WINO_PC", "DS6G_PC_CU_RESERVE", "DS6G_PC_XCD", "DS6G_WW_XCD")
PC_ONLY = {"kernel", "variant", "items", "rounds", "grid_x", "block", "lds_bytes", "xcd", "btw_shift", "th_magic"}
# variable, value -> the restated knobs, the fields it may change in a conv plan, in a wgrad plan
KNOBS = [("DS6G_WINO_PC", "0", Knobs(pc=0), PC_ONLY, set()),
         ("DS6G_PC_CU_RESERVE", "16", Knobs(reserve=16), {"rounds", "grid_x", "xcd"}, set()),
         ("DS6G_PC_XCD", "0", Knobs(pc_xcd=0), {"xcd"}, set()),
         ("DS6G_PC_XCD", "2", Knobs(pc_xcd=2), {"xcd"}, set()),
         ("DS6G_WW_XCD", "0", Knobs(ww_xcd=0), set(), {"xcd"})]


def _child_plans():
    """what a child process prints: the plans of KNOB_CASES under its environment"""
    print(json.dumps([query(op, s, 0, n_cu, ws)[1] for op, s, n_cu, ws in KNOB_CASES]))


def test_each_environment_knob_changes_its_fields_and_nothing_else():
    base_env = {k: v for k, v in os.environ.items() if k not in KNOB_VARS and k != "DS6G_WINO_DBG"}
    base_env["PYTHONPATH"] = ROOT + os.pathsep + base_env.get("PYTHONPATH", "")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", "from tests import test_winograd_plan_cpu as t; t._child_plans()"]
    procs = [subprocess.Popen(cmd, env=dict(base_env, **{var: val}), cwd=ROOT, stdout=subprocess.PIPE) for var, val, *_ in KNOBS]
    default = [restate(op, s, n_cu, ws, Knobs()) for op, s, n_cu, ws in KNOB_CASES]
    changed_somewhere = []
    for proc, (var, val, kn, conv_fields, wgrad_fields) in zip(procs, KNOBS):
        out, _ = proc.communicate(timeout=300)
        assert proc.returncode == 0, (var, val)
        plans = json.loads(out.decode().strip().splitlines()[-1])
        changed = set()
        for (op, s, n_cu, ws), p, d in zip(KNOB_CASES, plans, default):
            assert p == restate(op, s, n_cu, ws, kn), (var, val, op, s)
            check_plan(p, op, s, n_cu, ws, kn)
            diff = {n for n in FIELDS if p[n] != d[n]}
            assert diff <= (wgrad_fields if op == WGRAD else conv_fields), (var, val, op, s, diff)
            changed |= diff
        changed_somewhere.append(changed)
        by_case = {(op, s): p for (op, s, _, _), p in zip(KNOB_CASES, plans)}
        if var == "DS6G_WINO_PC":
            p = by_case[FWD, (60, 32, 32, 128, 128)]
            assert (p["kernel"], p["variant"], p["grid_x"], p["block"], p["lds_bytes"]) == (K_FWD1, 20000, 480 * 4, 256, 0)
            assert changed == PC_ONLY
        elif var == "DS6G_PC_CU_RESERVE":       # 240 CUs: the 60-frame layers keep their 240 workgroups; 512 items take a third round
            p = by_case[FWD, (16, 64, 64, 64, 64)]
            assert (p["rounds"], p["grid_x"], p["xcd"]) == (3, 171, 0) and changed == {"rounds", "grid_x", "xcd"}
            assert by_case[FWD, (60, 16, 16, 256, 256)]["grid_x"] == 240
        elif var == "DS6G_PC_XCD":
            gks = [by_case[FWD, s]["xcd"] for s, _, _ in BENCH]
            # forced gk = 2: one channel block cannot be halved, and 30 tile blocks do not split over 4 XCD groups
            assert gks == ([0, 0, 0, 0] if val == "0" else [0, 2, 2, 0]) and changed == {"xcd"}
        else:
            assert all(p["xcd"] == 0 for (op, _), p in by_case.items() if op == WGRAD) and changed == {"xcd"}
    assert len(changed_somewhere) == len(KNOBS)
