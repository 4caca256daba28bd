"""GPU tests of the grouped head pool on bf16 / f16 maps (ds6g_h16_pool_rows3_fwd / _bwd, csrc/time_mamba.hip; the 16-bit
branch of ops.pool_rows3_fwd / _bwd).  rows and drows stay fp32: they are the temporal head's input and its gradient.

Rules (tests/test_pool_rows3_gpu.py's and tests/test_mamba16_gpu.py's): the inputs are rounded to the type the kernel reads
them in, so the fp64 reference sees exactly what the kernel sees; yardstick e_32 = the error of the same arithmetic in fp32 on
the CPU, bar32 = max(10 e_32, 1e-5).
  forward   rows is an fp32 output: max|hip - ref| / max|ref| <= bar32
  backward  dfeats is a 16-bit output - fp32 arithmetic plus ONE rounding: |hip - ref| <= u16 |ref| + bar32 max|ref| elementwise,
            u16 = 2^-8 (bf16) / 2^-11 (f16)
Every operand that is read sits inside NaN moats, every output - pre-filled with NaN - inside 0xFF moats (tests/moat.py).
Shapes (N, C): (1, 8) one piece per row, one thread per map; (3, 136) 51 pieces forward / 3264 backward, a last workgroup that is
partly idle, C no power of two; (5, 512) the model's."""
import functools

import pytest
import torch

from tests import moat
from tests import test_mamba16_gpu as t16

pytestmark = pytest.mark.gpu

DEV, F32, F64 = t16.DEV, t16.F32, t16.F64
DTYPES, U16, ST = t16.DTYPES, t16.U16, t16.ST
_rd, _in, _out, _name = t16._rd, t16._in, t16._out, t16._name
SHAPES = [(1, 8), (3, 136), (5, 512)]


def _ops():
    from deepsense6g_tii_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _f32_mode_after_each_test():
    """the kernels here do not read the compute mode; whatever a test did, the next one starts in "f32" """
    yield
    _ops().set_compute_mode("f32")


@functools.lru_cache(maxsize=None)
def _case(dtype, N, C):
    """-> (feats, drows, dins) as fp64 values that `dtype` / fp32 hold exactly, the fp64 results, the fp32 results"""
    g = torch.Generator().manual_seed(5200 + 7 * N + C)
    feats = [_rd(torch.randn(N, 8, 8, C, generator=g, dtype=F64), dtype) for _ in range(3)]
    drows = _rd(torch.randn(3 * N, C, generator=g, dtype=F64), F32)
    dins = [_rd(torch.randn(N, 8, 8, C, generator=g, dtype=F64), dtype) for _ in range(3)]

    def run(dt):
        rows = torch.cat([f.to(dt).sum(dim=(1, 2)) / 64 for f in feats], 0)       # exact inputs: the mean, in dt
        spread = [(drows.to(dt)[m * N:(m + 1) * N] / 64)[:, None, None, :].expand(N, 8, 8, C) for m in range(3)]
        res = {"rows": rows}
        for m in range(3):
            res[f"plain{m}"] = spread[m].contiguous()
            res[f"acc{m}"] = dins[m].to(dt) + spread[m]
        return res
    return feats, drows, dins, run(F64), run(F32)


def _run(dtype, N, C, feats, drows, dins):
    ops = _ops()
    guards = []

    def rd(t, dt, name):
        v, g = _in(t, dt, name)
        guards.append(g)
        return v

    def wr(shape, dt, name):
        v, g = _out(shape, dt, name)
        guards.append(g)
        return v
    fd = [rd(f, dtype, f"feat{m}") for m, f in enumerate(feats)]
    rows = wr((3 * N, C), F32, "rows")
    ops.pool_rows3_fwd(fd, rows)
    dr = rd(drows, F32, "drows")
    plain = [wr((N, 8, 8, C), dtype, f"dfeat{m}") for m in range(3)]
    ops.pool_rows3_bwd(dr, None, plain)
    din = [rd(d, dtype, f"dfeat_in{m}") for m, d in enumerate(dins)]
    acc = [wr((N, 8, 8, C), dtype, f"dfeat{m} (accumulate)") for m in range(3)]
    ops.pool_rows3_bwd(dr, din, acc)
    alias = [rd(d, dtype, f"dfeat{m} (aliased)") for m, d in enumerate(dins)]           # dfeats is dfeats_in
    ops.pool_rows3_bwd(dr, alias, alias)
    once2 = alias[2].clone()
    mixed_in = [din[0], None, alias[2]]                                                  # separate, none, aliased
    mixed = [wr((N, 8, 8, C), dtype, "dfeat0 (mixed)"), wr((N, 8, 8, C), dtype, "dfeat1 (mixed)"), alias[2]]
    ops.pool_rows3_bwd(dr, mixed_in, mixed)
    torch.cuda.synchronize()
    for g in guards:
        g()
    return rows, plain, acc, alias, mixed, once2


@pytest.mark.parametrize("N,C", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_pool_rows3_on_16bit_maps_matches_fp64_inside_moats(dtype, N, C):
    feats, drows, dins, r64, r32 = _case(dtype, N, C)
    rows, plain, acc, alias, mixed, once2 = _run(dtype, N, C, feats, drows, dins)
    assert rows.dtype == F32 and all(t.dtype == dtype for t in (*plain, *acc, *alias))
    tag = f"pool_rows3 {_name(dtype)} N={N} C={C}"
    hip = {"rows": rows}
    for m in range(3):
        hip[f"plain{m}"], hip[f"acc{m}"] = plain[m], acc[m]
    t16._gate(tag, hip, r32, r64, dtype, out16=tuple(k for k in r64 if k != "rows"))
    for m in range(2):
        assert torch.equal(alias[m], acc[m]), m                      # in place = out of place, bit for bit
    assert torch.equal(once2, acc[2])
    assert torch.equal(mixed[0], acc[0]) and torch.equal(mixed[1], plain[1])
    # alias[2] went through the kernel twice: its second pass read what the first one stored (a value of `dtype`, exact in
    # fp64), so the reference of the second pass starts from HIP's own first result
    spread = (drows[2 * N:] / 64)[:, None, None, :].expand(N, 8, 8, C)
    ref2 = once2.double().cpu() + spread
    t16._gate(tag + " aliased twice", {"twice2": alias[2]}, {"twice2": (once2.float().cpu() + spread.float())},
              {"twice2": ref2}, dtype, out16=("twice2",))
    again = _run(dtype, N, C, feats, drows, dins)                    # fixed order, no atomics: two runs are bit-identical
    for a, b in zip((rows, *plain, *acc, *alias), (again[0], *again[1], *again[2], *again[3])):
        assert torch.equal(a, b)


def _probes(N, C):
    """(m, n, position, c, k): the first and last frame of every map, the first and last channel of the first and last
    8-group; the position and the power of two differ from probe to probe"""
    out = []
    for m in range(3):
        for n in sorted({0, N - 1}):
            for c in sorted({0, 7, C - 8, C - 1}):
                i = len(out)
                out.append((m, n, (11 * i + 5) % 64, c, i % 9 - 4))
    return out


@pytest.mark.parametrize("N,C", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_one_hot_probes_land_exactly(dtype, N, C):
    """a single map element 64 * 2^k gives exactly 2^k in one rows entry; a single drows entry 64 * 2^k gives exactly 2^k at the
    64 positions of one frame of one map and 0 elsewhere.  Each probe is a launch of its own."""
    ops = _ops()
    for m, n, p, c, k in _probes(N, C):
        feats = [torch.zeros((N, 8, 8, C), dtype=dtype, device=DEV) for _ in range(3)]
        feats[m].view(N, 64, C)[n, p, c] = 64.0 * 2.0 ** k
        rows = torch.full((3 * N, C), float("nan"), dtype=F32, device=DEV)
        ops.pool_rows3_fwd(feats, rows)
        want = torch.zeros_like(rows)
        want[m * N + n, c] = 2.0 ** k
        assert torch.equal(rows, want), (m, n, p, c, k)
        drows = torch.zeros((3 * N, C), dtype=F32, device=DEV)
        drows[m * N + n, c] = 64.0 * 2.0 ** k
        dfeats = [torch.full((N, 8, 8, C), float("nan"), dtype=dtype, device=DEV) for _ in range(3)]
        ops.pool_rows3_bwd(drows, None, dfeats)
        for q in range(3):
            want = torch.zeros_like(dfeats[q])
            if q == m:
                want[n, :, :, c] = 2.0 ** k
            assert torch.equal(dfeats[q], want), (m, n, p, c, k, q)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_bad_arguments_are_refused_before_a_launch(dtype):
    from deepsense6g_tii_amd import _lib
    L, ops = _lib.lib(), _ops()
    st, s = ST[dtype], ops._stream()
    N = 2
    buf = torch.full((3 * N * 64 * 16 + 64,), float("nan"), dtype=dtype, device=DEV)
    rows = torch.full((3 * N, 16), float("nan"), dtype=F32, device=DEV)
    p, r = buf.data_ptr(), rows.data_ptr()
    for args in ((st, p, p, p, r, N, 12),            # C % 8 != 0 (a multiple of 4: the fp32 rule is not enough)
                 (st, p, p, p, r, N, 4),
                 (st, p, p + 8, p, r, N, 16),        # a map that is 8-byte aligned only
                 (st, p, p, p, r + 4, N, 16),
                 (st, p, 0, p, r, N, 16),
                 (0, p, p, p, r, N, 16)):            # the fp32 code
        with pytest.raises(_lib.Ds6gError):
            L.h16_pool_rows3_fwd(*args, s)
    for args in ((st, r, 0, 0, 0, p, p, p, N, 12),
                 (st, r, 0, p + 8, 0, p, p, p, N, 16),
                 (st, r, 0, 0, 0, p, p + 2, p, N, 16),
                 (st, r + 8, 0, 0, 0, p, p, p, N, 16),
                 (st, r, 0, 0, 0, p, 0, p, N, 16),
                 (0, r, 0, 0, 0, p, p, p, N, 16)):
        with pytest.raises(_lib.Ds6gError):
            L.h16_pool_rows3_bwd(*args, s)
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    maps = [torch.zeros((N, 8, 8, 16), dtype=dt, device=DEV) for dt in (dtype, dtype, other)]
    with pytest.raises(ValueError):                  # a mixed-dtype triple, refused by the wrapper
        ops.pool_rows3_fwd(maps, rows)
    with pytest.raises(ValueError):
        ops.pool_rows3_bwd(rows, None, [maps[0], torch.zeros((N, 8, 8, 16), dtype=F32, device=DEV), maps[1]])
    with pytest.raises(ValueError):
        ops.pool_rows3_bwd(rows, [maps[2], None, None], maps[:2] + [maps[0].clone()])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf.float()).all()) and bool(torch.isnan(rows).all())     # nothing ran


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_fp32_entry_points_are_unchanged_by_a_16bit_call(dtype):
    ops = _ops()
    N, C = 3, 136
    g = torch.Generator().manual_seed(61)
    feats = [torch.randn(N, 8, 8, C, generator=g).to(DEV) for _ in range(3)]
    drows = torch.randn(3 * N, C, generator=g).to(DEV)
    dins = [torch.randn(N, 8, 8, C, generator=g).to(DEV) for _ in range(3)]

    def fp32_run():
        rows = ops.pool_rows3_fwd(feats, torch.empty((3 * N, C), dtype=F32, device=DEV))
        d = ops.pool_rows3_bwd(drows, [dins[0], None, dins[2]], [torch.empty_like(f) for f in feats])
        return [rows, *d]
    before = fp32_run()
    f16 = [f.to(dtype) for f in feats]
    ops.pool_rows3_fwd(f16, torch.empty((3 * N, C), dtype=F32, device=DEV))
    ops.pool_rows3_bwd(drows, None, [torch.empty_like(f) for f in f16])
    after = fp32_run()
    for a, b in zip(before, after):
        assert a.dtype == F32 and torch.equal(a, b)
    # and they are the fp32 kernel's arithmetic: the 64 positions summed in position order, times 1 / 64
    s = torch.zeros((N, C), dtype=F32, device=DEV)
    for p in range(64):
        s += feats[1].view(N, 64, C)[:, p]
    assert torch.equal(before[0][N:2 * N], s * (1.0 / 64.0))
