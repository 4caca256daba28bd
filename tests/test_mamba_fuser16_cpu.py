"""CPU-side checks of MambaFuser on 16-bit storage: the two new C entry points (ds6g_h16_pool_rows3_fwd / _bwd) are declared,
bound with the declared argument counts and refuse bad arguments on the host before any launch; ops.pool_rows3_* refuses a
mixed-dtype set of maps before it touches the library; the pure host rule that sends a stage's 16-bit GEMM weights to the walk's
shadow or to a copy (mamba_fuser.weight_route / block_weights16) on the four stage widths."""
import pytest
import torch

from deepsense6g_tii_amd import _lib

P = 0x1000   # a non-NULL, 16-byte aligned stand-in that is never dereferenced: every call below is refused on the host
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def test_the_header_declares_the_entry_points_and_the_binding_matches():
    protos = _lib.parse_header()
    fwd, bwd = protos["ds6g_h16_pool_rows3_fwd"], protos["ds6g_h16_pool_rows3_bwd"]
    # (st16, feat0..2, rows, N, C, stream) and (st16, drows, dfeat_in0..2, dfeat0..2, N, C, stream): the fp32 prototypes + st16
    assert len(fwd[1]) == 8 == len(protos["ds6g_pool_rows3_fwd"][1]) + 1
    assert len(bwd[1]) == 11 == len(protos["ds6g_pool_rows3_bwd"][1]) + 1
    L = _lib.lib()
    for name, (_, argtypes) in (("ds6g_h16_pool_rows3_fwd", fwd), ("ds6g_h16_pool_rows3_bwd", bwd)):
        assert len(getattr(L._dll, name).argtypes) == len(argtypes)
        assert callable(getattr(L, name[len("ds6g_"):]))


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    fwd_bad = [(0, P, P, P, P, 1, 8),            # st16 = 0 is fp32: it has entry points of its own
               (3, P, P, P, P, 1, 8),
               (1, P, P, P, P, 1, 12),           # C % 8
               (2, P, P, P, P, 1, 4),            # C % 4 is the fp32 rule, not enough here
               (1, P, P, P, P, 0, 8),
               (1, P, 0, P, P, 1, 8),
               (1, P, P, P, 0, 1, 8),
               (1, P, P + 8, P, P, 1, 8),        # a misaligned map
               (2, P, P, P, P + 4, 1, 8),        # misaligned rows
               (1, P, P, P, P, 1 << 20, 512)]    # N * 64 * C > 2^31
    for args in fwd_bad:
        with pytest.raises(_lib.Ds6gError):
            L.h16_pool_rows3_fwd(*args, 0)
    bwd_bad = [(0, P, 0, 0, 0, P, P, P, 1, 8),
               (1, 0, 0, 0, 0, P, P, P, 1, 8),
               (1, P, 0, 0, 0, P, P, 0, 1, 8),
               (2, P, 0, 0, 0, P, P, P, 1, 12),
               (1, P, 0, P + 8, 0, P, P, P, 1, 8),    # dfeat_in: nullable, but aligned
               (1, P, 0, 0, 0, P, P + 2, P, 1, 8),
               (2, P + 4, 0, 0, 0, P, P, P, 1, 8)]
    for args in bwd_bad:
        with pytest.raises(_lib.Ds6gError):
            L.h16_pool_rows3_bwd(*args, 0)


def test_ops_pool_rows3_refuses_mixed_dtypes_without_the_library(monkeypatch):
    from deepsense6g_tii_amd import ops

    def no_lib():
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(ops, "lib", no_lib)
    N, C = 2, 16
    mk = lambda dt: torch.zeros(N, 8, 8, C, dtype=dt)   # noqa: E731
    rows = torch.zeros(3 * N, C)
    for trio in ([mk(BF16), mk(BF16), mk(F32)], [mk(F16), mk(BF16), mk(BF16)], [mk(F32), mk(F16), mk(F32)],
                 [mk(torch.float64)] * 3):
        with pytest.raises(ValueError):
            ops.pool_rows3_fwd(trio, rows)
        with pytest.raises(ValueError):
            ops.pool_rows3_bwd(rows, None, trio)
    with pytest.raises(ValueError):    # dfeats_in of another dtype than dfeats
        ops.pool_rows3_bwd(rows, [mk(F32), None, None], [mk(BF16)] * 3)
    with pytest.raises(ValueError):
        ops.pool_rows3_bwd(rows, [None, None, mk(F16)], [mk(BF16)] * 3)


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_weight_route_on_the_four_stage_widths(C):
    from deepsense6g_tii_amd.mamba import x_proj_rows16
    from deepsense6g_tii_amd.mamba_fuser import SHADOW_ALIGN, block_weights16, weight_route
    from deepsense6g_tii_amd.mamba_fusion import MambaBlock
    blk = MambaBlock(C, (194, C), 16, 4, 2, device="cpu")
    ws = block_weights16(blk)
    assert len(ws) == 8
    names = ["fc1", "fc2"] + [f"{d}.{k}" for d in ("fwd", "bwd") for k in ("in_proj", "x_proj", "out_proj")]
    base = 0x7F0000000000
    routes = {n: weight_route(base, p.shape[0], r16) for n, (p, r16) in zip(names, ws)}
    r = blk.forward_mamba.dt_rank
    for n, (p, r16) in zip(names, ws):
        assert p.dim() == 2 and r16 % 8 == 0 and p.shape[1] % 64 == 0, (n, tuple(p.shape), r16)   # the 16-bit GEMM's shapes
        if "x_proj" in n:
            assert p.shape[0] == r + 32 and r16 == x_proj_rows16(r)
        else:
            assert r16 == p.shape[0]
    # C = 64: dt_rank 4, x_proj has 36 rows where the 16-bit GEMM needs 40 - the two x_proj weights take the copy route and
    # nothing else does; from C = 128 (40, 48, 64 rows) all eight read the shadow
    want_copy = {"fwd.x_proj", "bwd.x_proj"} if C == 64 else set()
    assert {n for n, v in routes.items() if v == "copy"} == want_copy, routes
    # the address half of the rule: whatever is not SHADOW_ALIGN-aligned is copied, whatever the shape
    assert weight_route(base + SHADOW_ALIGN, 64, 64) == "shadow"
    assert weight_route(base + SHADOW_ALIGN // 2, 64, 64) == "copy"
    assert weight_route(base + 2, 64, 64) == "copy"


def test_arena_shadow_offsets_meet_the_alignment_rule():
    """arena segments are padded to 4 elements, so every 16-bit shadow offset is a multiple of SHADOW_ALIGN bytes: on a real
    model no weight takes the copy route for its address"""
    from deepsense6g_tii_amd.mamba_fuser import SHADOW_ALIGN, MambaFuser
    from deepsense6g_tii_amd.model import GlobalConfig
    model = MambaFuser(GlobalConfig(TFM=0, seq_len=1, n_layer=1, embd_pdrop=0.0), torch.device("cpu"))
    _, pslice, _, total = model.arena_layout()
    assert total % 4 == 0
    for name, (off, n) in pslice.items():
        assert (2 * off) % SHADOW_ALIGN == 0, (name, off)
