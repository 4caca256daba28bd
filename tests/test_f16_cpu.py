"""CPU: the f16-storage mode at the C-ABI boundary (host state only, no launch): "f16" is compute mode 5, 4 stays
refused, and every 16-bit-storage entry point names its storage type (bf16 / f16) by its first argument."""
import pytest

from deepsense6g_tii_amd import _lib


def test_f16_mode_round_trips_and_4_stays_refused():
    from deepsense6g_tii_amd import ops
    L = _lib.lib()
    try:
        ops.set_compute_mode("f16")
        assert L.get_compute_mode() == 5 and ops.get_compute_mode() == "f16"
        with pytest.raises(_lib.Ds6gError):
            L.set_compute_mode(4)
        with pytest.raises(ValueError):
            ops.set_compute_mode("fp8")
        assert ops.get_compute_mode() == "f16"
        ops.set_compute_mode("bf16")
        assert L.get_compute_mode() == 1
    finally:
        ops.set_compute_mode("f32")
    assert L.get_compute_mode() == 0


BF16_ONLY = ("ds6g_attention_fwd_bf16out", "ds6g_attention_bwd_bf16")   # fp32 operands in, bf16 out: no f16 form
SIZE_QUERIES = ("ds6g_h16_conv_bnstats_workspace_bytes", "ds6g_h16_stem_workspace_bytes")   # the same for either storage


def test_16bit_storage_entry_points_take_a_storage_code():
    """one entry point per 16-bit-storage kernel: `h16` in its name, the storage code (1 bf16, 2 f16) as its first argument,
    and every other code refused on the host before anything is launched"""
    import ctypes
    protos = _lib.parse_header()
    assert not [n for n in protos if "f16" in n.replace("bf16", "")]
    assert sorted(n for n in protos if "bf16" in n) == sorted(BF16_ONLY)
    h16 = [n for n in protos if "h16" in n]
    assert len(h16) >= 33
    assert all(q in h16 for q in SIZE_QUERIES)
    L = _lib.lib()
    for name in h16:
        if name in SIZE_QUERIES:
            continue
        argtypes = protos[name][1]
        assert argtypes[0] is ctypes.c_int, name
        zeros = [0.0 if t is ctypes.c_float else 0 for t in argtypes[1:]]
        for st16 in (0, 3, -1):
            with pytest.raises(_lib.Ds6gError):
                getattr(L, name[len("ds6g_"):])(st16, *zeros)


def test_f16_winograd_gating_follows_f32():
    """the fp32-storage convs in "f16" mode are those of "f32": Winograd stays on"""
    from deepsense6g_tii_amd import ops
    try:
        ops.set_compute_mode("f32")
        on32 = ops.winograd_ok((12, 32, 32, 64), 64)
        ops.set_compute_mode("f16")
        assert ops.winograd_ok((12, 32, 32, 64), 64) == on32
    finally:
        ops.set_compute_mode("f32")
