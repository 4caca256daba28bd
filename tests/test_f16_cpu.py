"""CPU: the f16-storage mode at the C-ABI boundary (host state only, no launch): "f16" is compute mode 5, 4 stays
refused, and every bf16-storage entry point has an f16 twin with the same signature."""
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


def test_f16_twins_mirror_the_bf16_storage_entry_points():
    protos = _lib.parse_header()
    bf16 = [n for n in protos if "bf16" in n and n not in ("ds6g_attention_fwd_bf16out", "ds6g_attention_bwd_bf16")]
    assert len(bf16) >= 29
    for name in bf16:
        twin = name.replace("bf16", "f16")
        assert twin in protos, twin
        assert protos[twin] == protos[name], twin


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
