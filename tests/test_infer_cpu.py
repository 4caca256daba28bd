"""CPU-side checks of the frozen inference engine (TransFuser.freeze_inference): the C ABI declares and exports its new
entry points, and argument errors are raised before any GPU call."""
import ctypes

import pytest

NEW_ENTRY_POINTS = (
    "ds6g_h16_conv2d_bias_act_fwd",      # 16-bit conv with the inference epilogue
    "ds6g_bn_fold_h16",                  # BN fold to a 16-bit filter
    "ds6g_h16_stem_pack_filter",         # the stem route: pack, conv + bias + ReLU, max-pool
    "ds6g_h16_stem_bias_relu_fwd",
    "ds6g_h16_maxpool3x3s2_fwd",
)


def test_header_declares_and_library_exports_the_inference_entry_points():
    from deepsense6g_tii_amd import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
        assert hasattr(dll, name), name
    # the storage code, then the argument list of the fp32 contract (ds6g_conv2d_bias_act_fwd / ds6g_bn_fold), pointers void*
    assert protos["ds6g_h16_conv2d_bias_act_fwd"][1][1:] == protos["ds6g_conv2d_bias_act_fwd"][1]
    assert protos["ds6g_bn_fold_h16"][1][1:] == protos["ds6g_bn_fold"][1]


def test_null_pointers_are_rejected_on_the_host():
    from deepsense6g_tii_amd import _lib
    L = _lib.lib()
    for st16 in (1, 2):   # bf16, f16
        with pytest.raises(_lib.Ds6gError):
            L.h16_conv2d_bias_act_fwd(st16, 0, 0, 0, 0, 0, 1, 8, 8, 64, 64, 3, 3, 1, 1, 0, 0)
        with pytest.raises(_lib.Ds6gError):
            L.bn_fold_h16(st16, 0, 0, 0, 0, 0, 1e-5, 0, 0, 64, 9, 64, 64, 0)
        with pytest.raises(_lib.Ds6gError):
            L.h16_stem_bias_relu_fwd(st16, 0, 0, 0, 0, 1, 256, 256, 0)
        with pytest.raises(_lib.Ds6gError):
            L.h16_maxpool3x3s2_fwd(st16, 0, 0, 1, 128, 128, 64, 0)


def test_freeze_inference_argument_errors_come_before_any_gpu_call():
    """an unknown storage is a ValueError and a CPU-device model a RuntimeError (as forward()), both raised on a model that
    owns no device memory at all"""
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser, TransFuser30to5
    model = TransFuser(GlobalConfig(n_layer=1), "cpu")
    with pytest.raises(ValueError):
        model.freeze_inference(storage="fp8")
    for storage in ("f32", "bf16", "f16"):
        with pytest.raises(RuntimeError):
            model.freeze_inference(storage=storage)
    with pytest.raises(RuntimeError):
        model.freeze_inference()
    assert hasattr(TransFuser30to5, "freeze_inference")
