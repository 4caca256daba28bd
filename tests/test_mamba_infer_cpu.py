"""CPU-side checks of the frozen Mamba inference path: the grouped forward-only entry points of csrc/mamba_infer.hip refuse bad
arguments on the host before anything is launched (safe without a GPU), their workspace query is host-only, the stacked-weight
layout is what the engine and the frozen block agree on, and the engine's constructor refusals."""
import ctypes

import pytest
import torch

from deepsense6g_tii_amd import _lib, ops
from deepsense6g_tii_amd.mamba_fusion import cat9_layout, frozen_plan

A = 1 << 20          # a 16-byte aligned non-null "pointer": every call below must be refused before it is looked at
B, L, D, R = 2, 40, 128, 4


def _conv_dirs(n, **over):
    d = (ops._MambaConvDir * max(n, 1))()
    for k in range(min(n, len(d))):
        d[k].x, d[k].w, d[k].bias, d[k].y, d[k].ld_x, d[k].reverse = A, A, A, A, D, k
        for f, v in over.items():
            setattr(d[k], f, v)
    return d


def _scan_dirs(n, **over):
    d = (ops._MambaScanDir * max(n, 1))()
    for k in range(min(n, len(d))):
        for f in ("u", "z", "x_dbl", "dt_w", "dt_b", "A_log", "D", "y"):
            setattr(d[k], f, A)
        d[k].ld_u, d[k].ld_z, d[k].ld_x, d[k].reverse = D, D, R + 32, k
        for f, v in over.items():
            setattr(d[k], f, v)
    return d


def _ws(Bv=B, Lv=L, Dv=D, n=2):
    return int(_lib.lib().mamba_scan_fwd_grouped_workspace_size(Bv, Lv, Dv, n))


def _conv_calls(dirs, n, Bv, Lv, Dv):
    lib = _lib.lib()
    return [lambda: lib.mamba_conv_fwd_grouped(dirs, n, Bv, Lv, Dv, 0),
            lambda: lib.h16_mamba_conv_fwd_grouped(1, dirs, n, Bv, Lv, Dv, 0),
            lambda: lib.h16_mamba_conv_fwd_grouped(2, dirs, n, Bv, Lv, Dv, 0)]


def _scan_calls(dirs, n, Bv, Lv, Dv, r, ws=A, ws_bytes=None):
    lib = _lib.lib()
    nb = _ws(Bv, Lv, Dv, n) if ws_bytes is None else ws_bytes
    return [lambda: lib.mamba_scan_fwd_grouped(dirs, n, Bv, Lv, Dv, r, ws, nb, 0),
            lambda: lib.h16_mamba_scan_fwd_grouped(1, dirs, n, Bv, Lv, Dv, r, ws, nb, 0),
            lambda: lib.h16_mamba_scan_fwd_grouped(2, dirs, n, Bv, Lv, Dv, r, ws, nb, 0)]


def _refused(calls):
    for call in calls:
        with pytest.raises(_lib.Ds6gError):
            call()


def test_descriptors_match_the_header():
    """the ctypes mirrors have the C structs' size (pointers first, then ints: no padding surprises)"""
    assert ctypes.sizeof(ops._MambaConvDir) == 4 * 8 + 2 * 4
    assert ctypes.sizeof(ops._MambaScanDir) == 8 * 8 + 4 * 4
    protos = _lib.parse_header()
    for name in ("ds6g_mamba_conv_fwd_grouped", "ds6g_h16_mamba_conv_fwd_grouped", "ds6g_mamba_scan_fwd_grouped",
                 "ds6g_h16_mamba_scan_fwd_grouped", "ds6g_mamba_scan_fwd_grouped_workspace_size"):
        assert name in protos, name
    assert protos["ds6g_mamba_scan_fwd_grouped_workspace_size"][0] is ctypes.c_size_t


def test_grouped_conv_reports_bad_arguments_without_launching():
    _refused(_conv_calls(_conv_dirs(2), 2, B, L, 64))                     # D = 64
    _refused(_conv_calls(_conv_dirs(2), 2, 0, L, D))                      # B = 0
    _refused(_conv_calls(_conv_dirs(2), 2, B, 0, D))                      # L = 0
    _refused(_conv_calls(_conv_dirs(2), 3, B, L, D))                      # ndir = 3
    _refused(_conv_calls(_conv_dirs(2), 0, B, L, D))                      # ndir = 0
    _refused(_conv_calls(None, 1, B, L, D))                               # no descriptors
    _refused(_conv_calls(_conv_dirs(2, ld_x=D + 2), 2, B, L, D))          # a stride that is no whole 16-byte piece (any type)
    _refused(_conv_calls(_conv_dirs(2, ld_x=D - 8), 2, B, L, D))          # a stride below the width
    for f in ("x", "w", "bias", "y"):
        _refused(_conv_calls(_conv_dirs(2, **{f: None}), 2, B, L, D))     # a null operand
        _refused(_conv_calls(_conv_dirs(1, **{f: A + 4}), 1, B, L, D))    # a misaligned one
    d = _conv_dirs(2)
    d[1].y = None                                                         # only the SECOND direction is bad
    _refused(_conv_calls(d, 2, B, L, D))
    lib = _lib.lib()
    with pytest.raises(_lib.Ds6gError):
        lib.h16_mamba_conv_fwd_grouped(0, _conv_dirs(1), 1, B, L, D, 0)   # storage code 0 has its own entry point
    # fp32 rows are 4-element pieces: a stride that is a multiple of 4 but not of 8 is fine for fp32 only
    with pytest.raises(_lib.Ds6gError):
        lib.h16_mamba_conv_fwd_grouped(1, _conv_dirs(1, ld_x=D + 4), 1, B, L, D, 0)


def test_grouped_scan_reports_bad_arguments_without_launching():
    _refused(_scan_calls(_scan_dirs(2), 2, B, L, 64, R))                  # D = 64
    _refused(_scan_calls(_scan_dirs(2, ld_x=6 + 32), 2, B, L, D, 6))      # r = 6
    _refused(_scan_calls(_scan_dirs(2, ld_x=36 + 32), 2, B, L, D, 36))    # r = 36
    _refused(_scan_calls(_scan_dirs(2), 2, B, L, D, 0))                   # r = 0
    _refused(_scan_calls(_scan_dirs(2), 2, 0, L, D, R, ws_bytes=1 << 20)) # B = 0
    _refused(_scan_calls(_scan_dirs(2), 3, B, L, D, R, ws_bytes=1 << 30)) # ndir = 3
    _refused(_scan_calls(None, 1, B, L, D, R))                            # no descriptors
    for f in ("ld_u", "ld_z"):
        _refused(_scan_calls(_scan_dirs(2, **{f: D + 2}), 2, B, L, D, R)) # strides that are no whole 16-byte pieces
    _refused(_scan_calls(_scan_dirs(2, ld_x=R + 32 + 2), 2, B, L, D, R))
    _refused(_scan_calls(_scan_dirs(2, ld_x=R + 28), 2, B, L, D, R))      # x_dbl narrower than dt | Bm | Cm
    for f in ("u", "z", "x_dbl", "dt_w", "dt_b", "A_log", "D", "y"):
        _refused(_scan_calls(_scan_dirs(2, **{f: None}), 2, B, L, D, R))  # a null operand
    d = _scan_dirs(2)
    d[1].x_dbl = None
    _refused(_scan_calls(d, 2, B, L, D, R))
    _refused(_scan_calls(_scan_dirs(2), 2, B, L, D, R, ws=None))          # no workspace
    _refused(_scan_calls(_scan_dirs(2), 2, B, L, D, R, ws_bytes=_ws() - 1))   # one byte short
    _refused(_scan_calls(_scan_dirs(1), 1, B, 5, D, R, ws_bytes=_ws(B, 5, D, 1) - 1))   # also where one chunk makes one launch
    with pytest.raises(_lib.Ds6gError):
        _lib.lib().h16_mamba_scan_fwd_grouped(3, _scan_dirs(1), 1, B, L, D, R, A, _ws(n=1), 0)   # unknown storage code


def test_workspace_query_is_host_only_and_grows_with_ndir():
    chunk = int(_lib.lib().selective_scan_chunk())
    one, two = _ws(n=1), _ws(n=2)
    nc = -(-L // chunk)
    assert one == B * nc * D * 17 * 4           # per (sample, chunk, channel): 16 states and one delta sum, fp32
    assert two == 2 * one
    assert _ws(B, chunk, D, 1) == B * D * 17 * 4 and _ws(B, chunk + 1, D, 1) == 2 * B * D * 17 * 4
    for bad in ((0, L, D, 1), (B, 0, D, 1), (B, L, 0, 1), (B, L, D, 0), (-1, L, D, 2)):
        assert _ws(*bad) == 0
    assert ops.mamba_scan_fwd_grouped_workspace_bytes(B, L, D, 2) == two
    # what a training stage's workspace already holds is enough for the grouped scan of both directions
    assert int(_lib.lib().selective_scan_workspace_bytes(12, 962, 1024)) >= _ws(12, 962, 1024, 2)


@pytest.mark.parametrize("C", [64, 512])
def test_stacked_weight_layout(C):
    lay = cat9_layout(C)
    D_ = 2 * C
    assert lay.n == 9 * C and lay.D == D_
    assert lay.rows == {"in_proj_fwd": (0, 4 * C), "in_proj_bwd": (4 * C, 8 * C), "fc2": (8 * C, 9 * C)}
    assert lay.cols == {"x_fwd": (0, D_), "z_fwd": (D_, 2 * D_), "x_bwd": (2 * D_, 3 * D_), "z_bwd": (3 * D_, 4 * D_),
                        "f2": (8 * C, 9 * C)}
    # the row blocks tile [0, 9C) without gaps; the column blocks refine them (x | z = the halves of one in_proj)
    spans = sorted(lay.rows.values())
    assert spans[0][0] == 0 and spans[-1][1] == lay.n and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert (lay.cols["x_fwd"][0], lay.cols["z_fwd"][1]) == lay.rows["in_proj_fwd"]
    assert (lay.cols["x_bwd"][0], lay.cols["z_bwd"][1]) == lay.rows["in_proj_bwd"]
    assert lay.cols["f2"] == lay.rows["fc2"]
    # every block starts on a 16-byte piece of either storage, and the GEMM's row count suits the 16-bit kernel
    assert all(lo % 8 == 0 and hi % 8 == 0 for lo, hi in lay.cols.values()) and lay.n % 8 == 0


def test_frozen_plan_follows_the_measured_table():
    """profiles/mamba_infer.txt: the grouped scan loses at d_model 512, the stacked GEMM at 16-bit d_model 512; everywhere else
    the new forms win or tie"""
    for C in (64, 128, 256, 512):
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            plan = frozen_plan(C, dt)
            assert plan.grouped_scan == (C != 512), (C, dt)
            assert plan.stacked_gemm == (not (C == 512 and dt != torch.float32)), (C, dt)


def test_engine_refusals_on_the_host():
    import deepsense6g_tii_amd as pkg
    from deepsense6g_tii_amd import mamba_infer
    from deepsense6g_tii_amd.mamba_fuser import MambaFuser
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
    assert pkg.freeze is mamba_infer.freeze and pkg.MambaFuserEngine is mamba_infer.MambaFuserEngine
    assert issubclass(mamba_infer.MambaFuserEngine, __import__("deepsense6g_tii_amd.infer", fromlist=["x"]).InferenceEngine)
    torch.manual_seed(0)
    cpu_model = MambaFuser(GlobalConfig(n_layer=1), "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mamba_infer.freeze(cpu_model)
    with pytest.raises(ValueError, match="storage"):
        mamba_infer.freeze(cpu_model, storage="fp8")
    with pytest.raises(TypeError, match="MambaFuser"):
        mamba_infer.freeze(TransFuser(GlobalConfig(n_layer=1), "cpu"))
    with pytest.raises(TypeError):
        mamba_infer.MambaFuserEngine(object())
    with pytest.raises(NotImplementedError, match="mamba_infer.freeze"):
        cpu_model.freeze_inference()
