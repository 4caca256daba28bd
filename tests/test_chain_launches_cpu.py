"""Host-side refusals of the batched entry points (deferred LayerNorm finalize, grouped stage glue): a bad argument returns
the argument error before anything is launched - on a machine without a GPU a launch would fail with the launch error
instead - and the Python descriptor layouts match the C structs."""
import ctypes
import os

import pytest

from deepsense6g_tii_amd import _lib, ops

ARG = "code 1"


def _descs(n, **over):
    keep = (ctypes.c_float * 4096)()
    arr = (ops._LnFinalizeDesc * max(n, 1))()
    for d in arr:
        d.partial = d.dgamma = d.dbeta = ctypes.addressof(keep)
        d.nblk, d.C, d.accumulate = 3, 64, 0
        for k, v in over.items():
            setattr(d, k, v)
    return arr, keep


def test_descriptor_layouts_match_the_header():
    # include/ds6g.h: {const float*, int, int, float*, float*, int} and {const void*, void*, int, int} on LP64
    assert ctypes.sizeof(ops._LnFinalizeDesc) == 40 and ops._LnFinalizeDesc.dgamma.offset == 16
    assert ops._LnFinalizeDesc.accumulate.offset == 32
    assert ctypes.sizeof(ops._MapDesc) == 24 and ops._MapDesc.frames_per_sample.offset == 16
    # the kernel sources and the public header share ONE definition of the structs (include/ds6g_types.h)
    root = os.path.dirname(_lib.HEADER)
    types = open(os.path.join(root, "ds6g_types.h")).read()
    assert "ds6g_ln_finalize_desc;" in types and "ds6g_map_desc;" in types and "#define DS6G_LN_FINALIZE_MAX 24" in types
    assert '#include "ds6g_types.h"' in open(_lib.HEADER).read()
    common = open(os.path.join(os.path.dirname(root), "deepsense6g_tii_amd", "csrc", "common.h")).read()
    assert "ds6g_types.h" in common and "typedef struct" not in common.split("ds6g_types.h")[1][:400]
    assert ops.LN_FINALIZE_MAX == 24
    protos = _lib.parse_header()
    for name in ("ds6g_layernorm_bwd_partial", "ds6g_layernorm_bwd_h16_partial", "ds6g_layernorm_finalize_batched",
                 "ds6g_avgpool_tokens_fwd3", "ds6g_avgpool_tokens_bwd3", "ds6g_upsample_add_fwd3", "ds6g_upsample_add_bwd3"):
        assert name in protos, name


@pytest.mark.parametrize("count", [0, -1, 25])
def test_finalize_refuses_a_bad_count(count):
    L = _lib.lib()
    arr, _keep = _descs(25)
    with pytest.raises(_lib.Ds6gError, match=ARG):
        L.layernorm_finalize_batched(ctypes.addressof(arr), count, 0)


@pytest.mark.parametrize("over", [dict(partial=None), dict(dgamma=None), dict(dbeta=None), dict(C=96), dict(C=192), dict(C=320), dict(C=384), dict(C=576),
                                  dict(C=0), dict(nblk=0)])
def test_finalize_refuses_bad_descriptors(over):
    L = _lib.lib()
    arr, _keep = _descs(3, **over)
    with pytest.raises(_lib.Ds6gError, match=ARG):
        L.layernorm_finalize_batched(ctypes.addressof(arr), 3, 0)
    with pytest.raises(_lib.Ds6gError, match=ARG):
        L.layernorm_finalize_batched(0, 3, 0)


def test_deferred_layernorm_bwd_refuses_null_pointers_and_widths():
    L = _lib.lib()
    keep = (ctypes.c_float * 4096)()
    p = ctypes.addressof(keep)
    good = [p, p, p, p, p, 0, p, 16, 64, 0, 0.0, 0, 0, p, 16384, 0]   # dy x mean rstd gamma add dx M C dx_drop p seed off partial bytes
    for i in (0, 1, 2, 3, 4, 6, 13):
        args = list(good)
        args[i] = 0
        with pytest.raises(_lib.Ds6gError, match=ARG):
            L.layernorm_bwd_partial(*args)
        with pytest.raises(_lib.Ds6gError, match=ARG):
            L.layernorm_bwd_h16_partial(1, args[0], 1, *args[1:])
    for C in (96, 576):
        args = list(good)
        args[8] = C
        with pytest.raises(_lib.Ds6gError, match=ARG):
            L.layernorm_bwd_partial(*args)
    args = list(good)
    args[14] = 2 * 64 * 4 - 4                                          # one float short of cdiv(16, 16) x 2C floats
    with pytest.raises(_lib.Ds6gError, match="code 3"):
        L.layernorm_bwd_partial(*args)


def test_grouped_glue_refuses_bad_arguments():
    L = _lib.lib()
    keep = (ctypes.c_float * 4096)()
    p = ctypes.addressof(keep)
    maps = (ops._MapDesc * 3)()
    for d in maps:
        d.inp, d.out, d.frames_per_sample, d.mod_off = p, p, 1, 0
    mp = ctypes.addressof(maps)
    calls = {
        "avgpool_tokens_fwd3": lambda st, m, t, B, H, C: L.avgpool_tokens_fwd3(st, m, p, t, B, H, C, 194, 0.0, 0, 0, 0),
        "avgpool_tokens_bwd3": lambda st, m, t, B, H, C: L.avgpool_tokens_bwd3(st, m, t, B, H, C, 194, 0),
        "upsample_add_fwd3": lambda st, m, t, B, H, C: L.upsample_add_fwd3(st, m, t, B, H, C, 194, 0),
        "upsample_add_bwd3": lambda st, m, t, B, H, C: L.upsample_add_bwd3(st, m, t, B, H, C, 194, 0),
    }
    for name, call in calls.items():
        for bad in ((3, mp, p, 1, 8, 64), (0, 0, p, 1, 8, 64), (0, mp, 0, 1, 8, 64), (0, mp, p, 0, 8, 64),
                    (0, mp, p, 1, 12, 64), (0, mp, p, 1, 8, 66)):
            with pytest.raises(_lib.Ds6gError, match=ARG):
                call(*bad)
    maps[1].frames_per_sample = 0
    for call in calls.values():
        with pytest.raises(_lib.Ds6gError, match=ARG):
            call(0, mp, p, 1, 8, 64)
    maps[1].frames_per_sample = 1
    maps[2].inp = None                                                 # dfeat_in alone may be null
    for name, call in calls.items():
        if name != "avgpool_tokens_bwd3":
            with pytest.raises(_lib.Ds6gError, match=ARG):
                call(0, mp, p, 1, 8, 64)
