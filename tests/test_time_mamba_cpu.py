"""CPU-side checks of the temporal Mamba fusion head: the pure-torch restatement (tests/time_mamba_ref.py) equals the fixture
made from the reference's own TimeMamba, the module keeps the reference's parameter contract, and the two new C entry points
are declared, exported and refuse bad arguments on the host before any launch."""
import functools
import os

import numpy as np
import pytest
import torch

from deepsense6g_tii_amd import _lib
from tests import mamba_ref as mr
from tests import time_mamba_ref as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timemamba_golden.npz")
NEW = ("ds6g_time_attn_fwd", "ds6g_time_attn_bwd")


@functools.lru_cache(maxsize=None)
def _run64(case):
    B, pseed, iseed = case
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return tr.time_run(tr.make_params(pseed), *tr.make_inputs(B, iseed), torch.float64)


@pytest.mark.parametrize("tag,case", [("b1", tr.CASES[0]), ("b3", tr.CASES[1])])
def test_restatement_equals_reference_fixture(tag, case):
    gold = np.load(GOLDEN)
    assert list(gold[f"{tag}:meta"]) == [int(v) for v in case]
    r64, margin = _run64(case)
    assert margin >= 1e-3 and abs(margin - float(gold[f"{tag}:margin"])) <= 1e-9 * margin
    assert mr.rel_err(r64["out"], torch.from_numpy(gold[f"{tag}:out"])) <= 1e-12
    keys = [str(k) for k in gold["grad_keys"]]
    assert len(keys) == 17 and set(keys) == {"d" + k for k in tr.IN_KEYS} | set(tr.NAMES)
    for k, (absmax, l2, *head) in zip(keys, gold[f"{tag}:grad_probes"].tolist()):
        g = r64[k].double()
        assert abs(float(g.abs().max()) - absmax) <= 1e-12 * absmax, k
        assert abs(float(g.norm()) - l2) <= 1e-12 * l2, k
        assert float((g.flatten()[:2] - torch.tensor(head, dtype=torch.float64)).abs().max()) <= 1e-12 * absmax, k


def test_restatement_argmax_is_the_lowest_channel_of_a_tie():
    ins, _ = tr.make_inputs(1, seed=5)
    y = torch.cat([ins[k] for k in tr.IN_KEYS[:3]], 0)
    y[0, 2, 7] = y[0, 2, 300] = 9.0
    probe = {}
    tr.head_ref(tr.make_head_params(), y, ins["gps"], probe)
    assert tuple(probe["argmax"].shape) == (1, 17) and int(probe["argmax"][0, 2]) == 7 and probe["margin"] == 0.0


def test_module_contract():
    from deepsense6g_tii_amd.time_mamba import TimeMamba
    gold = np.load(GOLDEN)
    want = {str(n): tuple(int(v) for v in s[:len(tr.shapes()[str(n)])]) for n, s in zip(gold["names"], gold["shapes"])}
    assert len(want) == 13 and want == tr.shapes()
    torch.manual_seed(0)
    m = TimeMamba()
    sd = m.state_dict()
    assert set(sd) == set(want) == {n for n, _ in m.named_parameters()} and len(sd) == 13
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape and sd[k].dtype == torch.float32, k
    # torch's and the layer's own initialisation: no N(0, 0.02) redraw, dt_proj.bias is softplus^-1(dt) > -7, not 0
    assert float(sd["mamba.dt_proj.bias"].min()) < -1.0 and float(sd["mlp.0.weight"].abs().max()) <= 5 ** -0.5
    assert float(sd["mlp_gps.0.bias"].abs().max()) <= 2 ** -0.5
    p = {k: v.float() for k, v in tr.make_params(seed=2).items()}
    m.load_state_dict(p, strict=True)
    for k in want:
        assert torch.equal(m.state_dict()[k], p[k]), k
    holders = (m.mlp[0].weight, m.mlp[0].bias, m.mlp_gps[0].weight, m.mlp_gps[0].bias)
    assert len(m._params()) == 13 and all(q is r for q, r in zip(m._params()[9:], holders))


def test_module_refusals():
    from deepsense6g_tii_amd.time_mamba import TimeMamba
    for bad in (dict(d_model=256), dict(d_model=64), dict(d_state=8), dict(d_conv=3)):
        with pytest.raises(ValueError):
            TimeMamba(**bad)
    m = TimeMamba()
    z = torch.zeros(1, 5, 512)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        m(z, z, z, torch.zeros(1, 2, 512))


def test_header_declares_and_library_exports_the_entry_points():
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in NEW:
        assert name in protos and hasattr(L._dll, name) and callable(getattr(L, name[len("ds6g_"):]))
    mine = [n for n in protos if n.startswith("ds6g_time_")]
    assert sorted(mine) == sorted(NEW)
    assert not [n for n in mine if n.endswith("_bytes") or n.endswith("_floats")]     # plain shapes: no size query, no workspace
    assert len(protos["ds6g_time_attn_fwd"][1]) == 15 and len(protos["ds6g_time_attn_bwd"][1]) == 17


P = 0x1000   # a non-NULL, 16-byte aligned stand-in: every call below must be refused before anything is launched


def _fwd(L, ptrs=(P,) * 10, ld=1024, B=2, S=5, C=512):
    y, gps, w5, b5, w2, b2, out, attn, score, argmax = ptrs
    return L.time_attn_fwd(y, gps, ld, w5, b5, w2, b2, out, attn, score, argmax, B, S, C, 0)


def _bwd(L, ptrs=(P,) * 11, ld=1024, ld_d=1024, B=2, S=5, C=512):
    dout, y, gps, attn, score, argmax, w5, w2, dy, dgps, part = ptrs
    return L.time_attn_bwd(dout, y, gps, ld, attn, score, argmax, w5, w2, dy, dgps, ld_d, part, B, S, C, 0)


def test_entry_points_reject_bad_arguments_without_launching():
    L = _lib.lib()

    def refused(fn, **bad):
        with pytest.raises(_lib.Ds6gError, match="code 1$"):
            fn(L, **bad)

    for fn, nptr in ((_fwd, 10), (_bwd, 11)):
        for i in range(nptr):
            refused(fn, ptrs=tuple(0 if j == i else P for j in range(nptr)))
            refused(fn, ptrs=tuple(P + 4 if j == i else P for j in range(nptr)))
        for bad in (dict(B=0), dict(B=-1), dict(S=4), dict(S=6), dict(S=1), dict(C=256), dict(C=508), dict(C=1024),
                    dict(ld=1020), dict(ld=1026), dict(ld=0), dict(ld=-1024)):
            refused(fn, **bad)
    for bad in (dict(ld_d=1020), dict(ld_d=1026), dict(ld_d=0)):
        refused(_bwd, **bad)
