"""CPU tests of MambaFuser: the fp64 restatement (tests/mamba_fuser_ref.py) against the fixture generated from the reference's
own MambaFuser (tests/golden/mambafuser_golden.npz), the state dict, the arena layout and the unsupported configurations."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fusion_ref as fr
from tests import mamba_fuser_ref as mr

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
GOLD = os.path.join(GOLD_DIR, "mambafuser_golden.npz")
BARS = os.path.join(GOLD_DIR, "oracle_vs_reference_mambafuser.txt")


def _bars():
    """{quantity: bar} = max(1e-12, 10 x what the generator measured), as the generator wrote them"""
    out = {}
    with open(BARS) as f:
        next(f)
        for line in f:
            name, measured, bar = line.rstrip("\n").rsplit(None, 2)
            out[name.strip()] = float(bar)
            assert float(bar) == pytest.approx(max(1e-12, 10 * float(measured)), rel=1e-2)
    return out


def golden_case():
    """-> (cfg, fp64 parameters, inputs) of the fixture's configuration"""
    gold = np.load(GOLD)
    S, n_layer, B, seed, *stage_seeds = (int(v) for v in gold["meta"])
    cfg = fr.RefConfig(seq_len=S, n_layer=n_layer, embd_pdrop=0.0)
    return cfg, mr.make_params(cfg, seed, tuple(stage_seeds)), mr.make_inputs(cfg, B, seed=100 + seed)


def _model(**kw):
    from deepsense6g_tii_amd.mamba_fuser import MambaFuser
    from deepsense6g_tii_amd.model import GlobalConfig
    return MambaFuser(GlobalConfig(**kw), "cpu")


@functools.lru_cache(maxsize=None)
def _small():
    return _model(n_layer=1)


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    m = float(b.abs().max())
    return float((a - b).abs().max()) / m if m > 0 else float((a - b).abs().max())


@pytest.mark.parametrize("tfm", [1, 0])
def test_restatement_matches_the_reference_fixture(tfm):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    gold, bars = np.load(GOLD), _bars()
    cfg, p64, inputs = golden_case()
    r = mr.train_run(p64, inputs, cfg, tfm, torch.float64)
    tag = f"tfm{tfm}"
    assert r["kink"] >= mr.KINK_MIN and (not tfm or r["margin"] >= mr.MARGIN_MIN)
    bad = []

    def check(name, e):
        print(f"{name:80s} {e:.3e}  bar {bars[name]:.3e}")
        if not e <= bars[name]:
            bad.append((name, e, bars[name]))

    print()
    check(f"{tag} logits", _rel(r["logits"], gold[f"{tag}:logits"]))
    check(f"{tag} fused", _rel(r["cap"]["fused"], gold[f"{tag}:fused"]))
    check(f"{tag} loss", abs(float(r["loss"]) - float(gold[f"{tag}:loss"])) / abs(float(gold[f"{tag}:loss"])))
    probes = [k[len(tag) + 6:-len(":head")] for k in gold.files if k.startswith(f"{tag}:grad:") and k.endswith(":head")]
    assert len(probes) >= 12
    for k in probes:
        g = r["grads"][k]
        scale = float(gold[f"{tag}:grad:{k}:absmax"])
        e = max(float((g.flatten()[:16] - torch.from_numpy(gold[f"{tag}:grad:{k}:head"])).abs().max()) / scale,
                abs(float(g.abs().max()) - scale) / scale,
                abs(float(g.norm()) - float(gold[f"{tag}:grad:{k}:l2"])) / float(gold[f"{tag}:grad:{k}:l2"]))
        check(f"{tag} grad {k}", e)
    if not tfm:
        assert all(g is None for k, g in r["grads"].items() if k.startswith("encoder.time_mamba."))
    assert not bad, bad


def test_state_dict_has_the_fixtures_names_and_shapes():
    cfg, p64, _ = golden_case()
    model = _model(seq_len=cfg.seq_len, n_layer=cfg.n_layer)
    sd = model.state_dict()
    assert set(sd) == set(p64), sorted(set(sd) ^ set(p64))[:8]
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(p64[k].shape), k
    p32 = {k: (v.float() if v.is_floating_point() else v) for k, v in p64.items()}
    model.load_state_dict(p32, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, p32[k]), k
    other = _model(seq_len=cfg.seq_len, n_layer=cfg.n_layer)
    other.load_state_dict(model.state_dict(), strict=True)
    assert torch.equal(other.encoder.mambafusion3.mambablocks[0].backward_mamba.A_log,
                       p32["encoder.mambafusion3.mambablocks.0.backward_mamba.A_log"])


def test_stages_keep_the_references_initialisation_and_the_head_its_own():
    e = _small().encoder
    m = e.mambafusion2.mambablocks[0].forward_mamba
    assert float(m.dt_proj.bias.detach().abs().max()) == 0.0 and abs(float(m.in_proj.weight.detach().std()) - 0.02) < 2e-3
    assert float(e.mambafusion4.pos_emb.detach().abs().max()) == 0.0
    assert float(e.time_mamba.mamba.dt_proj.bias.detach().abs().max()) > 0.0     # no _init_weights on the head


def test_arena_layout_follows_the_backward_order():
    model = _small()
    named, pslice, milestone_end, total = model.arena_layout()
    ms = [model._milestone(n) for n, _ in named]
    assert ms == sorted(ms) and set(ms) == set(range(10))
    seen = set()
    for n, _ in named:
        k = model._milestone(n)
        for s in (1, 2, 3, 4):
            if f"mambafusion{s}." in n or f"vel_emb{s}." in n:
                assert k == 1 + 2 * (4 - s), n
                seen.add(("stage", s))
            if f".layer{s}." in n:
                assert k == 2 + 2 * (4 - s), n
        if "time_mamba." in n:
            assert k == 1, n
            seen.add("time")
        if n.startswith("join."):
            assert k == 0, n
        if n.endswith(("features.conv1.weight", "_model.conv1.weight", "features.bn1.weight", "_model.bn1.bias")):
            assert k == 9, n
            seen.add("stem")
    assert seen == {("stage", 1), ("stage", 2), ("stage", 3), ("stage", 4), "time", "stem"}
    offs = [pslice[n][0] for n, _ in named]
    assert offs == sorted(offs) and all(o % 4 == 0 for o in offs) and total == milestone_end[9]
    assert not any("transformer" in n for n, _ in named)


def test_unsupported_configurations_raise():
    with pytest.raises(ValueError, match="n_views"):
        _model(n_views=2, n_layer=1)
    with pytest.raises(ValueError, match="modality_missing"):
        _model(modality_missing="image", n_layer=1)
    with pytest.raises(ValueError, match="seq_len"):
        _model(TFM=1, seq_len=2, n_layer=1)
    with pytest.raises(ValueError, match="anchors"):
        _model(vert_anchors=4, n_layer=1)
    assert _model(TFM=0, seq_len=2, n_layer=1).encoder.mambafusion1.n_tokens == 386
    model = _small()
    imgs, lids, rads, gps, _ = mr.make_inputs(fr.RefConfig(seq_len=5), 1)
    with pytest.raises(RuntimeError, match="HIP"):
        model(imgs, lids, rads, gps)
    with pytest.raises(NotImplementedError):
        model(imgs, lids, rads, gps, rebuild_modality_feat_list=[imgs[0]])
    with pytest.raises(NotImplementedError):
        model.freeze_inference()
    with pytest.raises(NotImplementedError):
        model.capture_inference(imgs, lids, rads, gps)
