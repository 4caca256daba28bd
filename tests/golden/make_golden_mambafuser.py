"""Generates tests/golden/mambafuser_golden.npz by running the REFERENCE's own MambaFuser (mambafuser_seq.py:553-597, with its
EncoderWithMamba :286-550) on the CPU in fp64 and checking tests/mamba_fuser_ref.py against it.

mambafuser_seq.py imports `torchvision` and `mamba_ssm`, neither installed where the fixtures are made.  This script
pre-inserts two stub modules: `torchvision.models.resnet18 / resnet34` returning the ResNet-v1 skeleton of make_golden.py
(attribute names conv1 / bn1 / relu / maxpool / layer1-4 / avgpool / fc), and a `mamba_ssm.Mamba` that is the stub of
make_golden_mambafusion.py (mamba_ssm's nine parameter names and shapes, forward = tests/mamba_ref.mamba_ref; the layer itself
is pinned by the Mamba tests).  It then imports the reference's mambafuser_seq and config_seq, builds ITS MambaFuser(config,
"cpu"), loads the restatement's state dict with strict=True (proves every name and shape), runs forward and backward in fp64,
asserts the restatement equals it, and stores outputs only: logits, fused features, the loss and absmax / l2 / first-16 probes
of a dozen gradients from join down to a stem conv.  seq_len = 5 (the reference hard-codes ln_size (962, C)), n_layer = 1,
B = 1, embd_pdrop = 0, once with TFM = 1 and once with TFM = 0.  Parameters and inputs are regenerated from the seeds by
tests/mamba_fuser_ref.py.  Nothing from the reference is copied.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mambafuser.py <directory holding mambafuser_seq.py>
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import fusion_ref as fr
from tests import mamba_fuser_ref as mr

SEQ_LEN, N_LAYER, BATCH = 5, 1, 1
SEED = 3                                   # parameters (and 100 + SEED: inputs)
STAGE_SEEDS = (1001, 2006, 3000, 4062)     # picked on the CPU, stage by stage, for a LeakyReLU margin >= KINK_MIN
PROBES = ("join.4.bias", "join.0.weight", "encoder.time_mamba.mamba.in_proj.weight", "encoder.time_mamba.mlp.0.weight",
          "encoder.vel_emb4.weight", "encoder.mambafusion4.ln_f.weight",
          "encoder.mambafusion4.mambablocks.0.forward_mamba.A_log", "encoder.radar_encoder._model.layer4.1.bn2.weight",
          "encoder.mambafusion3.mambablocks.0.fc2.weight", "encoder.mambafusion2.mambablocks.0.backward_mamba.conv1d.weight",
          "encoder.lidar_encoder._model.layer2.0.downsample.0.weight", "encoder.mambafusion1.pos_emb",
          "encoder.vel_emb1.weight", "encoder.image_encoder.features.conv1.weight")
TIME_ONLY = ("encoder.time_mamba.mamba.in_proj.weight", "encoder.time_mamba.mlp.0.weight")   # no gradient without TFM


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _install_stubs():
    res, mam = _load("make_golden"), _load("make_golden_mambafusion")
    tv = types.ModuleType("torchvision")
    tvm = types.ModuleType("torchvision.models")
    tvm.resnet34 = lambda weights=None, **kw: res._StubResNet((3, 4, 6, 3))
    tvm.resnet18 = lambda weights=None, **kw: res._StubResNet((2, 2, 2, 2))
    tv.models = tvm
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tvm
    ms = types.ModuleType("mamba_ssm")
    ms.Mamba = mam._StubMamba
    sys.modules["mamba_ssm"] = ms


def _rel(a, b):
    m = float(b.abs().max())
    return float((a - b).abs().max()) / m if m > 0 else float((a - b).abs().max())


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "mambafuser_seq.py")):
        raise SystemExit(__doc__)
    torch.set_num_threads(8)
    _install_stubs()
    sys.path.insert(0, sys.argv[1])
    import config_seq      # the reference's configuration class
    import mambafuser_seq  # the reference file

    cfg = fr.RefConfig(seq_len=SEQ_LEN, n_layer=N_LAYER, embd_pdrop=0.0)
    p64 = mr.make_params(cfg, SEED, STAGE_SEEDS)
    inputs = mr.make_inputs(cfg, BATCH, seed=100 + SEED)
    imgs, lids, rads, gps, target = inputs
    d = torch.float64
    out, report = {}, []
    for tfm in (1, 0):
        tag = f"tfm{tfm}"
        rc = config_seq.GlobalConfig(seq_len=SEQ_LEN, n_views=1, n_layer=N_LAYER, embd_pdrop=0.0, add_velocity=1)
        rc.TFM, rc.modality_missing = tfm, None
        torch.manual_seed(0)
        ref = mambafuser_seq.MambaFuser(rc, "cpu").double()
        sd0 = ref.state_dict()
        assert set(sd0) == set(p64), (sorted(set(sd0) ^ set(p64))[:8])
        assert all(tuple(sd0[k].shape) == tuple(p64[k].shape) for k in p64)
        ref.load_state_dict({k: v.clone() for k, v in p64.items()}, strict=True)
        ref.train()
        fused = ref.encoder([t.to(d) for t in imgs], [t.to(d) for t in lids], [t.to(d) for t in rads], gps.to(d))
        logits = ref.join(fused)
        loss = mr.focal_loss(logits, target)
        loss.backward()
        mine = mr.train_run(p64, inputs, cfg, tfm, d)
        assert mine["kink"] >= mr.KINK_MIN, (tag, mine["kink"])
        assert not tfm or mine["margin"] >= mr.MARGIN_MIN, (tag, mine["margin"])
        named = dict(ref.named_parameters())
        report.append((f"{tag} logits", _rel(mine["logits"], logits.detach())))
        report.append((f"{tag} fused", _rel(mine["cap"]["fused"], fused.detach())))
        report.append((f"{tag} loss", abs(float(mine["loss"]) - float(loss.detach())) / abs(float(loss.detach()))))
        worst = 0.0
        for k, v in named.items():
            if v.grad is None:
                assert k.startswith("encoder.time_mamba.") and not tfm and mine["grads"][k] is None, k
                continue
            worst = max(worst, _rel(mine["grads"][k], v.grad))
        report.append((f"{tag} parameter gradients (worst)", worst))
        bufs = dict(ref.named_buffers())
        report.append((f"{tag} BN running statistics (worst)",
                       max(_rel(mine["state"][k].double(), v.double()) for k, v in bufs.items() if v.is_floating_point())))
        out[f"{tag}:logits"] = logits.detach().numpy()
        out[f"{tag}:fused"] = fused.detach().numpy()
        out[f"{tag}:loss"] = np.array(float(loss.detach()))
        for k in PROBES:
            g = named[k].grad
            if g is None:
                assert k in TIME_ONLY and not tfm, k
                continue
            report.append((f"{tag} grad {k}", _rel(mine["grads"][k], g)))
            out[f"{tag}:grad:{k}:absmax"] = np.array(float(g.abs().max()))
            out[f"{tag}:grad:{k}:l2"] = np.array(float(g.norm()))
            out[f"{tag}:grad:{k}:head"] = g.flatten()[:16].numpy()
        out[f"{tag}:kink_margin"] = np.array(mine["kink"])
        if tfm:
            out[f"{tag}:argmax_margin"] = np.array(mine["margin"])
    out["meta"] = np.array([SEQ_LEN, N_LAYER, BATCH, SEED, *STAGE_SEEDS], dtype=np.int64)

    print("restatement vs reference (max abs diff / max abs of the reference tensor, fp64):")
    for k, v in report:
        print(f"  {k:80s} {v:.3e}")
    np.savez(os.path.join(HERE, "mambafuser_golden.npz"), **out)
    with open(os.path.join(HERE, "oracle_vs_reference_mambafuser.txt"), "w") as f:
        f.write("tests/mamba_fuser_ref.py vs the reference's mambafuser_seq.MambaFuser, fp64 (torch %s, CPU): max abs diff / max "
                "abs of the reference tensor as measured here, and the bar of tests/test_mamba_fuser_cpu.py = max(1e-12, 10 x "
                "measured)\n" % torch.__version__)
        for k, v in report:
            f.write(f"{k:80s} {v:.3e} {max(1e-12, 10 * v):.3e}\n")
    if not all(v <= 1e-10 for _, v in report):
        raise SystemExit("restatement does not match the reference")


if __name__ == "__main__":
    main()
