"""Generates tests/golden/mambafusion_golden.npz by running the REFERENCE's own MambaFusion (mambafuser_seq.py:111-231, with
its MambaBlock :74-109) on the CPU in fp64 and checking tests/mamba_fusion_ref.py against it.

mambafuser_seq.py imports `torchvision` and `mamba_ssm`, neither installed where the fixtures are made.  This script
pre-inserts two stub modules: an empty `torchvision.models`, and a `mamba_ssm.Mamba` that is an nn.Module with mamba_ssm's nine
parameter names and shapes whose forward is tests/mamba_ref.mamba_ref (the layer itself is pinned by the Mamba tests; what
this fixture pins is everything the reference wires AROUND it: the (T, C) LayerNorm, the flips, the gate, the channel swap,
the token order, the unpack, and self.apply(_init_weights)).  It then imports the reference's mambafuser_seq, builds ITS
MambaFusion, loads the restatement's state dict with strict=True (proves names and shapes), runs forward and backward in
fp64, asserts the restatement equals it, and stores outputs only: the four outputs, absmax / l2 / head probes of a dozen
gradients, and the seeds.  Parameters and inputs are regenerated from the seeds by tests/mamba_fusion_ref.py.  Nothing from
the reference is copied.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mambafusion.py <directory holding mambafuser_seq.py>
"""
import math
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np
import torch
from torch import nn

from tests import mamba_fusion_ref as fr
from tests import mamba_ref as mr

# (tag, C, S, n_layer, B, spread, parameter seed, input seed): the first two module-level cases of the GPU tests
CASES = [("spread", *fr.FUSION_CASES[0]), ("refinit", *fr.FUSION_CASES[1])]
PROBES = ("pos_emb", "mambablocks.0.ln1.weight", "mambablocks.0.ln1.bias", "mambablocks.0.fc1.weight",
          "mambablocks.0.fc2.bias", "mambablocks.0.forward_mamba.in_proj.weight", "mambablocks.0.forward_mamba.A_log",
          "mambablocks.0.backward_mamba.x_proj.weight", "mambablocks.1.backward_mamba.conv1d.weight",
          "mambablocks.1.backward_mamba.dt_proj.bias", "mambablocks.1.fc2.weight", "ln_f.weight")


class _StubMamba(nn.Module):
    """mamba_ssm.Mamba's parameter names and shapes; forward = the pure-torch restatement of the layer"""

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2):
        super().__init__()
        D, r = expand * d_model, math.ceil(d_model / 16)
        self.in_proj = nn.Linear(d_model, 2 * D, bias=False)
        self.conv1d = nn.Conv1d(D, D, d_conv, groups=D, padding=d_conv - 1, bias=True)
        self.x_proj = nn.Linear(D, r + 2 * d_state, bias=False)
        self.dt_proj = nn.Linear(r, D, bias=True)
        self.A_log = nn.Parameter(torch.log(torch.arange(1, d_state + 1, dtype=torch.float32)).repeat(D, 1))
        self.D = nn.Parameter(torch.ones(D))
        self.out_proj = nn.Linear(D, d_model, bias=False)

    def forward(self, x):
        return mr.mamba_ref(dict(self.named_parameters()), x)


def _install_stubs():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tv.models
    ms = types.ModuleType("mamba_ssm")
    ms.Mamba = _StubMamba
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
    import mambafuser_seq  # the reference file

    out, report = {}, []
    for tag, C, S, n_layer, B, spread, pseed, iseed in CASES:
        T = 192 * S + 2
        cfg = types.SimpleNamespace(n_views=1)
        torch.manual_seed(0)
        ref = mambafuser_seq.MambaFusion(n_embd=C, ln_size=(T, C), d_state=16, d_conv=4, expand=2, n_layer=n_layer,
                                         vert_anchors=8, horz_anchors=8, seq_len=S, embd_pdrop=0.0, config=cfg).double()
        # the init facts the module is asked to reproduce, read off the reference's own object
        sd0 = ref.state_dict()
        assert len(sd0) == 3 + 24 * n_layer and set(sd0) == set(fr.fusion_names(n_layer))
        assert float(sd0["mambablocks.0.forward_mamba.dt_proj.bias"].abs().max()) == 0.0
        assert float(sd0["pos_emb"].abs().max()) == 0.0
        assert abs(float(sd0["mambablocks.0.forward_mamba.in_proj.weight"].std()) - 0.02) < 2e-3
        p64 = fr.make_fusion_params(C, S, n_layer, seed=pseed, spread=spread)
        ref.load_state_dict(p64, strict=True)
        ref.train()
        ins64, douts64 = fr.make_fusion_inputs(C, B, S, seed=iseed)
        ins = {k: v.clone().requires_grad_(True) for k, v in ins64.items()}
        outs = ref(*(ins[k] for k in fr.IN_KEYS))
        sum((o * douts64[k]).sum() for k, o in zip(fr.OUT_KEYS, outs)).backward()
        mine, margin = fr.fusion_run(p64, ins64, douts64, n_layer, S, torch.float64)
        assert margin >= fr.KINK_MIN, (tag, margin)
        for k, o in zip(fr.OUT_KEYS, outs):
            report.append((f"{tag} {k}", _rel(mine[k], o.detach())))
            out[f"{tag}:{k}"] = o.detach().numpy()
        for k in fr.IN_KEYS:
            report.append((f"{tag} d{k}", _rel(mine["d" + k], ins[k].grad)))
        named = dict(ref.named_parameters())
        report.append((f"{tag} parameter gradients (worst)", max(_rel(mine[k], v.grad) for k, v in named.items())))
        grads = {k: named[k].grad for k in PROBES}
        grads["dimage"] = ins["image"].grad
        for k, g in grads.items():
            out[f"{tag}:grad:{k}:absmax"] = np.array(float(g.abs().max()))
            out[f"{tag}:grad:{k}:l2"] = np.array(float(g.norm()))
            out[f"{tag}:grad:{k}:head"] = g.flatten()[:16].numpy()
        out[f"{tag}:meta"] = np.array([C, S, n_layer, B, int(spread), pseed, iseed], dtype=np.int64)
        out[f"{tag}:kink_margin"] = np.array(margin)

    print("restatement vs reference (max abs diff / max abs of the reference tensor, fp64):")
    for k, v in report:
        print(f"  {k:45s} {v:.3e}")
    np.savez(os.path.join(HERE, "mambafusion_golden.npz"), **out)
    with open(os.path.join(HERE, "oracle_vs_reference_mambafusion.txt"), "w") as f:
        f.write("max abs diff / max abs of the reference tensor, tests/mamba_fusion_ref.py vs the reference's "
                "mambafuser_seq.MambaFusion, fp64 (torch %s, CPU)\n" % torch.__version__)
        for k, v in report:
            f.write(f"{k:45s} {v:.3e}\n")
    if not all(v <= 1e-12 for _, v in report):
        raise SystemExit("restatement does not match the reference")


if __name__ == "__main__":
    main()
