"""Generates tests/golden/timemamba_golden.npz by running the REFERENCE's own TimeMamba (mambafuser_seq.py:233-284) on the
CPU in fp64 and checking tests/time_mamba_ref.py against it.

mambafuser_seq.py imports `torchvision` and `mamba_ssm`, neither installed where the fixtures are made.  This script
pre-inserts the two stub modules of make_golden_mambafusion.py: an empty `torchvision.models`, and a `mamba_ssm.Mamba` that is
an nn.Module with mamba_ssm's nine parameter names and shapes whose forward is tests/mamba_ref.mamba_ref (the layer itself is
pinned by the Mamba tests; what this fixture pins is what the reference wires AROUND it: three calls of one shared layer, the
max + mean pooled scores, the two small linears and softmaxes, the weighted sums and the 4-way sum).  It then imports the
reference's mambafuser_seq, builds ITS TimeMamba, loads the restatement's state dict with strict=True (proves names and
shapes), runs forward and backward in fp64, asserts the restatement - which pushes the three modalities through the layer as
one batch - equals it to 1e-12 of each tensor's maximum, and stores outputs only: the output, absmax / l2 / head probes of the
4 input and 13 parameter gradients, the seeds, the argmax margin, and the reference object's state-dict names and shapes.
Parameters and inputs are regenerated from the seeds by tests/time_mamba_ref.py.  Nothing from the reference is copied.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_timemamba.py <directory holding mambafuser_seq.py>
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np
import torch

from make_golden_mambafusion import _install_stubs, _rel
from tests import time_mamba_ref as tr

CASES = [("b1", *tr.CASES[0]), ("b3", *tr.CASES[1])]     # (tag, B, parameter seed, input seed)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "mambafuser_seq.py")):
        raise SystemExit(__doc__)
    torch.set_num_threads(8)
    _install_stubs()
    sys.path.insert(0, sys.argv[1])
    import mambafuser_seq  # the reference file

    out, report = {}, []
    for tag, B, pseed, iseed in CASES:
        torch.manual_seed(0)
        ref = mambafuser_seq.TimeMamba(d_model=512, d_state=16, d_conv=4, expand=2).double()
        sd0 = ref.state_dict()
        assert len(sd0) == 13 and set(sd0) == set(tr.NAMES) and {k: tuple(v.shape) for k, v in sd0.items()} == tr.shapes()
        p64 = tr.make_params(seed=pseed)
        ref.load_state_dict(p64, strict=True)
        ref.train()
        ins64, dout64 = tr.make_inputs(B, seed=iseed)
        ins = {k: v.clone().requires_grad_(True) for k, v in ins64.items()}
        o = ref(*(ins[k] for k in tr.IN_KEYS))
        (o * dout64).sum().backward()
        mine, margin = tr.time_run(p64, ins64, dout64, torch.float64)
        assert margin >= tr.MARGIN_MIN, (tag, margin)
        report.append((f"{tag} out", _rel(mine["out"], o.detach())))
        out[f"{tag}:out"] = o.detach().numpy()
        grads = {"d" + k: ins[k].grad for k in tr.IN_KEYS}
        grads.update({k: v.grad for k, v in ref.named_parameters()})
        out["grad_keys"] = np.array(list(grads))
        for k, g in grads.items():
            report.append((f"{tag} {k if k[1:] in tr.IN_KEYS else 'd ' + k}", _rel(mine[k], g)))
        # one row per gradient, in grad_keys order: absmax, l2, then its first two elements (every gradient has >= 2)
        out[f"{tag}:grad_probes"] = np.array([[float(g.abs().max()), float(g.norm()), *g.flatten()[:2].tolist()]
                                              for g in grads.values()])
        out[f"{tag}:meta"] = np.array([B, pseed, iseed], dtype=np.int64)
        out[f"{tag}:margin"] = np.array(margin)
        report.append((f"{tag} argmax margin (top1 - top2) / max|row|", margin))
    out["names"] = np.array(list(sd0))
    out["shapes"] = np.array([list(v.shape) + [0] * (3 - v.dim()) for v in sd0.values()], dtype=np.int64)

    print("restatement vs reference (max abs diff / max abs of the reference tensor, fp64):")
    for k, v in report:
        print(f"  {k:50s} {v:.3e}")
    np.savez(os.path.join(HERE, "timemamba_golden.npz"), **out)
    with open(os.path.join(HERE, "oracle_vs_reference_timemamba.txt"), "w") as f:
        f.write("max abs diff / max abs of the reference tensor, tests/time_mamba_ref.py vs the reference's "
                "mambafuser_seq.TimeMamba, fp64 (torch %s, CPU)\n" % torch.__version__)
        for k, v in report:
            f.write(f"{k:50s} {v:.3e}\n")
    if not all(v <= 1e-12 for k, v in report if "margin" not in k):
        raise SystemExit("restatement does not match the reference")


if __name__ == "__main__":
    main()
