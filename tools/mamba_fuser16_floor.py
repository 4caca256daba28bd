#!/usr/bin/env python3
"""The CPU yardstick of tests/test_mamba_fuser16_gpu.py: the MambaFuser restatement (tests/mamba_fuser_ref.py) in fp32 under
torch.autocast("cpu", bf16 / f16), on cases A and B of tests/test_mamba_fuser_gpu.py, against the same restatement in fp64.
The f16 run takes minutes on a CPU (fp16 convolutions have no fast path there), too long for a test: this tool runs it once and
the test carries the printed f16 values as named constants.  No GPU needed.

    python tools/mamba_fuser16_floor.py [--dtypes f16 bf16] [--cases A B] [--out profiles/mamba_fuser16_floor.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import mamba_fuser16_yard as yard                      # noqa: E402
from tests.test_mamba_fuser_gpu import CASES, _case               # noqa: E402

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "f16"], choices=sorted(DT))
    ap.add_argument("--cases", nargs="+", default=["A", "B"], choices=sorted(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# tools/mamba_fuser16_floor.py: the restatement under torch.autocast(\"cpu\", dtype) against its fp64 run",
             f"# torch {torch.__version__}, {torch.get_num_threads()} threads",
             "# logits / eval: max-norm relative error of the train / eval logits; med / worst: per-tensor L2-relative gradient "
             "error; cos: share of tensors with cosine > 0.9",
             f"{'dtype':<6s}{'case':<6s}{'logits':>12s}{'med':>12s}{'worst':>12s}{'cos':>8s}{'eval':>12s}{'tensors':>9s}"
             f"{'seconds':>9s}"]
    for name in args.cases:
        tfm = CASES[name][0]
        cfg, p64, inputs, r64, r32, eval64 = _case(name)
        l2, cos = yard.grad_stats(r32["grads"], r64["grads"])
        lines.append(f"{'f32':<6s}{name:<6s}{yard.rel64(r32['logits'], r64['logits']):>12.3e}{yard.median(l2):>12.3e}"
                     f"{l2[0][0]:>12.3e}{cos:>8.3f}{'':>12s}{len(l2):>9d}{'':>9s}")
        print(lines[-1], flush=True)
        for d in args.dtypes:
            t0 = time.time()
            f = yard.autocast_floor(p64, inputs, cfg, tfm, DT[d], r64, eval64)
            lines.append(f"{d:<6s}{name:<6s}{f['logits']:>12.3e}{f['med']:>12.3e}{f['worst']:>12.3e}{f['cos']:>8.3f}"
                         f"{f['eval']:>12.3e}{f['n']:>9d}{time.time() - t0:>9.0f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
