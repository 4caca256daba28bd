"""The yardstick of the 16-bit MambaFuser tests: the CPU restatement (tests/mamba_fuser_ref.py) in fp32 under
torch.autocast("cpu", dtype) - conv / linear / matmul on 16-bit operands with 16-bit outputs, the rest in fp32: an independent
16-bit forward / backward of the same network - measured against the same restatement in fp64.  It is not the code under test.
Shared by tests/test_mamba_fuser16_gpu.py (bf16: computed live) and tools/mamba_fuser16_floor.py (f16: minutes on the CPU, so
run once and recorded in profiles/mamba_fuser16_floor.txt).  No fixtures here."""
import torch

from tests import mamba_fuser_ref as mr

F32, F64 = torch.float32, torch.float64


def rel64(a, ref):
    """max |a - ref| / max |ref| in fp64"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().max() / ref.abs().max()).item()


def grad_stats(grads, g64):
    """per-tensor L2-relative error of `grads` against the fp64 gradients `g64` -> ([(error, name)] sorted worst first, the
    share of tensors whose cosine with the fp64 gradient exceeds 0.9).  Tensors without an fp64 gradient (the temporal head
    without TFM) are skipped, as is a gradient that is identically zero in fp64."""
    l2, cos = [], []
    for k, r in g64.items():
        if r is None or r.abs().max().item() < 1e-12:
            continue
        g, r = grads[k].detach().double().cpu().flatten(), r.double().flatten()
        l2.append(((g - r).norm().item() / r.norm().item(), k))
        cos.append((torch.dot(g, r) / (g.norm() * r.norm() + 1e-300)).item())
    l2.sort(reverse=True)
    return l2, sum(c > 0.9 for c in cos) / len(cos)


def median(l2):
    return l2[len(l2) // 2][0]


def autocast_floor(p64, inputs, cfg, tfm, dtype, r64, eval64):
    """-> dict(logits, med, worst, cos, eval): the autocast run's errors against the fp64 run r64 / the fp64 eval logits"""
    with torch.autocast("cpu", dtype=dtype):
        ra = mr.train_run(p64, inputs, cfg, tfm, F32)
        ev = mr.eval_run(r64["state"], inputs, cfg, tfm, F32)
    l2, cos = grad_stats(ra["grads"], r64["grads"])
    return dict(logits=rel64(ra["logits"].float(), r64["logits"]), med=median(l2), worst=l2[0][0], cos=cos,
                eval=rel64(ev.float(), eval64), n=len(l2))
