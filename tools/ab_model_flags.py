"""A/B of TransFuser scheduling flags on the bs=12 training step (interleaved rounds in one process):
   python tools/ab_model_flags.py overlap_wgrad_trunks=1 [DTYPE=bf16]
flags (model attributes): overlap_wgrad, overlap_wgrad_trunks, multi_stream, fuse_qkv, use_winograd,
   defer_ln_finalize=0  one col_finalize launch behind every GPT LayerNorm backward, not one batched finalize per stage
   group_stage_glue=0   token pooling / upsampling of the three modality maps in three launches, not one
DEBUG_FLAGS=0x08000000 in the environment sets ds6g_set_debug_flags for BOTH legs (that value: two attention slab sums)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from deepsense6g_tii_amd import ops
from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
from deepsense6g_tii_amd.synthetic import make_batch
from deepsense6g_tii_amd.train import FusedAdamW, train_iteration

flags = dict(a.split("=") for a in sys.argv[1:])
dev = torch.device("cuda:0")
ops.set_compute_mode(os.environ.get("DTYPE", "f32"))
if os.environ.get("DEBUG_FLAGS"):
    from deepsense6g_tii_amd._lib import lib
    lib().set_debug_flags(int(os.environ["DEBUG_FLAGS"], 0))
model = TransFuser(GlobalConfig(), dev); model.train()
opt = FusedAdamW(model, lr=1e-4)
batch = make_batch(12, seed=100, device=dev)[:5]
base = {k: getattr(model, k) for k in flags}


def run(setting, n=10):
    for k, v in setting.items():
        setattr(model, k, type(base[k])(int(v)))
    for _ in range(3): train_iteration(model, opt, batch)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): train_iteration(model, opt, batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


for rnd in range(3):
    a = run(base); b = run(flags)
    print(f"round {rnd}: base {a:.2f} ms  {flags} {b:.2f} ms", flush=True)
