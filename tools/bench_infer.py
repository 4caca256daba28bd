"""Frozen inference engine (TransFuser.freeze_inference) beside model.eval() in ONE process: for B = 12 and B = 1 the
model.eval() forward and the "f32" / "bf16" / "f16" engines, each eager and replayed from its HIP graph, measured in
alternating passes (every pass visits every variant once; the table shows the median pass and the min .. max spread, which
is the noise to read the differences against).  Device-synchronised timing, 3 warm-up and 20 timed forwards per pass.

Kernel launches per forward are counted from `rocprofv3 --kernel-trace --stats` runs of this script's own child mode (the
library has no call counter): a child does the set-up (model + the three engines), then N forwards of one variant; launches
per forward = (kernels of the 3-forward child - kernels of the 1-forward child) / 2, so set-up and first-call work cancel.
A child that fails leaves its output in the error message.  `--no-count` skips that.

usage: python tools/bench_infer.py [--passes 3] [--timed 20] [--no-count]"""
import argparse
import csv
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from deepsense6g_tii_amd.model import GlobalConfig, TransFuser  # noqa: E402
from deepsense6g_tii_amd.synthetic import make_batch  # noqa: E402

VARIANTS = ("model.eval()", "engine f32", "engine bf16", "engine f16")
COUNT_LO, COUNT_HI = 1, 3


def setup(dev):
    model = TransFuser(GlobalConfig(), dev).eval()
    engines = {s: model.freeze_inference(s) for s in ("f32", "bf16", "f16")}
    fns = {"model.eval()": model, "engine f32": engines["f32"], "engine bf16": engines["bf16"], "engine f16": engines["f16"]}
    return model, engines, fns


def timeit(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def child(variant, B, n):
    """set-up, then n forwards of one variant (run under rocprofv3 by count_launches)"""
    dev = torch.device("cuda:0")
    _, _, fns = setup(dev)
    batch = make_batch(B, seed=100, device=dev)[:4]
    torch.cuda.synchronize()
    with torch.no_grad():
        for _ in range(n):
            fns[variant](*batch)
    torch.cuda.synchronize()


def kernels_of(variant, B, n, tmp):
    d = os.path.join(tmp, f"c_{VARIANTS.index(variant)}_{B}_{n}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "c", "--",
           sys.executable, os.path.abspath(__file__), "--child", variant, str(B), str(n)]
    log = os.path.join(tmp, f"c_{VARIANTS.index(variant)}_{B}_{n}.log")
    with open(log, "w") as lf:   # own process group: a timeout ends rocprofv3 AND the python it started
        proc = subprocess.Popen(cmd, stdout=lf, stderr=subprocess.STDOUT, start_new_session=True)
        try:
            rc = proc.wait(timeout=600)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)
            proc.wait()
            rc = "timeout"
    if rc != 0:
        with open(log) as lf:
            raise RuntimeError(f"launch-count child ({variant}, B={B}, n={n}) ended with {rc}:\n" + lf.read()[-4000:])
    for root, _, files in os.walk(d):
        if "c_kernel_stats.csv" in files:
            with open(os.path.join(root, "c_kernel_stats.csv")) as f:
                return sum(int(r["Calls"]) for r in csv.DictReader(f))
    raise RuntimeError(f"no kernel stats under {d}")


def count_launches():
    """{(variant, B): kernel launches per eager forward}"""
    tmp = tempfile.mkdtemp(prefix="bench_infer_")
    try:
        out = {}
        for B in (12, 1):
            for v in VARIANTS:
                lo, hi = kernels_of(v, B, COUNT_LO, tmp), kernels_of(v, B, COUNT_HI, tmp)
                out[(v, B)] = (hi - lo) / (COUNT_HI - COUNT_LO)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--no-count", action="store_true")
    ap.add_argument("--child", nargs=3, metavar=("VARIANT", "B", "N"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), int(args.child[2]))
        return
    assert args.timed >= 20 and args.passes >= 1
    counts = {} if args.no_count else count_launches()   # before this process opens the GPU
    dev = torch.device("cuda:0")
    model, engines, fns = setup(dev)
    print(f"snapshot bytes: " + ", ".join(f"{s} {e.nbytes / 2**20:.0f} MiB" for s, e in engines.items()), flush=True)
    summary = {}
    for B in (12, 1):
        batch = make_batch(B, seed=100, device=dev)[:4]
        with torch.no_grad():
            runs = {}
            for v in VARIANTS:
                runs[(v, "eager")] = lambda f=fns[v]: f(*batch)
                g = model.capture_inference(*batch) if v == "model.eval()" else fns[v].capture(*batch)
                assert torch.equal(g(*batch), fns[v](*batch)), v
                runs[(v, "graph")] = lambda g=g: g(*batch)
            ref = fns["model.eval()"](*batch)
            assert torch.equal(fns["engine f32"](*batch), ref)
            dev16 = {s: ((engines[s](*batch) - ref).abs().max() / ref.abs().max()).item() for s in ("bf16", "f16")}
            times = {k: [] for k in runs}
            for _ in range(args.passes):          # alternating: every pass visits every variant once
                for k, fn in runs.items():
                    times[k].append(timeit(fn, args.timed))
        print(f"\nB = {B}: engine f32 == model.eval() bit for bit; max-norm deviation of the logits from it: "
              f"bf16 {dev16['bf16']:.2e}, f16 {dev16['f16']:.2e}")
        print(f"{'variant':14s} {'how':6s} {'ms / forward':>12s} {'min .. max over passes':>24s} {'samples/s':>10s} "
              f"{'vs model.eval()':>15s} {'launches':>9s}")
        for (v, how), ts in times.items():
            med = statistics.median(ts)
            summary[(B, v, how)] = med
            base = statistics.median(times[("model.eval()", how)])
            n = f"{counts[(v, B)]:g}" if (how == "eager" and (v, B) in counts) else ("-" if how == "eager" else "1 graph")
            print(f"{v:14s} {how:6s} {med * 1e3:12.3f} {min(ts) * 1e3:11.3f} .. {max(ts) * 1e3:9.3f} {B / med:10.0f} "
                  f"{base / med:14.2f}x {n!s:>9s}", flush=True)
    return summary


if __name__ == "__main__":
    main()
