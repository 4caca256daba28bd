"""The MambaFuser training step (deepsense6g_tii_amd/mamba_fuser.py) at the reference's shapes - B = 12, seq_len 5, n_layer 8,
dropout 0.1 - with config.TFM on and off, beside TransFuser (the GPT variant), each in the compute modes "f32", "bf16" and "f16"
(f16 under train.DynamicLossScaler) in the same process: ms / step and samples/s of train_step_loss (forward + focal loss +
backward), the four fusion stages alone (each model's own _stage_fwd + _stage_bwd on random maps of the walk's shapes and
storage, one after the other on one stream), torch.cuda.max_memory_allocated of one step, and kernel launches per step from
rocprofv3 --kernel-trace --stats child runs (--no-count skips them).

"rest" = step - stages alone: stems, BasicBlocks, head, join, loss.  The three models run the same trunks, so their rests
should agree; where the Mamba models' rest is larger, the stages cost more inside the step than alone (or the reverse).

The models and their three storages alternate inside every repeat.  Device-synchronised HIP-event timing, 3 warm-up and
`--steps` timed steps per figure, median of 3 repeats; `--runs` child processes (the spread column is the noise between them).

usage: python tools/bench_mamba_fuser.py [--runs 2] [--steps 10] [--variants ...] [--modes f32 bf16 f16] [--no-count]
                                         [--count-variants ...] [--out profiles/mamba_fuser16.txt]"""
import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S, N_LAYER, PDROP = 12, 5, 8, 0.1
VARIANTS = ("transfuser", "mamba_tfm1", "mamba_tfm0")
MODES = ("f32", "bf16", "f16")
COUNT_LO, COUNT_HI = 2, 4


def build(variant):
    import torch
    from deepsense6g_tii_amd.mamba_fuser import MambaFuser
    from deepsense6g_tii_amd.model import GlobalConfig, TransFuser
    dev = torch.device("cuda:0")
    kw = dict(seq_len=S, n_layer=N_LAYER, embd_pdrop=PDROP, attn_pdrop=PDROP, resid_pdrop=PDROP)
    torch.manual_seed(0)
    if variant == "transfuser":
        model = TransFuser(GlobalConfig(**kw), dev)
    else:
        model = MambaFuser(GlobalConfig(TFM=int(variant == "mamba_tfm1"), **kw), dev)
    model.train()
    return model


def inputs():
    from oracle import fusion_ref as fr
    return fr.make_inputs(fr.RefConfig(seq_len=S), B, seed=100)[:5]


def stepper(model, mode, batch):
    """-> a callable: one train_step_loss of `model` in compute mode `mode` ("f16": under a dynamic loss scaler)"""
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.train import DynamicLossScaler
    scaler = DynamicLossScaler().bind(model.device, model.flat_parameters()[0].numel()) if mode == "f16" else None

    def step():
        ops.set_compute_mode(mode)
        return model.train_step_loss(*batch, loss_scaler=scaler)
    return step


def stages_alone(model, mode):
    """-> a callable running the four fusion stages forward + backward on random maps of the mode's storage, as the walk
    calls them"""
    import torch
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd._lib import lib
    from deepsense6g_tii_amd.model import STAGE_WIDTH
    dev = model.device
    ops.set_compute_mode(mode)
    wk = model._new_walk(True)      # refreshes the 16-bit weight shadow the stages read
    feats = [[torch.randn(B * S, 64 >> (s - 1), 64 >> (s - 1), C, device=dev).to(wk.dtype) for _ in range(3)]
             for s, C in enumerate(STAGE_WIDTH, start=1)]
    gps = torch.randn(B, 2, 2, device=dev)
    dgps4 = torch.randn(B, 2, 512, device=dev)
    for p in model.parameters():
        p.grad = None
    model._begin_backward(wk)

    def run():
        ops.set_compute_mode(mode)
        model._advance_salt()
        lib().set_dropout_salt(model._salt_cur.data_ptr())
        recs, src = [], (gps, gps.data_ptr(), 2 * B, 0, 2)
        for s in range(1, 5):
            outs, xo, rec = model._stage_fwd(wk, s, feats[s - 1], src, B)
            recs.append((rec, outs))
            src = (xo, xo.data_ptr() + (rec.T - 2) * rec.C * 4, 2, rec.T * rec.C, rec.C)
        dg = (dgps4, False)
        for rec, outs in reversed(recs):
            _, dprev = model._stage_bwd(wk, rec, outs, dg, B)   # the outputs stand in for their gradients
            dg = (dprev, False)
        model._wg_join()
        lib().set_dropout_salt(0)
    return run


def timed(fn, n):
    import torch
    reps = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        reps.append(e0.elapsed_time(e1) / n)
    return reps


def time_child(steps, variants, modes):
    import torch
    batch = inputs()
    built = {v: build(v) for v in variants}
    models = {f"{v}|{mode}": built[v] for v in variants for mode in modes}     # a model's three storages share its weights
    steppers = {k: stepper(m, k.split("|")[1], batch) for k, m in models.items()}
    res = {}
    for v, m in models.items():
        step = steppers[v]
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss, logits = step()
        torch.cuda.synchronize()
        res[f"{v}_peak_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
        res[f"{v}_resident_gib"] = base / 2 ** 30
        res[f"{v}_finite"] = int(bool(torch.isfinite(loss).all()) and bool(torch.isfinite(logits).all()))
    reps = {v: [] for v in models}
    for _ in range(3):                                  # the models and their storages alternate inside every repeat
        for v in models:
            reps[v].append(timed(steppers[v], steps)[0])
    for v in models:
        res[f"{v}_step_ms"] = statistics.median(reps[v])
    for v, m in models.items():
        run = stages_alone(m, v.split("|")[1])
        for _ in range(2):
            run()
        res[f"{v}_stages_ms"] = statistics.median(timed(run, steps))
    print("RESULT " + json.dumps(res), flush=True)


def count_child(key, n):
    import torch
    variant, mode = key.split("|")
    step = stepper(build(variant), mode, inputs())
    for _ in range(n):
        step()
    torch.cuda.synchronize()


def kernels_of(variant, n, tmp):
    d = os.path.join(tmp, f"{variant.replace('|', '_')}_{n}")
    cmd = ["timeout", "-k", "10", "280", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "c", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--count-child", variant, str(n)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"launch-count child ({variant}, n={n}) ended with {p.returncode}:\n{p.stdout[-3000:]}")
    for root, _, files in os.walk(d):
        if "c_kernel_stats.csv" in files:
            with open(os.path.join(root, "c_kernel_stats.csv")) as f:
                return sum(int(r["Calls"]) for r in csv.DictReader(f))
    raise RuntimeError(f"no kernel stats under {d}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--variants", nargs="+", default=list(VARIANTS), choices=VARIANTS)
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=MODES)
    ap.add_argument("--no-count", action="store_true")
    ap.add_argument("--count-variants", nargs="*", default=None, choices=VARIANTS, help="default: --variants")
    ap.add_argument("--out")
    ap.add_argument("--time-child", action="store_true")
    ap.add_argument("--count-child", nargs=2, metavar=("VARIANT", "N"))
    args = ap.parse_args()
    if args.time_child:
        time_child(args.steps, args.variants, args.modes)
        return 0
    if args.count_child:
        count_child(args.count_child[0], int(args.count_child[1]))
        return 0
    runs = []
    for run in range(args.runs):
        cmd = ["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--time-child", "--steps", str(args.steps),
               "--variants", *args.variants, "--modes", *args.modes]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"run {run}: child ended with {p.returncode}; sweep stopped\n{p.stdout[-3000:]}")
            return 1
        runs.append(json.loads(line[0][7:]))
        print(f"run {run} timed", file=sys.stderr, flush=True)
    counts = {}
    if not args.no_count:
        tmp = tempfile.mkdtemp(prefix="bench_mamba_fuser_")
        try:
            for v in [f"{a}|{m}" for a in (args.variants if args.count_variants is None else args.count_variants)
                      for m in args.modes]:
                counts[v] = (kernels_of(v, COUNT_HI, tmp) - kernels_of(v, COUNT_LO, tmp)) / (COUNT_HI - COUNT_LO)
                print(f"{v}: launches counted", file=sys.stderr, flush=True)
        except RuntimeError as e:
            print(f"launch count failed; sweep stopped\n{e}")
            return 1
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    lines = [f"training step (train_step_loss: forward + focal loss + backward), B = {B}, seq_len {S}, n_layer {N_LAYER}, dropout "
             f"{PDROP}, one MI355X; {args.runs} runs, each the median of 3 x {args.steps} steps, the models and their storages "
             "(compute modes; f16 under the dynamic loss scaler) alternating in one process",
             f"{'model|mode':16s} {'figure':22s} " + " ".join(f"{'run ' + str(i):>9s}" for i in range(args.runs)) + f" {'spread':>8s}"]
    for v in [f"{a}|{m}" for a in args.variants for m in args.modes]:
        for fig, key, fmt in (("ms / step", "step_ms", "9.2f"), ("stages alone, ms", "stages_ms", "9.2f"),
                              ("peak GiB in a step", "peak_gib", "9.2f"), ("resident GiB", "resident_gib", "9.2f")):
            ts = [r[f"{v}_{key}"] for r in runs]
            lines.append(f"{v:16s} {fig:22s} " + " ".join(format(t, fmt) for t in ts) +
                         f" {(max(ts) - min(ts)) / min(ts) * 100:7.1f}%")
        step = statistics.median(r[f"{v}_step_ms"] for r in runs)
        stages = statistics.median(r[f"{v}_stages_ms"] for r in runs)
        lines.append(f"{v:16s} samples/s {B / step * 1e3:.1f}; rest = step - stages alone = {step - stages:.2f} ms; launches / step "
                     f"{counts[v]:.0f}" if v in counts else
                     f"{v:16s} samples/s {B / step * 1e3:.1f}; rest = step - stages alone = {step - stages:.2f} ms")
        lines.append(f"{v:16s} loss and logits finite: {'yes' if all(r[f'{v}_finite'] for r in runs) else 'NO'}")
    # the same figures as one table (medians over the runs); working set = peak in a step - resident before it
    med = lambda v, key: statistics.median(r[f"{v}_{key}"] for r in runs)   # noqa: E731
    lines += ["", f"{'model|mode':16s} {'ms / step':>10s} {'samples/s':>10s} {'stages, ms':>11s} {'rest, ms':>9s} "
                  f"{'launches':>9s} {'working set, GiB':>17s}"]
    for v in [f"{a}|{m}" for a in args.variants for m in args.modes]:
        step, stages = med(v, "step_ms"), med(v, "stages_ms")
        launches = f"{counts[v]:.0f}" if v in counts else "-"
        lines.append(f"{v:16s} {step:10.2f} {B / step * 1e3:10.1f} {stages:11.2f} {step - stages:9.2f} {launches:>9s} "
                     f"{med(v, 'peak_gib') - med(v, 'resident_gib'):17.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
