"""The frozen inference engine of MambaFuser (deepsense6g_tii_amd/mamba_infer.py) beside the model's own eval() forward, and the
grouped kernels of csrc/mamba_infer.hip beside what they replace.  One MI355X, seq_len 5, n_layer 8, TFM 1.

engine     contenders alternating in one process, `--rounds` rounds, at B = 1 and B = 12:
             eval_f32     model.eval() in mode "f32": BatchNorm folded on every call, fp32 storage
             eval_bf16    model.eval() with fold_bn_eval = False in mode "bf16": the only 16-bit inference without the engine
             eng_f32 / eng_bf16 / eng_f16   the three engines
           ms / forward, samples/s, the four fusion stages alone (the model's _stage_fwd on random maps under each contender's
           walk), and kernel launches per forward from rocprofv3 --kernel-trace --stats child runs (--no-count skips them).
           The spread of a contender is the difference between its rounds.
kernels    at B = 12, L = 962, d_model 64 / 128 / 256 / 512, fp32 and bf16 storage, alternating, `--rounds` rounds:
             scan   ops.mamba_scan_fwd_grouped (both directions, dt_proj inside)  vs  2 x (copy_cols + dt_proj GEMM +
                    selective_scan_fwd)
             conv   ops.mamba_conv_fwd_grouped  vs  2 x causal_conv1d_silu_fwd
             gemm   one [9C, C] GEMM  vs  in_proj + in_proj + fc2
Device-synchronised HIP-event timing, 3 warm-up calls, median of 3 x `--steps` calls per figure.

usage: python tools/bench_mamba_infer.py [--steps 10] [--rounds 2] [--no-count] [--no-kernels] [--no-engine]
                                         [--out profiles/mamba_infer.txt]"""
import argparse
import csv
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, N_LAYER, L_TOK = 5, 8, 962
CONTENDERS = ("eval_f32", "eval_bf16", "eng_f32", "eng_bf16", "eng_f16")
PARENT_OF = {"eng_f32": "eval_f32", "eng_bf16": "eval_bf16", "eng_f16": "eval_bf16"}
COUNT_LO, COUNT_HI = 2, 4


def build():
    import torch
    from deepsense6g_tii_amd.mamba_fuser import MambaFuser
    from deepsense6g_tii_amd.model import GlobalConfig
    torch.manual_seed(0)
    model = MambaFuser(GlobalConfig(seq_len=S, n_layer=N_LAYER, TFM=1, embd_pdrop=0.0), torch.device("cuda:0"))
    return model.eval()


def inputs(B):
    from oracle import fusion_ref as fr
    return fr.make_inputs(fr.RefConfig(seq_len=S), B, seed=100)[:4]


def contender(model, name, engines):
    """-> (forward(x), walk()) of a contender; walk() is what its stages run under"""
    import torch
    from deepsense6g_tii_amd import ops
    if name.startswith("eng_"):
        if name not in engines:
            from deepsense6g_tii_amd.mamba_infer import freeze
            engines[name] = freeze(model, name[4:])
        eng = engines[name]

        def fwd(x):
            ops.set_compute_mode("f32")
            return eng(*x)
        return fwd, lambda: eng._walk
    mode, fold = ("f32", True) if name == "eval_f32" else ("bf16", False)

    def fwd(x):
        ops.set_compute_mode(mode)
        model.fold_bn_eval = fold
        with torch.no_grad():
            return model(*x)

    def walk():
        ops.set_compute_mode(mode)
        model.fold_bn_eval = fold
        return model._new_walk(False)
    return fwd, walk


def stages_alone(model, walk, B):
    import torch
    from deepsense6g_tii_amd.model import STAGE_WIDTH
    wk = walk()
    dev = model.device
    feats = [[torch.randn(B * S, 64 >> (s - 1), 64 >> (s - 1), C, device=dev).to(wk.dtype) for _ in range(3)]
             for s, C in enumerate(STAGE_WIDTH, start=1)]
    gps = torch.randn(B, 2, 2, device=dev)

    def run():
        with torch.no_grad():
            src = (gps, gps.data_ptr(), 2 * B, 0, 2)
            for s in range(1, 5):
                _, xo, rec = model._stage_fwd(wk, s, feats[s - 1], src, B)
                src = (xo, xo.data_ptr() + (rec.T - 2) * rec.C * 4, 2, rec.T * rec.C, rec.C)
    return run


def timed(fn, n):
    import torch
    for _ in range(3):
        fn()
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
    return statistics.median(reps)


def engine_tables(steps, rounds):
    import torch
    from deepsense6g_tii_amd import ops
    model, engines, res = build(), {}, {}
    try:
        for B in (1, 12):
            x = inputs(B)
            made = {c: contender(model, c, engines) for c in CONTENDERS}
            for rnd in range(rounds):
                for c, (fwd, walk) in made.items():
                    res[(B, c, "fwd", rnd)] = timed(lambda: fwd(x), steps)
                    res[(B, c, "stages", rnd)] = timed(stages_alone(model, walk, B), steps)
            for c, (fwd, _) in made.items():
                res[(B, c, "finite")] = bool(torch.isfinite(fwd(x)).all())
    finally:
        ops.set_compute_mode("f32")
        model.fold_bn_eval = True
    return res


def count_child(name, n):
    import torch
    model = build()
    fwd, _ = contender(model, name, {})
    x = inputs(12)
    for _ in range(n):
        fwd(x)
    torch.cuda.synchronize()


def kernels_of(name, n, tmp):
    d = os.path.join(tmp, f"{name}_{n}")
    cmd = ["timeout", "-k", "10", "280", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "c", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--count-child", name, str(n)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"launch-count child ({name}, n={n}) ended with {p.returncode}:\n{p.stdout[-3000:]}")
    for root, _, files in os.walk(d):
        if "c_kernel_stats.csv" in files:
            with open(os.path.join(root, "c_kernel_stats.csv")) as f:
                return sum(int(r["Calls"]) for r in csv.DictReader(f))
    raise RuntimeError(f"no kernel stats under {d}")


def kernel_tables(steps, rounds):
    """-> {(d_model, storage, op, "new" | "old", round): ms}"""
    import torch
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.mamba import x_proj_rows16
    dev, B, L = torch.device("cuda:0"), 12, L_TOK
    M = B * L
    res = {}
    for dm in (64, 128, 256, 512):
        C, D, r = dm, 2 * dm, dm // 16
        ws = ops.Workspace(dev, max(int(ops.lib().selective_scan_workspace_bytes(B, L, D)), 64 << 20))
        for st in (torch.float32, torch.bfloat16):
            h16 = st != torch.float32
            g = torch.Generator(device="cpu").manual_seed(dm)
            rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
            n_x = x_proj_rows16(r) if h16 else r + 32
            cat = rn(M, 9 * C).to(st)
            x1 = rn(M, C).to(st)
            w9, b9 = (0.05 * rn(9 * C, C)).to(st), torch.zeros(9 * C, device=dev)
            dirs = []
            for k in range(2):
                dirs.append(dict(conv_w=0.5 * rn(D, 1, 4), conv_b=0.1 * rn(D), x_dbl=rn(M, n_x), dt_w=r ** -0.5 * rn(D, r),
                                 dt_b=0.1 * rn(D), A_log=torch.log(torch.arange(1, 17, device=dev).float()).repeat(D, 1).contiguous(),
                                 Dp=torch.ones(D, device=dev), xc=rn(M, D).to(st)))
            lin = ops.bf16_linear_fwd if h16 else ops.linear_fwd
            x_of = lambda k: cat[:, 2 * k * D:(2 * k + 1) * D]  # noqa: E731
            z_of = lambda k: cat[:, (2 * k + 1) * D:(2 * k + 2) * D]  # noqa: E731

            def scan_new():
                ops.mamba_scan_fwd_grouped([(d["xc"], z_of(k), d["x_dbl"], d["dt_w"], d["dt_b"], d["A_log"], d["Dp"], bool(k))
                                            for k, d in enumerate(dirs)], B, L, r, ws)

            def scan_old():
                for k, d in enumerate(dirs):
                    dt = ops.copy_cols(d["x_dbl"][:, :r], torch.empty((M, r), dtype=torch.float32, device=dev))
                    raw = ops.linear_fwd(dt, d["dt_w"].data_ptr(), 0, D)
                    ops.selective_scan_fwd(d["xc"], raw, d["dt_b"], d["A_log"], d["x_dbl"][:, r:r + 16],
                                           d["x_dbl"][:, r + 16:r + 32], d["Dp"], z_of(k), B, L, ws, bool(k), False)

            def conv_new():
                ops.mamba_conv_fwd_grouped([(x_of(k), d["conv_w"], d["conv_b"], bool(k)) for k, d in enumerate(dirs)], B, L)

            def conv_old():
                for k, d in enumerate(dirs):
                    ops.causal_conv1d_silu_fwd(x_of(k), d["conv_w"], d["conv_b"], B, L, bool(k))

            def gemm_new():
                lin(x1, w9.data_ptr(), b9.data_ptr(), 9 * C)

            def gemm_old():
                lin(x1, w9.data_ptr(), 0, 4 * C)
                lin(x1, w9[4 * C:].data_ptr(), 0, 4 * C)
                lin(x1, w9[8 * C:].data_ptr(), b9.data_ptr(), C)
            for rnd in range(rounds):
                for op, new, old in (("scan", scan_new, scan_old), ("conv", conv_new, conv_old), ("gemm", gemm_new, gemm_old)):
                    res[(dm, "bf16" if h16 else "f32", op, "new", rnd)] = timed(new, steps)
                    res[(dm, "bf16" if h16 else "f32", op, "old", rnd)] = timed(old, steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-count", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--count-child", nargs=2, metavar=("CONTENDER", "N"))
    args = ap.parse_args()
    if args.count_child:
        count_child(args.count_child[0], int(args.count_child[1]))
        return 0
    R = range(args.rounds)
    lines = []
    if not args.no_engine:
        res = engine_tables(args.steps, args.rounds)
        counts = {}
        if not args.no_count:
            tmp = tempfile.mkdtemp(prefix="bench_mamba_infer_")
            try:
                for c in CONTENDERS:
                    counts[c] = (kernels_of(c, COUNT_HI, tmp) - kernels_of(c, COUNT_LO, tmp)) / (COUNT_HI - COUNT_LO)
                    print(f"{c}: launches counted", file=sys.stderr, flush=True)
            except RuntimeError as e:
                print(f"launch count failed; sweep stopped\n{e}")
                return 1
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        lines += [f"MambaFuser inference, seq_len {S}, n_layer {N_LAYER}, TFM 1, one MI355X; contenders alternating in one process, "
                  f"{args.rounds} rounds, each figure the median of 3 x {args.steps} forwards; spread = max - min over the rounds",
                  f"{'B':>3s} {'contender':10s} " + " ".join(f"{'ms r' + str(i):>8s}" for i in R) + f" {'spread':>7s} {'samples/s':>10s} " +
                  " ".join(f"{'stages r' + str(i):>10s}" for i in R) + f" {'launches':>9s} {'finite':>7s}"]
        for B in (1, 12):
            for c in CONTENDERS:
                f = [res[(B, c, "fwd", i)] for i in R]
                st = [res[(B, c, "stages", i)] for i in R]
                lines.append(f"{B:3d} {c:10s} " + " ".join(f"{t:8.2f}" for t in f) + f" {max(f) - min(f):7.2f} "
                             f"{B / statistics.median(f) * 1e3:10.1f} " + " ".join(f"{t:10.2f}" for t in st) +
                             (f" {counts[c]:9.0f}" if c in counts else f" {'-':>9s}") +
                             f" {'yes' if res[(B, c, 'finite')] else 'NO':>7s}")
            for c, par in PARENT_OF.items():
                e, p = [res[(B, c, "fwd", i)] for i in R], [res[(B, par, "fwd", i)] for i in R]
                spread = max(max(e) - min(e), max(p) - min(p))
                me, mp = statistics.median(e), statistics.median(p)
                verdict = "faster" if me < mp - spread else "slower" if me > mp + spread else "inside the spread"
                lines.append(f"{B:3d} {c} vs {par}: {me:.2f} vs {mp:.2f} ms ({mp / me:.2f}x), spread {spread:.2f} ms: {verdict}")
    if not args.no_kernels:
        res = kernel_tables(args.steps, args.rounds)
        lines += ["", f"kernels at B = 12, L = {L_TOK}; new = the grouped / stacked form, old = what it replaces; ms, {args.rounds} "
                      f"rounds, median of 3 x {args.steps} calls each",
                  f"{'d_model':>7s} {'storage':8s} {'op':5s} " + " ".join(f"{'new r' + str(i):>8s}" for i in R) + " " +
                  " ".join(f"{'old r' + str(i):>8s}" for i in R) + f" {'old/new':>8s} {'spread':>7s}  verdict"]
        for dm in (64, 128, 256, 512):
            for st in ("f32", "bf16"):
                for op in ("scan", "conv", "gemm"):
                    n, o = [res[(dm, st, op, "new", i)] for i in R], [res[(dm, st, op, "old", i)] for i in R]
                    spread = max(max(n) - min(n), max(o) - min(o))
                    mn, mo = statistics.median(n), statistics.median(o)
                    verdict = "wins" if mn < mo - spread else "loses" if mn > mo + spread else "inside the spread"
                    lines.append(f"{dm:7d} {st:8s} {op:5s} " + " ".join(f"{t:8.3f}" for t in n) + " " +
                                 " ".join(f"{t:8.3f}" for t in o) + f" {mo / mn:8.2f} {spread:7.3f}  {verdict}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
