"""The Mamba layer (deepsense6g_tii_amd/mamba.py) at the reference's fusion-stage shapes: B = 12, L = 962, d_model in
{64, 128, 256, 512}.  Per width: microseconds of each new kernel entry point (conv forward / backward, scan forward with
its checkpoints / backward), of the whole layer forward (no tape) and forward + backward, the algorithmic bytes of the two
scan entry points and the bandwidth they reach against them.

Algorithmic bytes (fp32, M = B * L tokens, D = 2 * d_model channels, 16 states; every operand once, parameters ignored):
    scan forward    reads u, delta_raw, z (3 M D) and Bm, Cm (32 M), writes y (M D)                       = 4 (4 M D + 32 M)
    scan backward   reads u, delta_raw, z, dy (4 M D) and Bm, Cm (32 M), writes du, d delta_raw, dz (3 M D)
                    and dBm, dCm (32 M)                                                                   = 4 (7 M D + 64 M)
The chunked implementation moves more than that (the forward reads u, delta_raw and Bm twice, the backward reads delta_raw, z,
dy and Cm twice and passes dBm / dCm through per-channel-group slabs); the figure is achieved bandwidth against the minimum.

Every width of every run is a child process of its own under a time limit; the first child that fails ends the sweep.
Device-synchronised HIP-event timing, 5 warm-up and `--iters` timed calls per figure, median of 3 repeats.

usage: python tools/bench_mamba.py [--runs 2] [--iters 20] [--widths 64 128 256 512]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L = 12, 962
FIGS = ("conv_fwd", "conv_bwd", "scan_fwd", "scan_bwd", "layer_fwd", "layer_fwd_bwd")


def scan_bytes(M, D):
    return 4 * (4 * M * D + 32 * M), 4 * (7 * M * D + 64 * M)


def child(d_model, iters):
    import torch
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.mamba import Mamba
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    M, D, r = B * L, 2 * d_model, max(d_model // 16, 1)
    m = Mamba(d_model, device=dev)
    ws = m._workspace(dev, B, L)
    f = lambda *s: torch.randn(*s, device=dev)
    xz, x_dbl, xc, draw, dy = f(M, 2 * D), f(M, r + 32), f(M, D), f(M, D), f(M, D)
    dxz, dxdbl, du, dd = f(M, 2 * D), f(M, r + 32), f(M, D), f(M, D)
    cw, cb, bdt, A_log, Dp = m.conv1d.weight.data, m.conv1d.bias.data, m.dt_proj.bias.data, m.A_log.data, m.D.data
    Bm, Cm, z = x_dbl[:, r:r + 16], x_dbl[:, r + 16:], xz[:, D:]
    _, saved = ops.selective_scan_fwd(xc, draw, bdt, A_log, Bm, Cm, Dp, z, B, L, ws, save=True)
    u = torch.randn(B, L, d_model, device=dev, requires_grad=True)
    dout = torch.randn(B, L, d_model, device=dev)

    def layer_fwd():
        with torch.no_grad():
            m(u)

    def layer_fwd_bwd():
        m.zero_grad(set_to_none=True)
        u.grad = None
        m(u).backward(dout)

    fns = {
        "conv_fwd": lambda: ops.causal_conv1d_silu_fwd(xz[:, :D], cw, cb, B, L),
        "conv_bwd": lambda: ops.causal_conv1d_silu_bwd(xz[:, :D], cw, cb, dy, dxz[:, :D], B, L, ws),
        "scan_fwd": lambda: ops.selective_scan_fwd(xc, draw, bdt, A_log, Bm, Cm, Dp, z, B, L, ws, save=True),
        "scan_bwd": lambda: ops.selective_scan_bwd(xc, draw, bdt, A_log, Bm, Cm, Dp, z, dy, saved, du, dd, dxdbl[:, r:r + 16],
                                                   dxdbl[:, r + 16:], dxz[:, D:], B, L, ws),
        "layer_fwd": layer_fwd, "layer_fwd_bwd": layer_fwd_bwd,
    }
    res = {}
    for name in FIGS:
        fn = fns[name]
        for _ in range(5):
            fn()
        reps = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) * 1e3 / iters)
        res[name] = statistics.median(reps)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--child", type=int)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.iters)
        return 0
    table = {}
    for run in range(args.runs):
        for w in args.widths:
            cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--child", str(w), "--iters",
                   str(args.iters)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"run {run} d_model {w}: child ended with {p.returncode}; sweep stopped\n{p.stdout[-3000:]}")
                return 1
            table.setdefault(w, []).append(json.loads(line[0][7:]))
    print(f"Mamba layer, B = {B}, L = {L}, fp32; microseconds, {args.runs} runs (each the median of 3 x {args.iters} calls)")
    print(f"{'d_model':>7s} {'figure':14s} " + " ".join(f"{'run ' + str(i):>10s}" for i in range(args.runs)) +
          f" {'spread':>8s} {'alg. MB':>9s} {'TB/s':>6s}")
    for w in args.widths:
        fb, bb = scan_bytes(B * L, 2 * w)
        for name in FIGS:
            ts = [r[name] for r in table[w]]
            nbytes = {"scan_fwd": fb, "scan_bwd": bb}.get(name)
            extra = f" {nbytes / 1e6:9.1f} {nbytes / (statistics.median(ts) * 1e-6) / 1e12:6.2f}" if nbytes else ""
            print(f"{w:7d} {name:14s} " + " ".join(f"{t:10.1f}" for t in ts) +
                  f" {(max(ts) - min(ts)) / min(ts) * 100:7.1f}%" + extra)
    return 0


if __name__ == "__main__":
    sys.exit(main())
