"""The Mamba fusion stage (deepsense6g_tii_amd/mamba_fusion.py) at the reference's shapes: B = 12, seq_len = 5 (T = 962),
C in {64, 128, 256, 512}.  Per width: microseconds of each kernel entry point of csrc/mamba_fusion.hip, forward and backward,
with its algorithmic bytes and the bandwidth reached against them (~6.3 TB/s is the HBM roof; a tensor of
these sizes, 3 - 24 MB, usually sits in the 256 MiB Infinity Cache, so a figure above the roof is a cache figure), then one
MambaBlock and an 8-layer MambaFusion, forward (no tape) and forward + backward, and whether the 8-layer stage's fp32
outputs and gradients stay finite (reference initialisation and a unit-variance input: the stage has no residual and
multiplies two branches per block).

Algorithmic bytes (fp32, n = T * C, every operand once):
    sample_ln fwd   x, y (2 B n) + gamma, beta (2 n)                     bwd   dy, x, dx (3 B n) + gamma, dgamma, dbeta (3 n)
    gate fwd        fm, bm, f2, out (4 B n)                              bwd   dout, fm, bm, f2, dfm, dbm, df2 (7 B n)
    pack fwd        maps + gps, tokens (2 B n) + pos_emb (n)             bwd   dtokens, dmaps + dgps (2 B n) + dpos (n)
    unpack fwd/bwd  tokens, maps + gps (2 B n)
The implementation moves more in two places: the LayerNorm reads x twice in the forward (statistics, apply) and dy, x twice
in the backward (batch-loop pass, dx pass); the pack backward reads dtokens twice (scatter, dpos).

Every width of every run is a child process of its own under a time limit; the first child that fails ends the sweep.
Device-synchronised HIP-event timing, 5 warm-up and `--iters` timed calls per figure, median of 3 repeats.

usage: python tools/bench_mamba_fusion.py [--runs 2] [--iters 20] [--widths 64 128 256 512]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S = 12, 5
T = 192 * S + 2
N_LAYER = 8
KERNELS = ("sample_ln_fwd", "sample_ln_bwd", "gate_fwd", "gate_bwd", "pack_fwd", "pack_bwd", "unpack_fwd", "unpack_bwd")
FIGS = KERNELS + ("block_fwd", "block_fwd_bwd", "stage8_fwd", "stage8_fwd_bwd")


def alg_bytes(C):
    n = T * C
    return {"sample_ln_fwd": 4 * (2 * B * n + 2 * n), "sample_ln_bwd": 4 * (3 * B * n + 3 * n), "gate_fwd": 4 * 4 * B * n,
            "gate_bwd": 4 * 7 * B * n, "pack_fwd": 4 * (2 * B * n + n), "pack_bwd": 4 * (2 * B * n + n),
            "unpack_fwd": 4 * 2 * B * n, "unpack_bwd": 4 * 2 * B * n}


def child(C, iters):
    import torch
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.mamba_fusion import MambaBlock, MambaFusion
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    M, n = B * T, T * C
    f = lambda *s: torch.randn(*s, device=dev)
    ws = ops.Workspace(dev, 64 << 20)
    x, dy, gam, bet = f(B, n), f(B, n), f(T, C), f(T, C)
    dgam, dbet = f(T, C), f(T, C)
    _, mean, rstd = ops.sample_layernorm_fwd(x, gam, bet, ws)
    fm, bm, f2, dout = f(M, C), f(M, C), f(M, C), f(M, C)
    gout = tuple(f(M, C) for _ in range(3))
    maps = [f(B * S, C, 8, 8) for _ in range(3)]
    gps, pos, tok = f(B, 2, C), f(1, T, C), f(B, T, C)
    blk = MambaBlock(C, (T, C), 16, 4, 2, device=dev)
    stage = MambaFusion(n_embd=C, ln_size=(T, C), d_state=16, d_conv=4, expand=2, n_layer=N_LAYER, vert_anchors=8,
                        horz_anchors=8, seq_len=S, embd_pdrop=0.1, config=types.SimpleNamespace(n_views=1), device=dev)
    xb = torch.randn(B, T, C, device=dev, requires_grad=True)
    ins = [m.clone().requires_grad_(True) for m in maps] + [gps.clone().requires_grad_(True)]
    douts = [f(B * S, C, 8, 8) for _ in range(3)] + [f(B, 2, C)]

    def block_fwd():
        with torch.no_grad():
            blk(xb)

    def block_fwd_bwd():
        blk.zero_grad(set_to_none=True)
        xb.grad = None
        blk(xb).backward(tok)

    def stage_fwd():
        with torch.no_grad():
            stage(*ins)

    def stage_fwd_bwd():
        stage.zero_grad(set_to_none=True)
        for t in ins:
            t.grad = None
        torch.autograd.backward(stage(*ins), douts)

    fns = {
        "sample_ln_fwd": lambda: ops.sample_layernorm_fwd(x, gam, bet, ws),
        "sample_ln_bwd": lambda: ops.sample_layernorm_bwd(dy, x, mean, rstd, gam, dgam, dbet, ws),
        "gate_fwd": lambda: ops.bimamba_gate_fwd(fm, bm, f2, B, T, out=gout[0]),
        "gate_bwd": lambda: ops.bimamba_gate_bwd(dout, fm, bm, f2, B, T, out=gout),
        "pack_fwd": lambda: ops.swap_pack_fwd(*maps, gps, pos, B, S, drop_p=0.1, seed=1, seed_off=0),
        "pack_bwd": lambda: ops.swap_pack_bwd(tok, B, S, drop_p=0.1, seed=1, seed_off=0),
        "unpack_fwd": lambda: ops.token_unpack_fwd(tok, B, S),
        "unpack_bwd": lambda: ops.token_unpack_bwd(*maps, gps, B, S),
        "block_fwd": block_fwd, "block_fwd_bwd": block_fwd_bwd, "stage8_fwd": stage_fwd, "stage8_fwd_bwd": stage_fwd_bwd,
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
    stage_fwd_bwd()
    with torch.no_grad():
        outs = stage(*ins)
    tensors = list(outs) + [t.grad for t in ins] + [p.grad for p in stage.parameters()]
    res["finite"] = int(all(t is not None and bool(torch.isfinite(t).all()) for t in tensors))
    res["out_absmax"] = max(float(o.abs().max()) for o in outs)
    res["grad_absmax"] = max(float(p.grad.abs().max()) for p in stage.parameters())
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
            cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--child", str(w), "--iters",
                   str(args.iters)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"run {run} C {w}: child ended with {p.returncode}; sweep stopped\n{p.stdout[-3000:]}")
                return 1
            table.setdefault(w, []).append(json.loads(line[0][7:]))
    print(f"Mamba fusion stage, B = {B}, T = {T}, fp32; microseconds, {args.runs} runs (each the median of 3 x {args.iters} "
          f"calls); stage8 = {N_LAYER}-layer MambaFusion, embd_pdrop 0.1")
    print(f"{'C':>4s} {'figure':15s} " + " ".join(f"{'run ' + str(i):>10s}" for i in range(args.runs)) +
          f" {'spread':>8s} {'alg. MB':>9s} {'TB/s':>6s}")
    for w in args.widths:
        nb = alg_bytes(w)
        for name in FIGS:
            ts = [r[name] for r in table[w]]
            extra = f" {nb[name] / 1e6:9.1f} {nb[name] / (statistics.median(ts) * 1e-6) / 1e12:6.2f}" if name in nb else ""
            print(f"{w:4d} {name:15s} " + " ".join(f"{t:10.1f}" for t in ts) +
                  f" {(max(ts) - min(ts)) / min(ts) * 100:7.1f}%" + extra)
        r = table[w][-1]
        print(f"{w:4d} stage8 fp32 run finite: {'yes' if r['finite'] else 'NO'}  (max |output| {r['out_absmax']:.3e}, "
              f"max |parameter gradient| {r['grad_absmax']:.3e}; reference initialisation, unit-variance inputs)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
