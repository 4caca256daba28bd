"""The Mamba fusion block and walk-form stage (deepsense6g_tii_amd/mamba_fusion.py) on fp32, bf16 and f16 storage at the
reference's shapes: B = 12, seq_len = 5 (T = 962), (C, H) = (64, 64), (128, 32), (256, 16), (512, 8).  Per width, the three
storages ALTERNATE inside one process (figure by figure: fp32, bf16, f16, then the next figure), so they share the clock
state and the cache history:

    sample_ln fwd / bwd, gate fwd / bwd, pool-swap pack fwd / bwd   the kernels of csrc/mamba_fusion.hip through ops.*
    block fwd+bwd        block_forward + block_backward, 16-bit weight copies kept by the caller (w16=)
    stage8 fwd+bwd       the 8-layer stage_forward + stage_backward, embd_pdrop 0.1, kept w16=, gradients into an arena
    tape MB              bytes of the distinct tensors the stage's tape holds

Every width of every run is a child process of its own under a time limit; the first child that fails ends the sweep.
Device-synchronised HIP-event timing, 3 warm-up and `--iters` timed calls per figure, median of 3 repeats.

usage: python tools/bench_mamba_stage16.py [--runs 2] [--iters 10] [--widths 64 128 256 512]"""
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
MAP_H = {64: 64, 128: 32, 256: 16, 512: 8}
FIGS = ("sample_ln_fwd", "sample_ln_bwd", "gate_fwd", "gate_bwd", "pack_fwd", "pack_bwd", "block_fwd_bwd", "stage8_fwd_bwd")
STORAGES = ("fp32", "bf16", "f16")


def _tensors(obj, seen):
    import torch
    if isinstance(obj, torch.Tensor):
        key = obj.untyped_storage().data_ptr()
        if key not in seen:
            seen[key] = obj.untyped_storage().nbytes()
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            _tensors(o, seen)


def child(C, iters):
    import torch
    from deepsense6g_tii_amd import mamba_fusion as mf
    from deepsense6g_tii_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H, M, n = MAP_H[C], B * T, T * C
    dts = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    stage = mf.MambaFusion(n_embd=C, ln_size=(T, C), d_state=16, d_conv=4, expand=2, n_layer=N_LAYER, vert_anchors=8,
                           horz_anchors=8, seq_len=S, embd_pdrop=0.1, config=types.SimpleNamespace(n_views=1), device=dev)
    blk = stage.mambablocks[0]
    ws = ops.Workspace(dev, mf.stage_workspace_bytes(stage, B))
    arena = {id(p): torch.zeros_like(p) for p in stage.parameters()}
    g = lambda p: (arena[id(p)].data_ptr(), 0)
    gam, bet, dgam, dbet = (torch.randn(T, C, device=dev) for _ in range(4))
    gemb, dgemb, dgps = (torch.randn(B, 2, C, device=dev) for _ in range(3))
    dpos = torch.zeros(T, C, device=dev)
    fns, tape_mb = {}, {}
    for sname, dt in dts.items():
        f = lambda *s: torch.randn(*s, device=dev).to(dt)
        x, dy = f(B, n), f(B, n)
        _, mean, rstd = ops.sample_layernorm_fwd(x, gam, bet, ws)
        fm, bm, f2, dout = f(M, C), f(M, C), f(M, C), f(M, C)
        gout = tuple(f(M, C) for _ in range(3))
        feats, outs, douts = ([f(B * S, H, H, C) for _ in range(3)] for _ in range(3))
        tok, dtok = f(B, T, C), f(B, T, C)
        params = [p.detach() for p in blk._params()]
        h16 = sname != "fp32"
        bw16 = mf.block_weight_copies16(blk, params, dt) if h16 else (None, None)
        sw16 = [mf.block_weight_copies16(b, [p.detach() for p in b._params()], dt) for b in stage.mambablocks] if h16 else None

        def block(x=x, dout=dout, params=params, bw16=bw16):
            out, tape = mf.block_forward(blk, ws, True, x, B, T, params, w16=bw16[0])
            mf.block_backward(blk, ws, tape, dout, B, T, params, gdst=[g(p) for p in blk._params()], w16=bw16[0])

        def stage8(feats=feats, outs=outs, douts=douts, sw16=sw16):
            _, tape = mf.stage_forward(stage, ws, True, feats, gemb, outs, B, drop=(0.1, 1, 0),
                                       w16=[w[0] for w in sw16] if sw16 else None)
            mf.stage_backward(stage, ws, tape, douts, (dgps, False), outs, dgemb, B, g)
            return tape

        fns[sname] = {
            "sample_ln_fwd": lambda x=x: ops.sample_layernorm_fwd(x, gam, bet, ws),
            "sample_ln_bwd": lambda x=x, dy=dy, mean=mean, rstd=rstd: ops.sample_layernorm_bwd(dy, x, mean, rstd, gam, dgam, dbet, ws),
            "gate_fwd": lambda fm=fm, bm=bm, f2=f2, gout=gout: ops.bimamba_gate_fwd(fm, bm, f2, B, T, out=gout[0]),
            "gate_bwd": lambda dout=dout, fm=fm, bm=bm, f2=f2, gout=gout: ops.bimamba_gate_bwd(dout, fm, bm, f2, B, T, out=gout),
            "pack_fwd": lambda feats=feats, tok=tok: ops.pool_swap_tokens_fwd(feats, gemb, stage.pos_emb.data_ptr(), tok, S, 0.1, 1, 0),
            "pack_bwd": lambda dtok=dtok, douts=douts, outs=outs: ops.pool_swap_tokens_bwd(dtok, douts, outs, dgemb, dpos.data_ptr(),
                                                                                         False, S, 0.1, 1, 0),
            "block_fwd_bwd": block, "stage8_fwd_bwd": stage8,
        }
        seen = {}
        _tensors(stage8()[:5], seen)
        tape_mb[sname] = sum(seen.values()) / 1e6
    res = {s: {} for s in STORAGES}
    for name in FIGS:
        for sname in STORAGES:
            fn = fns[sname][name]
            for _ in range(3):
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
            res[sname][name] = statistics.median(reps)
    for sname in STORAGES:
        res[sname]["tape_mb"] = tape_mb[sname]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--child", type=int)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.iters)
        return 0
    table = {}
    for run in range(args.runs):
        for w in args.widths:
            cmd = ["timeout", "-k", "10", "200", sys.executable, os.path.abspath(__file__), "--child", str(w), "--iters",
                   str(args.iters)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"run {run} C {w}: child ended with {p.returncode}; sweep stopped\n{p.stdout[-3000:]}")
                return 1
            table.setdefault(w, []).append(json.loads(line[0][7:]))
    print(f"Mamba fusion block and walk-form stage, B = {B}, T = {T}; microseconds per call, {args.runs} runs (each the median of "
          f"3 x {args.iters} calls), the three storages alternating inside one process per width; stage8 = {N_LAYER} layers, "
          f"embd_pdrop 0.1, kept 16-bit weight copies")
    print(f"{'C':>4s} {'H':>3s} {'figure':15s} " + " ".join(f"{s + ' run ' + str(i):>12s}" for s in STORAGES for i in range(args.runs)) +
          f" {'bf16/fp32':>10s} {'f16/fp32':>9s}")
    for w in args.widths:
        for name in FIGS + ("tape_mb",):
            ts = {s: [r[s][name] for r in table[w]] for s in STORAGES}
            med = {s: statistics.median(ts[s]) for s in STORAGES}
            print(f"{w:4d} {MAP_H[w]:3d} {name:15s} " + " ".join(f"{t:12.1f}" for s in STORAGES for t in ts[s]) +
                  f" {med['bf16'] / med['fp32']:10.2f} {med['f16'] / med['fp32']:9.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
