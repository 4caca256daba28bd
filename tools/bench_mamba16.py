"""The Mamba layer (deepsense6g_tii_amd/mamba.py) in fp32, bf16 and f16 storage at the reference's fusion-stage shapes:
B = 12, L = 962, d_model in {64, 128, 256, 512}.  Per width and storage, microseconds of

    conv_fwd, conv_bwd    the causal conv1d + SiLU entry points
    scan_fwd, scan_bwd    the selective-scan entry points (forward with its checkpoints)
    proj                  the six GEMMs of in_proj and out_proj (forward, data gradient, weight gradient each): the ones that
                          move to the 16-bit GEMM
    layer_fwd             the whole layer, no tape
    layer_fwd_bwd         forward + backward through the module (one autograd node)
    walk_fwd_bwd          layer_forward + layer_backward called directly, the way a model walk does: no autograd node, and the
                          16-bit weight copies passed in (w16=) instead of cast on every call
    rest                  layer_fwd_bwd - (conv + scan + proj): the low-rank side (x_proj, dt_proj, the dt column copies), the
                          casts of the 16-bit path (three weight copies per direction, xc -> fp32, dxc -> 16-bit) and the host
and the bytes the layer keeps on its tape for the backward.

The three storages alternate figure by figure inside ONE child process per width, so they see the same machine state; every
width of every run is a child of its own under a time limit, and the first child that fails ends the sweep.
Device-synchronised HIP-event timing, 5 warm-up and `--iters` timed calls per figure, median of 3 repeats.

usage: python tools/bench_mamba16.py [--runs 2] [--iters 20] [--widths 64 128 256 512]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L = 12, 962
FIGS = ("conv_fwd", "conv_bwd", "scan_fwd", "scan_bwd", "proj", "layer_fwd", "layer_fwd_bwd", "walk_fwd_bwd")
STORAGES = ("fp32", "bf16", "f16")


def _figures(torch, ops, m, dt, d_model):
    """-> ({figure: callable}, tape bytes) of one storage type"""
    from deepsense6g_tii_amd.mamba import layer_backward, layer_forward, weight_copies16
    dev = torch.device("cuda:0")
    F32 = torch.float32
    M, D, r = B * L, 2 * d_model, m.dt_rank
    ws = m._workspace(dev, B, L)
    f = lambda *s, t=F32: torch.randn(*s, device=dev).to(t)
    xz, xc, dy, dxz = f(M, 2 * D, t=dt), f(M, D, t=dt), f(M, D, t=dt), f(M, 2 * D, t=dt)
    x_dbl, draw, dxdbl, du, dd = f(M, r + 32), f(M, D), f(M, r + 32), f(M, D), f(M, D)
    cw, cb, bdt, A_log, Dp = m.conv1d.weight.data, m.conv1d.bias.data, m.dt_proj.bias.data, m.A_log.data, m.D.data
    Bm, Cm, z = x_dbl[:, r:r + 16], x_dbl[:, r + 16:], xz[:, D:]
    u2, y, dout2 = f(M, d_model, t=dt), f(M, D, t=dt), f(M, d_model, t=dt)
    w_in, w_out = m.in_proj.weight.data, m.out_proj.weight.data
    g_in, g_out = torch.empty_like(w_in), torch.empty_like(w_out)
    conv_f, conv_b, scan_f, scan_b = (ops.causal_conv1d_silu_fwd, ops.causal_conv1d_silu_bwd, ops.selective_scan_fwd,
                                      ops.selective_scan_bwd)   # they pick the entry point by operand dtype
    if dt == F32:
        p_in, p_out = w_in.data_ptr(), w_out.data_ptr()
        lin_f, lin_d, lin_w = ops.linear_fwd, ops.linear_dgrad, ops.linear_wgrad
        w16 = alive = None
    else:
        w16, alive = weight_copies16(m, m._params(), dt)
        p_in, _, p_out = w16
        lin_f, lin_d, lin_w = ops.bf16_linear_fwd, ops.bf16_linear_dgrad, ops.bf16_linear_wgrad
    _, saved = scan_f(xc, draw, bdt, A_log, Bm, Cm, Dp, z, B, L, ws, save=True)
    u = torch.randn(B, L, d_model, device=dev).to(dt).requires_grad_(True)
    dout = torch.randn(B, L, d_model, device=dev).to(dt)

    def proj():
        lin_f(u2, p_in, 0, 2 * D)
        lin_f(y, p_out, 0, d_model)
        lin_d(dout2, p_out, D)
        lin_d(dxz, p_in, d_model)
        lin_w(y, dout2, g_out.data_ptr(), ws)
        lin_w(u2, dxz, g_in.data_ptr(), ws)

    def layer_fwd():
        with torch.no_grad():
            m(u)

    def layer_fwd_bwd():
        m.zero_grad(set_to_none=True)
        u.grad = None
        m(u).backward(dout)

    proj.alive = alive   # the 16-bit weight copies live as long as the figures that read them
    params = [q.detach() for q in m._params()]
    uw = u.detach().reshape(M, d_model)

    def walk_fwd_bwd():
        _, tp = layer_forward(m, ws, False, True, uw, B, L, params, w16=w16)
        layer_backward(m, ws, False, B, L, tp, params, dout2, w16=w16)

    with torch.no_grad():
        _, tape = layer_forward(m, ws, False, True, uw, B, L, params)
    tape_bytes = sum(t.numel() * t.element_size() for t in tape)
    return {
        "conv_fwd": lambda: conv_f(xz[:, :D], cw, cb, B, L),
        "conv_bwd": lambda: conv_b(xz[:, :D], cw, cb, dy, dxz[:, :D], B, L, ws),
        "scan_fwd": lambda: scan_f(xc, draw, bdt, A_log, Bm, Cm, Dp, z, B, L, ws, save=True),
        "scan_bwd": lambda: scan_b(xc, draw, bdt, A_log, Bm, Cm, Dp, z, dy, saved, du, dd, dxdbl[:, r:r + 16],
                                   dxdbl[:, r + 16:], dxz[:, D:], B, L, ws),
        "proj": proj, "layer_fwd": layer_fwd, "layer_fwd_bwd": layer_fwd_bwd, "walk_fwd_bwd": walk_fwd_bwd,
    }, tape_bytes


def child(d_model, iters):
    import torch
    from deepsense6g_tii_amd import ops
    from deepsense6g_tii_amd.mamba import Mamba
    torch.manual_seed(0)
    m = Mamba(d_model, device=torch.device("cuda:0"))
    dts = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    fns, res = {}, {}
    for s in STORAGES:
        fns[s], tape = _figures(torch, ops, m, dts[s], d_model)
        res[s] = {"tape_bytes": tape}
    for name in FIGS:
        for s in STORAGES:
            for _ in range(5):
                fns[s][name]()
        reps = {s: [] for s in STORAGES}
        for _ in range(3):
            for s in STORAGES:   # alternating: one repeat of each storage in turn
                fn = fns[s][name]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                reps[s].append(e0.elapsed_time(e1) * 1e3 / iters)
        for s in STORAGES:
            res[s][name] = statistics.median(reps[s])
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
            cmd = ["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--child", str(w), "--iters",
                   str(args.iters)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"run {run} d_model {w}: child ended with {p.returncode}; sweep stopped\n{p.stdout[-3000:]}")
                return 1
            table.setdefault(w, []).append(json.loads(line[0][7:]))
    print(f"Mamba layer, B = {B}, L = {L}; microseconds per storage, {args.runs} runs (each the median of 3 x {args.iters} "
          f"calls, the storages alternating); x = fp32 / 16-bit on the run medians")
    runs = range(args.runs)
    print(f"{'d_model':>7s} {'figure':14s} " + " ".join(f"{s + ' r' + str(i):>9s}" for s in STORAGES for i in runs) +
          f" {'spread':>7s} {'x bf16':>7s} {'x f16':>7s}")
    for w in args.widths:
        med = {s: {} for s in STORAGES}
        rows = list(FIGS) + ["rest"]
        for name in rows:
            def val(rec, s):
                if name != "rest":
                    return rec[s][name]
                return rec[s]["layer_fwd_bwd"] - sum(rec[s][k] for k in ("conv_fwd", "conv_bwd", "scan_fwd", "scan_bwd", "proj"))
            ts = {s: [val(rec, s) for rec in table[w]] for s in STORAGES}
            for s in STORAGES:
                med[s][name] = statistics.median(ts[s])
            spread = max((max(t) - min(t)) / abs(min(t)) for t in ts.values()) * 100
            print(f"{w:7d} {name:14s} " + " ".join(f"{t:9.1f}" for s in STORAGES for t in ts[s]) + f" {spread:6.1f}%" +
                  f" {med['fp32'][name] / med['bf16'][name]:7.2f} {med['fp32'][name] / med['f16'][name]:7.2f}")
        tb = {s: table[w][0][s]["tape_bytes"] for s in STORAGES}
        print(f"{w:7d} {'tape MiB':14s} " + " ".join(f"{tb[s] / 2 ** 20:9.1f}" for s in STORAGES for _ in runs) +
              f" {'':7s} {tb['fp32'] / tb['bf16']:7.2f} {tb['fp32'] / tb['f16']:7.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
