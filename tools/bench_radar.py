"""Times the device radar-map path (csrc/radar.hip) for one batch of raw radar cubes against the host path it replaces.

    python tools/bench_radar.py [--frames 60] [--steps 50] [--rounds 3] [--host-frames 60] [--out FILE]

Device: the three launches (range FFT, raw maps, finish) one by one and together, and the host-to-device copy of the cubes,
each the median over `rounds` rounds of `steps` calls between two device events after a warm-up.  Host: tests/radar_ref.py
maps() in complex128 and complex64 (scipy.fft, one thread, as the reference's numpy functions) for the same frames.
Fails without a GPU.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from deepsense6g_tii_amd import data, ops
from tests import radar_ref as rr


def timed(fn, steps, rounds):
    """-> per-call ms of each round: `steps` calls of fn between two device events"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-frames", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_radar.py needs a GPU")
    dev = torch.device("cuda:0")
    N, A = args.frames, rr.A
    base = [rr.cube(sd) for sd in range(4)]
    cubes = np.stack([base[i % 4] for i in range(N)])          # 1 MB per frame
    host = torch.from_numpy(cubes).pin_memory()
    cube = torch.view_as_real(host.to(dev)).contiguous()
    R, raw, part = ops.radar_scratch(N, A, dev)
    dst = torch.empty((N, 256, 256, 4), dtype=torch.float32, device=dev)
    staging = torch.empty_like(host, device=dev)
    rows = [("range_fft", lambda: ops.radar_range_fft(cube, R)),
            ("maps_raw", lambda: ops.radar_maps_raw(R, raw, part, True)),
            ("maps_raw, angle only", lambda: ops.radar_maps_raw(R, raw, part, False)),
            ("finish", lambda: ops.radar_finish(raw, part, dst, 0, True, False)),
            ("the three launches", lambda: (ops.radar_range_fft(cube, R), ops.radar_maps_raw(R, raw, part, True),
                                            ops.radar_finish(raw, part, dst, 0, True, False))),
            ("H2D copy, pinned", lambda: staging.copy_(host, non_blocking=True)),
            ("data.radar_maps, pinned host cubes", lambda: data.radar_maps(host, device=dev))]
    lines = [f"radar maps, {N} frames of ({A}, 256, 128) complex64 = {cubes.nbytes / 1e6:.1f} MB, one MI355X; per call, "
             f"{args.rounds} rounds of {args.steps} calls between device events after 3 warm-up calls",
             f"  {'what':<38}{'median ms':>10}{'min':>9}{'max':>9}{'us / frame':>12}"]
    for name, fn in rows:
        ms = timed(fn, args.steps, args.rounds)
        med = statistics.median(ms)
        lines.append(f"  {name:<38}{med:>10.3f}{min(ms):>9.3f}{max(ms):>9.3f}{med * 1e3 / N:>12.2f}")
    torch.cuda.synchronize()
    torch.set_num_threads(1)
    H = min(args.host_frames, N)
    for prec in (np.complex128, np.complex64):
        t0 = time.perf_counter()
        for i in range(H):
            rr.maps(cubes[i], prec)
        dt = time.perf_counter() - t0
        lines.append(f"  host radar_ref.maps {np.dtype(prec).name:<18}{dt * 1e3:>10.0f}{'':>18}{dt * 1e6 / H:>12.0f}   ({H} frames, one thread)")
    got = data.radar_maps(cubes[:4], device=dev).cpu().numpy().astype(np.float64)
    want = np.stack([rr.maps(c) for c in cubes[:4]])
    lines.append(f"  max |device - host complex128| on the first 4 frames: ang {np.abs(got[:, 0] - want[:, 0]).max():.3e}, "
                 f"vel {np.abs(got[:, 1] - want[:, 1]).max():.3e}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
