"""GPU: csrc/radar.hip (raw radar cube -> normalised range-angle / range-velocity maps) against the host reference
tests/radar_ref.py in double precision and against the reference's own outputs (tests/golden/radar_golden.npz).

The bar of every comparison is 10 x e32 per map kind, e32 = max |maps(complex64) - maps(complex128)| of the host path on the
same cubes (about 1.4e-7 for ang, 1e-7 for vel): the project's usual margin for a different summation order over the error of
the fp32 host path itself.  There is no absolute floor - the velocity map's median is about 1e-4."""
import os

import numpy as np
import pytest
import torch

from tests import moat
from tests import radar_ref as rr

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "radar_golden.npz")
KINDS = ("ang", "vel")
_CACHE = {}


def seeded():
    """-> (cubes (3, 4, 256, 128) complex64, truth (3, 2, 256, 256) float64, e32 [ang, vel]), computed once"""
    if "seeded" not in _CACHE:
        cubes = np.stack([rr.cube(sd) for sd in (0, 1, 2)])
        truth = np.stack([rr.maps(c, np.complex128) for c in cubes])
        single = np.stack([rr.maps(c, np.complex64) for c in cubes])
        assert single.dtype == np.float32
        e32 = [float(np.abs(single[:, j].astype(np.float64) - truth[:, j]).max()) for j in range(2)]
        truth.setflags(write=False)
        _CACHE["seeded"] = (cubes, truth, e32)
    return _CACHE["seeded"]


def device_maps(dev, cubes, **kw):
    from deepsense6g_tii_amd import data
    out = data.radar_maps(cubes, device=dev, **kw)
    torch.cuda.synchronize()
    return out


def test_parity_with_double_precision_host_maps(dev):
    cubes, truth, e32 = seeded()
    got = device_maps(dev, cubes)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 2, 256, 256) and got.is_contiguous()
    got = got.cpu().numpy()
    for j, name in enumerate(KINDS):
        err = float(np.abs(got[:, j].astype(np.float64) - truth[:, j]).max())
        print(f"radar parity {name}: max abs err {err:.3e}, e32 {e32[j]:.3e}, ratio {err / e32[j]:.2f} (bar 10)")
        assert 0.5e-7 < e32[j] < 3e-7, (name, e32[j])       # the bar itself is where the host path's error has been measured
        assert err <= 10 * e32[j], (name, err, e32[j])
        for n in range(3):
            assert got[n, j].min() == 0.0 and got[n, j].max() == 1.0, (n, name)
    # the angle map alone (add_velocity=False) is the same map, bit for bit
    ang = device_maps(dev, cubes, add_velocity=False)
    assert tuple(ang.shape) == (3, 1, 256, 256) and np.array_equal(ang.cpu().numpy()[:, 0], got[:, 0])


def test_parity_other_antenna_counts(dev):
    """A = 1, 3 and 8: the other instantiations of the per-row kernel (A = 8 fills its LDS budget)"""
    _, _, e32 = seeded()
    for A in (1, 3, 8):
        c = rr.cube(10 + A, antennas=A)
        want = rr.maps(c, np.complex128)
        got = device_maps(dev, c[None]).cpu().numpy()[0]
        for j, name in enumerate(KINDS):
            err = float(np.abs(got[j].astype(np.float64) - want[j]).max())
            print(f"radar parity A={A} {name}: max abs err {err:.3e}, ratio {err / e32[j]:.2f} (bar 10)")
            assert err <= 10 * e32[j], (A, name, err)


def test_reference_fixture(dev):
    from tests.test_radar_cpu import fixture_cubes
    g = np.load(GOLD)
    cubes = fixture_cubes()
    got = device_maps(dev, np.stack(list(cubes.values()))).cpu().numpy().astype(np.float64)
    for i, key in enumerate(cubes):
        for j, name in enumerate(KINDS):
            bar = 10 * float(g[f"e32_{name}"])
            smp, rows, cols = rr.sample(got[i, j])
            errs = (np.abs(smp - g[f"{key}_{name}_sample"]).max(), np.abs(rows - g[f"{key}_{name}_rows"]).max(),
                    np.abs(cols - g[f"{key}_{name}_cols"]).max())
            print(f"radar fixture {key} {name}: sample {errs[0]:.3e} rows {errs[1]:.3e} cols {errs[2]:.3e} (bar {bar:.3e}, x256 for sums)")
            assert errs[0] <= bar and errs[1] <= bar * 256 and errs[2] <= bar * 256, (key, name, errs)


def test_tone_probes(dev):
    _, _, e32 = seeded()
    got = device_maps(dev, np.stack([rr.tone(*t) for t in rr.TONES])).cpu().numpy()
    for i, (t, peaks) in enumerate(zip(rr.TONES, rr.TONE_PEAKS)):
        for j, name in enumerate(KINDS):
            m = got[i, j]
            assert np.unravel_index(m.argmax(), m.shape) == peaks[j], (t, name, np.unravel_index(m.argmax(), m.shape))
            off = float(np.delete(m, t[0], axis=0).max())
            print(f"radar tone {t} {name}: off-row max {off:.3e} (bar {10 * e32[j]:.3e})")
            assert off <= 10 * e32[j], (t, name, off)


def _batch(B, S, seed):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, (B, 256, 256, 3), dtype=np.uint8) for _ in range(S)]
    clouds = [[rng.uniform(-50, 0, (500, 3)) for _ in range(B)] for _ in range(S)]
    gps = rng.uniform(-1.5, 1.5, (B, 2, 2))
    return images, clouds, gps


@pytest.mark.parametrize("flip,vel", [(False, True), (True, True), (False, False), (True, False)])
def test_pack_takes_cubes(dev, flip, vel):
    from deepsense6g_tii_amd import data
    B, S = 2, 2
    cubes, _, _ = seeded()
    images, clouds, gps = _batch(B, S, 3)
    radars = [cubes[0:2], np.stack([cubes[2], cubes[0]]).astype(np.complex128)]     # wider input is rounded to complex64
    pipe = data.DeviceInputPipeline(dev, seq_len=S, flip=flip, add_velocity=vel)
    pk = pipe.pack(images, clouds, radars, gps)
    # the float maps of radar_maps are flipped by pack itself
    maps = [data.radar_maps(r, add_velocity=vel, device=dev) for r in radars]
    pk2 = data.DeviceInputPipeline(dev, seq_len=S, flip=flip).pack(images, clouds, maps, gps)
    torch.cuda.synchronize()
    assert torch.equal(moat.bits(pk.radars), moat.bits(pk2.radars))
    assert torch.equal(moat.bits(pk.images), moat.bits(pk2.images)) and torch.equal(moat.bits(pk.lidars), moat.bits(pk2.lidars))
    rad = pk.radars.cpu().numpy().reshape(B, S, 256, 256, 4)
    nch = 2 if vel else 1
    assert not rad[..., nch:].any() and np.isfinite(rad).all()
    for t in range(S):
        m = data.radar_maps(radars[t], add_velocity=vel, flip=flip, device=dev).cpu().numpy()
        plain = maps[t].cpu().numpy()
        assert np.array_equal(m, plain[..., ::-1] if flip else plain)
        for b in range(B):
            assert np.array_equal(rad[b, t, :, :, :nch], m[b].transpose(1, 2, 0)), (b, t)
    # the cached scratch is reused by a second call, with the same result
    pk3 = pipe.pack(images, clouds, radars, gps)
    assert torch.equal(moat.bits(pk3.radars), moat.bits(pk.radars))


def test_entry_points_inside_moats(dev):
    """the three launches with dst and all scratch embedded in guard regions: no guard word changes, and no value of a
    NaN moat or of a poisoned payload reaches an output"""
    from deepsense6g_tii_amd import ops
    cubes, truth, e32 = seeded()
    N, A, S, t = 2, 4, 2, 1
    M = moat.MIN_MOAT
    cube, gc = moat.embed(torch.view_as_real(torch.from_numpy(cubes[:N].copy())).contiguous().to(dev), M, M, "nan", "cube")
    R0, raw0, part0 = ops.radar_scratch(N, A, dev)
    R, gR = moat.embed(moat.nan_like(R0), M, M, "nan", "R")
    raw, graw = moat.embed(moat.nan_like(raw0), M, M, "nan", "raw")
    part, gpart = moat.embed(moat.nan_like(part0), M, M, "nan", "part")
    dst, gdst = moat.embed(moat.nan_like(torch.empty((N * S, 256, 256, 4), device=dev)), M, M, 0xFF, "dst")
    pl, gpl = moat.embed(moat.nan_like(torch.empty((N, 2, 256, 256), device=dev)), M, M, 0xFF, "planar dst")
    ops.radar_range_fft(cube, R)
    ops.radar_maps_raw(R, raw, part, True)
    ops.radar_finish(raw, part, dst, t, True, False)
    ops.radar_finish(raw, part, pl, 0, True, True)
    torch.cuda.synchronize()
    for g in (gc, gR, graw, gpart, gdst, gpl):
        g()
    for x in (R, raw, part, pl):
        assert bool(torch.isfinite(x).all())
    d = dst.view(N, S, 256, 256, 4)
    assert bool(torch.isnan(d[:, 0]).all())                       # the other time step's rows are untouched
    got = d[:, t].cpu().numpy()
    assert not got[..., 2:].any()
    for j in range(2):
        assert np.abs(got[..., j].astype(np.float64) - truth[:N, j]).max() <= 10 * e32[j]
    assert np.array_equal(pl.cpu().numpy()[..., ::-1], got[..., :2].transpose(0, 3, 1, 2))
    # the angle map alone: plane 1 of raw, its partials and channel 1 are not written
    raw.fill_(float("nan")); part.fill_(float("nan")); dst.fill_(float("nan"))
    ops.radar_maps_raw(R, raw, part, False)
    ops.radar_finish(raw, part, dst, t, False, False)
    torch.cuda.synchronize()
    for g in (gR, graw, gpart, gdst):
        g()
    assert bool(torch.isnan(raw[:, 1]).all()) and bool(torch.isnan(part[:, :, 1]).all())
    got1 = dst.view(N, S, 256, 256, 4)[:, t].cpu().numpy()
    assert np.array_equal(got1[..., 0], got[..., 0]) and not got1[..., 1:].any()


def test_determinism_and_frame_independence(dev):
    cubes, _, _ = seeded()
    batch = np.stack([cubes[0], np.zeros_like(cubes[0]), cubes[1]])
    a = device_maps(dev, batch)
    b = device_maps(dev, batch)
    assert torch.equal(moat.bits(a), moat.bits(b))
    assert bool(torch.isnan(a[1]).all()) and bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[2]).all())
    full = device_maps(dev, cubes)
    alone = device_maps(dev, cubes[1:2])
    assert torch.equal(moat.bits(full[1:2]), moat.bits(alone))
    assert torch.equal(moat.bits(a[2]), moat.bits(full[1])) and torch.equal(moat.bits(a[0]), moat.bits(full[0]))
