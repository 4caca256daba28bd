"""CPU: the radar-map host reference (tests/radar_ref.py) against the reference's own functions (tests/golden/radar_golden.npz,
made by tests/golden/make_golden_radar.py), the three radar prototypes of the C ABI, and the host-side refusals of
csrc/radar.hip - every one of them returns before any launch, so they run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import radar_ref as rr

GOLD = os.path.join(os.path.dirname(__file__), "golden", "radar_golden.npz")
ENTRIES = ("ds6g_radar_range_fft", "ds6g_radar_maps_raw", "ds6g_radar_finish")


def fixture_cubes():
    out = {f"seed{sd}": rr.cube(sd) for sd in (0, 1)}
    out.update({f"tone{i}": rr.tone(*t) for i, t in enumerate(rr.TONES)})
    return out


def test_host_reference_matches_reference_golden():
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < 200 << 10
    assert 1e-7 < float(g["e32_ang"]) < 2e-7 and 0.5e-7 < float(g["e32_vel"]) < 2e-7
    for key, c in fixture_cubes().items():
        assert c.shape == (4, 256, 128) and c.dtype == np.complex64
        got = rr.maps(c, np.complex128)
        assert got.dtype == np.float64 and got.shape == (2, 256, 256)
        for j, name in enumerate(("ang", "vel")):
            smp, rows, cols = rr.sample(got[j])
            assert np.abs(smp - g[f"{key}_{name}_sample"]).max() <= 1e-12, (key, name)
            assert np.abs(rows - g[f"{key}_{name}_rows"]).max() <= 1e-12 * 256, (key, name)
            assert np.abs(cols - g[f"{key}_{name}_cols"]).max() <= 1e-12 * 256, (key, name)
            assert got[j].min() == 0.0 and got[j].max() == 1.0


def test_host_reference_single_precision_and_tone_peaks():
    s = rr.maps(rr.cube(0), np.complex64)
    assert s.dtype == np.float32                      # scipy.fft keeps complex64 under every numpy version
    for t, (pa, pv) in zip(rr.TONES, rr.TONE_PEAKS):
        m = rr.maps(rr.tone(*t))
        assert np.unravel_index(m[0].argmax(), m[0].shape) == pa and np.unravel_index(m[1].argmax(), m[1].shape) == pv
    with np.errstate(invalid="ignore"):
        assert np.isnan(rr.maps(np.zeros((4, 256, 128), np.complex64))).all()    # max == min: 0 / 0, as in numpy


def test_prototypes():
    from deepsense6g_tii_amd import _lib
    from tests import perturb
    protos = _lib.parse_header()
    names = perturb.stream_entry_points()
    L = _lib.lib()
    for name in ENTRIES:
        assert name in protos and hasattr(L._dll, name) and callable(getattr(L, name[len("ds6g_"):])), name
        ret, args = protos[name]
        assert ret is ctypes.c_int and args[-1] is ctypes.c_void_p and name[len("ds6g_"):] in names, name
        assert not re.search(r"_(bytes|floats)$", name)
    assert [n for n in protos if "radar" in n] == list(ENTRIES)
    assert protos["ds6g_radar_range_fft"][1].count(ctypes.c_long) == 2
    assert protos["ds6g_radar_maps_raw"][1].count(ctypes.c_long) == 3
    assert protos["ds6g_radar_finish"][1].count(ctypes.c_long) == 3


def test_host_refusals():
    """NULL pointers, an antenna count of 0 or 9, a cube of 128 samples and short buffers are refused on the host.  The
    pointers are never dereferenced: they only have to be non-NULL and 16-byte aligned."""
    from deepsense6g_tii_amd._lib import Ds6gError, lib
    L = lib()
    P, N, A = 1 << 20, 2, 4
    cube, raw, part, dst = N * A * 256 * 128 * 2, N * 2 * 256 * 256, N * 256 * 4, N * 256 * 256 * 4
    bad_fft = [(0, cube, P, cube, N, A, 256, 128), (P, cube, 0, cube, N, A, 256, 128), (P, cube, P, cube, N, 0, 256, 128),
               (P, cube * 3, P, cube * 3, N, 9, 256, 128), (P, cube, P, cube, N, A, 128, 128), (P, cube, P, cube, N, A, 256, 256),
               (P, cube, P, cube, 0, A, 256, 128), (P, cube - 1, P, cube, N, A, 256, 128), (P, cube, P, cube - 1, N, A, 256, 128),
               (P + 8, cube, P, cube, N, A, 256, 128)]
    for a in bad_fft:
        with pytest.raises(Ds6gError):
            L.radar_range_fft(*a, 0)
    bad_raw = [(0, cube, P, raw, P, part, N, A, 256, 128, 2), (P, cube, 0, raw, P, part, N, A, 256, 128, 2),
               (P, cube, P, raw, 0, part, N, A, 256, 128, 2), (P, cube, P, raw, P, part, N, 0, 256, 128, 2),
               (P, cube * 3, P, raw, P, part, N, 9, 256, 128, 2), (P, cube, P, raw, P, part, N, A, 128, 128, 2),
               (P, cube, P, raw, P, part, N, A, 256, 128, 3), (P, cube, P, raw, P, part, N, A, 256, 128, 0),
               (P, cube - 1, P, raw, P, part, N, A, 256, 128, 2), (P, cube, P, raw - 1, P, part, N, A, 256, 128, 2),
               (P, cube, P, raw, P, part - 1, N, A, 256, 128, 1)]
    for a in bad_raw:
        with pytest.raises(Ds6gError):
            L.radar_maps_raw(*a, 0)
    #          raw raw_elems part part_elems dst dst_elems N nch Cd frames_per_sample t flip planar
    bad_fin = [(0, raw, P, part, P, dst, N, 2, 4, 1, 0, 0, 0), (P, raw, 0, part, P, dst, N, 2, 4, 1, 0, 0, 0),
               (P, raw, P, part, 0, dst, N, 2, 4, 1, 0, 0, 0), (P, raw, P, part, P, dst, N, 3, 4, 1, 0, 0, 0),
               (P, raw, P, part, P, dst, N, 2, 1, 1, 0, 0, 0), (P, raw, P, part, P, dst, N, 2, 4, 1, 1, 0, 0),
               (P, raw, P, part, P, dst, N, 2, 4, 1, -1, 0, 0), (P, raw, P, part, P, dst, N, 2, 4, 1, 0, 0, 1),
               (P, raw, P, part, P, dst, N, 2, 2, 2, 0, 0, 1), (P, raw - 1, P, part, P, dst, N, 2, 4, 1, 0, 0, 0),
               (P, raw, P, part - 1, P, dst, N, 2, 4, 1, 0, 0, 0), (P, raw, P, part, P, dst - 1, N, 2, 4, 1, 0, 0, 0),
               (P, raw, P, part, P, dst, N, 2, 4, 2, 1, 0, 0), (P, raw, P, part, P + 4, dst, N, 2, 4, 1, 0, 0, 0)]
    for a in bad_fin:
        with pytest.raises(Ds6gError):
            L.radar_finish(*a, 0)


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from deepsense6g_tii_amd import data, ops
    cubes = np.zeros((1, 4, 256, 128), np.complex64)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        data.radar_maps(torch.from_numpy(cubes))
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        data.radar_maps(cubes, device="cpu")
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        data.DeviceInputPipeline("cpu")
    f = torch.zeros((1, 4, 256, 128, 2))
    with pytest.raises(AssertionError):     # a CPU tensor never reaches the library
        ops.radar_range_fft(f, torch.empty_like(f))
    with pytest.raises(AssertionError):
        ops.radar_maps_raw(f, torch.empty((1, 2, 256, 256)), torch.empty((1, 256, 2, 2)))
    with pytest.raises(AssertionError):
        ops.radar_finish(torch.empty((1, 2, 256, 256)), torch.empty((1, 256, 2, 2)), torch.empty((1, 2, 256, 256)))
