"""Host reference of the radar maps (Data_Preprocessing/Radar_data_preprocessing.py:7-23,41-42 of the reference, restated)
and the seeded synthetic cubes the radar tests share.

    R[a, r, k]  = sum_s x[a, s, k] exp(-2 pi i r s / 256)                                range FFT
    m[a, r]     = mean_k R[a, r, k]
    ang[r, th]  = sum_k | sum_a (R[a, r, k] - m[a, r]) exp(-2 pi i th a / 256) |          angle FFT, A -> 256 zero-padded
    vel[r, v]   = sum_a | sum_k  R[a, r, k]            exp(-2 pi i v k / 256) |           Doppler FFT, 128 -> 256 zero-padded
    map         = (map - min) / (max - min)

scipy.fft keeps single precision for complex64 input under every numpy version (np.fft does so only under numpy >= 2), so
maps(cube, np.complex64) is the fp32 host path whose error against maps(cube, np.complex128) sets the tests' bar.

No fixtures here: the tests import this module.
"""
import numpy as np
import scipy.fft

A, S, K, BINS = 4, 256, 128, 256


def cube(seed, ntg=6, antennas=A, clutter=True):
    """(antennas, 256, 128) complex64 of integer ADC counts: `ntg` moving point targets, four static clutter returns,
    complex Gaussian noise"""
    rng = np.random.default_rng(seed)
    a = np.arange(antennas)[:, None, None]
    s = np.arange(S)[None, :, None]
    k = np.arange(K)[None, None, :]
    x = np.zeros((antennas, S, K), np.complex128)
    for _ in range(ntg):
        amp, fr, fd, fa = rng.uniform(200, 2000), rng.uniform(2, 120), rng.uniform(-40, 40), rng.uniform(-0.5, 0.5)
        x += amp * np.exp(2j * np.pi * (fr * s / S + fd * k / K + fa * a + rng.uniform()))
    if clutter:
        for _ in range(4):
            amp, fr, fa = rng.uniform(1000, 5000), rng.uniform(1, 60), rng.uniform(-0.5, 0.5)
            x += amp * np.exp(2j * np.pi * (fr * s / S + fa * a + rng.uniform()))
    x += 50 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    x = np.round(x.real) + 1j * np.round(x.imag)
    return x.astype(np.complex64)


def tone(r0, d0, t0, amp=1000.0, antennas=A):
    """one complex tone amp * exp(+2 pi i (r0 s / 256 + d0 k / 128 + t0 a / 256)): peaks at ang[r0, t0] and vel[r0, 2 d0]"""
    a = np.arange(antennas)[:, None, None]
    s = np.arange(S)[None, :, None]
    k = np.arange(K)[None, None, :]
    return (amp * np.exp(2j * np.pi * (r0 * s / S + d0 * k / K + t0 * a / 256))).astype(np.complex64)


TONES = ((37, 11, 200), (37, 117, 56))          # (range bin, Doppler cycles per frame, angle bin); the second mirrors the first
TONE_PEAKS = (((37, 200), (37, 22)), ((37, 56), (37, 234)))   # argmax of (ang, vel) per tone


def minmax(m):
    return (m - m.min()) / (m.max() - m.min())


def raw_maps(x, precision=np.complex128):
    """-> (ang, vel) before normalisation, [range][angle] and [range][velocity], real dtype of `precision`"""
    x = np.asarray(x).astype(precision)
    R = scipy.fft.fft(x, axis=1)
    assert R.dtype == precision
    d = R - R.mean(axis=2, keepdims=True)
    ang = np.abs(scipy.fft.fft(d, BINS, axis=0)).sum(axis=2).T
    vel = np.abs(scipy.fft.fft(R, BINS, axis=2)).sum(axis=0)
    return ang, vel


def maps(x, precision=np.complex128):
    """-> (2, 256, 256): the normalised range-angle and range-velocity maps of one cube"""
    with np.errstate(invalid="ignore"):
        return np.stack([minmax(m) for m in raw_maps(x, precision)])


def sample(m):
    """what the fixture stores of one (256, 256) map: every 61st element, the row sums and the column sums"""
    return m.reshape(-1)[::61].copy(), m.sum(axis=1), m.sum(axis=0)
