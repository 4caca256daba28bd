"""GPU-side input pipeline: the per-sample work of CARLA_Data.__getitem__ (/root/reference/data2_seq.py:42-173)
plus the DataLoader collate and the dtype casts of Engine.train (train2_seq.py:111-116), done ON the device for a
whole batch.  What stays on the host is file I/O and decoding (JPEG, .ply, .npy), exactly
the part the reference's 8 loader workers (train2_seq.py:531) spend on libraries; everything after the decode runs as
HIP kernels of libds6g.so (csrc/input.hip) and lands directly in the NHWC x4 layout the stem convolutions read, so
the model skips its own pack pass (`TransFuser.forward(PackedInputs)`).  The radar may arrive as raw cubes: `radar_maps` and
`pack` compute the reference's offline range-angle / range-velocity maps (Data_Preprocessing/Radar_data_preprocessing.py:7-23)
on the device (csrc/radar.hip).

Not covered (host, once per dataset, needs the `utm` package the image lacks): the GPS normalisation of
`Normalize_loc` (data2_seq.py:224-290); pass its (B, 2, 2) result in as `gps`.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from ._lib import lib

F32 = torch.float32
NBINS = 256          # data2_seq.py:181 ("256 x 256 grid")
HIST_CAP = 5         # hist_max_per_pixel, data2_seq.py:184
N_BEAMS = 64


@dataclass
class PackedInputs:
    """Stem-ready batch: each modality is [B*seq_len, H, W, 4] fp32 NHWC (frame t of sample b at row b*seq_len + t;
    unused channels zero; camera frames already ImageNet-normalised)."""
    images: torch.Tensor
    lidars: torch.Tensor
    radars: torch.Tensor
    gps: torch.Tensor
    batch: int
    seq_len: int
    target: torch.Tensor | None = None    # (B, 64) soft beam target
    beamidx: torch.Tensor | None = None   # (B,) int32


def fov_edges(address: str = "", custom_fov: bool = False):
    """(xbins, ybins) of lidar_to_histogram_features, data2_seq.py:185-202 (np.linspace, float64)."""
    x, y = (-50, 0), (-50, 50)
    if custom_fov:
        for key, xr, yr in (("scenario31", (-70, 0), (-25, 14)), ("scenario32", (-60, 0), (-40, 5.5)),
                            ("scenario33", (-50, 0), (-12, 7)), ("scenario34", (-50, 0), (-20, 10))):
            if key in address:
                x, y = xr, yr
                break
    return np.linspace(x[0], x[1], NBINS + 1), np.linspace(y[0], y[1], NBINS + 1)


def _is_complex(a):
    return a.is_complex() if torch.is_tensor(a) else np.iscomplexobj(a)


def _cube_floats(cubes, device):
    """complex (N, A, 256, 128) numpy / torch cubes -> contiguous complex64 on the device, viewed as (N, A, 256, 128, 2) fp32"""
    t = cubes if torch.is_tensor(cubes) else torch.from_numpy(np.ascontiguousarray(cubes))
    assert t.is_complex() and t.dim() == 4, (t.dtype, tuple(t.shape))
    return torch.view_as_real(t.to(device, torch.complex64, non_blocking=True).contiguous())


def radar_maps(cubes, add_velocity=True, flip=False, device=None):
    """The reference's radar preprocessing (Data_Preprocessing/Radar_data_preprocessing.py:7-23,41-42) on the device: raw cubes
    (N, A, 256, 128) complex64 / complex128 (numpy or torch; wider input is rounded to complex64) -> (N, 1 | 2, 256, 256) fp32
    device tensor, channel 0 the min-max normalised range-angle map, channel 1 (add_velocity) the range-velocity map - what
    np.save(path_ang / path_vel) held, stacked (and flipped) as data2_seq.py:142-151 does.  HIP kernels only: a CPU tensor
    without a device, or a CPU device, is refused."""
    dev = torch.device(device) if device is not None else (cubes.device if torch.is_tensor(cubes) else torch.device("cuda"))
    if dev.type != "cuda":
        raise RuntimeError("radar_maps runs HIP kernels only (no CPU path)")
    cube = _cube_floats(cubes, dev)
    N, A = cube.shape[:2]
    R, raw, part = ops.radar_scratch(N, A, dev)
    out = torch.empty((N, 2 if add_velocity else 1, NBINS, NBINS), dtype=F32, device=dev)
    ops.radar_range_fft(cube, R)
    ops.radar_maps_raw(R, raw, part, add_velocity)
    return ops.radar_finish(raw, part, out, 0, add_velocity, flip)


class DeviceInputPipeline:
    """Builds PackedInputs from decoded host arrays.

    images : seq_len arrays / tensors (B, H, W, 3) uint8  - PIL decode + resize output, data2_seq.py:110-141
    clouds : seq_len lists of B arrays (P_i, >=2) float64 - np.asarray(o3d point cloud), data2_seq.py:155
    radars : seq_len arrays (B, C, H, W) float           - range-angle (+ velocity) maps, data2_seq.py:142-154
             or (B, A, 256, 128) complex                 - raw radar cubes (radar_data/*.npy): the maps are computed on the
                                                           device (radar_maps below) and written straight into the batch
    gps    : (B, 2, 2)                                    - Normalize_loc output, data2_seq.py:48
    beam   : (B,) 0-based beam index (csv value - 1, data2_seq.py:162) or None (test split)
    addresses : B strings deciding the custom LiDAR field of view (data2_seq.py:190-202); ignored unless custom_fov.
    flip   : the horizontal-flip augmentation (data2_seq.py:49-50,144-146,157-158,168-170) applied to the whole batch
    add_velocity : with raw radar cubes, also compute the range-velocity map (channel 1), data2_seq.py:148-154
    """

    def __init__(self, device, seq_len=5, custom_fov=False, flip=False, add_velocity=True):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceInputPipeline runs HIP kernels only (no CPU path)")
        self.seq_len = seq_len
        self.custom_fov = custom_fov
        self.flip = flip
        self.add_velocity = add_velocity
        self._counts = None
        self._radar_scratch = None

    def _dev(self, a, dtype):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(self.device, dtype, non_blocking=True).contiguous()

    def pack(self, images, clouds, radars, gps, beam=None, addresses=None) -> PackedInputs:
        L, st, S = lib(), ops._stream(), self.seq_len
        assert len(images) == S and len(clouds) == S and len(radars) == S
        B, H, W, _ = images[0].shape
        flip = int(self.flip)
        img = torch.empty((B * S, H, W, 4), dtype=F32, device=self.device)
        lid = torch.empty((B * S, NBINS, NBINS, 4), dtype=F32, device=self.device)
        rad = torch.empty((B * S, H, W, 4), dtype=F32, device=self.device)
        if self._counts is None or self._counts.shape[0] != B:
            self._counts = torch.zeros((B, NBINS, NBINS), dtype=torch.int32, device=self.device)
        # per-cloud bin edges (mixed scenarios in one batch are allowed)
        if addresses is None:
            addresses = [""] * B
        edges = [fov_edges(a, self.custom_fov) for a in addresses]
        xe = self._dev(np.stack([e[0] for e in edges]), torch.float64)
        ye = self._dev(np.stack([e[1] for e in edges]), torch.float64)
        for t in range(S):
            u8 = self._dev(images[t], torch.uint8)
            assert u8.shape == (B, H, W, 3), u8.shape
            L.pack_image_u8(u8.data_ptr(), img.data_ptr(), B, H, W, S, t, flip, st)
            pts = [np.asarray(c, dtype=np.float64).reshape(-1, np.asarray(c).shape[-1]) for c in clouds[t]]
            assert len(pts) == B
            stride = pts[0].shape[1]
            offs = np.zeros(B + 1, dtype=np.int64)
            offs[1:] = np.cumsum([p.shape[0] for p in pts])
            allp = self._dev(np.concatenate(pts, 0) if offs[-1] else np.zeros((1, stride)), torch.float64)
            offd = self._dev(offs, torch.int64)
            L.lidar_bev_count(allp.data_ptr(), stride, offd.data_ptr(), B, int(offs[-1]), xe.data_ptr(), ye.data_ptr(), 1,
                              NBINS, self._counts.data_ptr(), st)
            L.lidar_bev_finish(self._counts.data_ptr(), lid.data_ptr(), B, NBINS, 4, S, t, flip, HIST_CAP, st)
            if _is_complex(radars[t]):
                assert (H, W) == (NBINS, NBINS), (H, W)
                cube = _cube_floats(radars[t], self.device)
                assert cube.shape[0] == B, (tuple(cube.shape), B)
                if self._radar_scratch is None or self._radar_scratch[0].shape[:2] != cube.shape[:2]:
                    self._radar_scratch = ops.radar_scratch(B, cube.shape[1], self.device)
                R, raw, part = self._radar_scratch
                ops.radar_range_fft(cube, R)
                ops.radar_maps_raw(R, raw, part, self.add_velocity)
                ops.radar_finish(raw, part, rad, t, self.add_velocity, flip)
                continue
            r = self._dev(radars[t], F32)
            if flip:
                r = torch.flip(r, dims=(3,)).contiguous()  # np.flip(radar, 1) on the (H, W) map, data2_seq.py:145,152
            Cr = r.shape[1]
            assert r.shape == (B, Cr, H, W) and Cr <= 4
            L.pack_input(r.data_ptr(), rad.data_ptr(), B, Cr, H, W, 4, S, t, 0, st)
        g = self._dev(gps, F32).clone()
        assert g.shape == (B, 2, 2)
        if flip:
            g[:, :, 1] = -g[:, :, 1]  # data2_seq.py:49-50
        target = idx = None
        if beam is not None:
            bi = self._dev(np.asarray(beam, dtype=np.int32) if not torch.is_tensor(beam) else beam, torch.int32)
            target = torch.empty((B, N_BEAMS), dtype=F32, device=self.device)
            idx = torch.empty((B,), dtype=torch.int32, device=self.device)
            L.soft_beam_target(bi.data_ptr(), target.data_ptr(), idx.data_ptr(), B, N_BEAMS, flip, st)
        return PackedInputs(img, lid, rad, g, B, S, target, idx)
