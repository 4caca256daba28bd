"""Frozen inference engine: ``TransFuser.freeze_inference(storage)`` -> :class:`InferenceEngine`.

``model.eval()`` folds every eval-mode BatchNorm into its convolution and transforms the Winograd filters again on EVERY
forward (the weights of a model in training change between calls), and it always runs the fp32-storage kernels.  A deployed
model's weights do not change, so the engine does that work ONCE, into memory it owns, in the storage type asked for:

  storage   convolutions                                               GPT / head
  "f32"     BN-folded fp32 filter + bias of every conv; the            fp32 copies
            Winograd-transformed filter u of every 3x3 / stride-1 conv
  "bf16",   BN folded in fp32, rounded once to the 16-bit type          16-bit copies of the key|query|value, proj, fc1, fc2
  "f16"     (ds6g_bn_fold_h16); fp32 bias; the stem filter             weights; biases, LayerNorm, pos_emb, vel_emb*, join
            also in the stem kernel's packed layout                     (and decoder / output of the 30->5 head) fp32

The engine is a SNAPSHOT: between ``refresh()`` calls it never reads the model's parameters or buffers, so the model may go
on training, be re-pointed by an EMA shadow or be reloaded.  ``refresh()`` writes the new snapshot into the SAME device
buffers, so a HIP graph captured by ``capture()`` sees it.  (``TransFuser.capture_inference`` is the opposite contract: a
graph that follows the live weights.)

The forward itself is the model's own walk (``TransFuser._run_forward_walk``) under a ``_Walk`` the engine builds from
its own pointer tables, folded convs and storage type; it writes nothing on the model.  It does borrow the model's scratch
workspaces and trunk streams, so calls on one model and its engines must come from one thread, as for the model itself.  The snapshot tables are keyed by the model's Parameter objects: re-pointing
``param.data`` (EMA, load_state_dict, optimizer steps) is what refresh() follows; a model whose Parameter OBJECTS were
replaced after the freeze is a different model - refresh() refuses it, freeze it again.
"""
from __future__ import annotations

import re

import torch

from . import ops
from ._lib import lib
from .model import _Folded, _live_ptr, _table, _Walk, capture_forward

F32 = torch.float32
_STORAGE = {"f32": F32, "bf16": torch.bfloat16, "f16": torch.float16}
_TRUNKS = ("encoder.image_encoder.", "encoder.lidar_encoder.", "encoder.radar_encoder.")
# the GEMM operands of the GPT blocks: stored in the engine's 16-bit type under "bf16" / "f16"
_GEMM_WEIGHT = re.compile(r"\.attn\.(key|query|value|proj)\.weight$|\.mlp\.[02]\.weight$")


class InferenceEngine:
    """See the module docstring.  ``engine(image_list, lidar_list, radar_list, gps)`` takes what ``TransFuser.forward`` takes
    (``data.PackedInputs`` included) and returns fp32 logits; it records no tape and touches no ``requires_grad``."""

    def __init__(self, model, storage="f32"):
        if storage not in _STORAGE:
            raise ValueError(f"storage must be one of {sorted(_STORAGE)}, got {storage!r}")
        if model.device.type != "cuda":
            raise RuntimeError("deepsense6g_tii_amd.TransFuser runs on MI355X HIP kernels only (no CPU path)")
        self.model = model
        self.storage = storage
        self.dtype = _STORAGE[storage]
        self._allocate()
        self.refresh()

    # ---------------------------------------------------------------- snapshot ------------------
    def _allocate(self):
        """device buffers of the snapshot (allocated once: refresh() writes into them) and the walk that reads them"""
        self._allocate_params()
        self._allocate_folds()
        self._walk = self._make_walk()

    def _placement(self, name):
        """where the snapshot keeps the non-trunk parameter `name`: True - the 16-bit flat buffer (a GEMM operand on 16-bit
        storage), False - the fp32 one, None - the engine snapshots it in a buffer of its own layout (a subclass does)"""
        return self.dtype != F32 and _GEMM_WEIGHT.search(name) is not None

    def _allocate_params(self):
        m, dev, h16 = self.model, self.model.device, self.dtype != F32
        named = [(n, p) for n, p in m.arena_layout()[0] if not n.startswith(_TRUNKS)]   # arena order: k|q|v stay adjacent
        place = {n: self._placement(n) for n, _ in named}
        self._own_ids = {id(p) for n, p in named if place[n] is None}
        named = [(n, p) for n, p in named if place[n] is not None]
        pad4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
        in16 = lambda n: place[n]  # noqa: E731
        self._flat32 = torch.zeros(sum(pad4(p.numel()) for n, p in named if not in16(n)), dtype=F32, device=dev)
        self._flat16 = torch.zeros(sum(pad4(p.numel()) for n, p in named if in16(n)), dtype=self.dtype if h16 else F32,
                                   device=dev)
        self.wtable, self.wtable16, self._copies = {}, {}, []
        self._trunk_ids = {id(p) for n, p in m.arena_layout()[0] if n.startswith(_TRUNKS)}
        off = {False: 0, True: 0}
        for n, p in named:
            k = in16(n)
            flat = self._flat16 if k else self._flat32
            seg = flat[off[k]:off[k] + p.numel()]
            off[k] += pad4(p.numel())
            (self.wtable16 if k else self.wtable)[id(p)] = seg.data_ptr()
            self._copies.append((p, seg))

    def _allocate_folds(self):
        # every BatchNorm-followed conv: (conv, bn, K, taps, cin, cpad) -> folded filter w, bias b, Winograd filter u (fp32
        # storage, 3x3 / stride 1), packed stem filter wp (16-bit storage)
        m = self.model
        self.folded, self._folds = {}, []
        for trunk, _, cin, _ in m._trunks():
            self._add_fold(trunk.conv1, trunk.bn1, 64, 49, cin, 4, stem=True)
            for s in range(1, 5):
                for blk in getattr(trunk, f"layer{s}"):
                    K, C = blk.conv1.out_channels, blk.conv1.in_channels
                    self._add_fold(blk.conv1, blk.bn1, K, 9, C, C, wino=blk.stride == 1)
                    self._add_fold(blk.conv2, blk.bn2, K, 9, K, K, wino=True)
                    if blk.downsample is not None:
                        self._add_fold(blk.downsample[0], blk.downsample[1], K, 1, C, C)

    def _make_walk(self):
        return _Walk(_table(self.wtable), _table(self.wtable16) if self.dtype != F32 else None,
                     lambda conv, *_: self.folded[id(conv.weight)], self.dtype)

    def _add_fold(self, conv, bn, K, taps, cin, cpad, wino=False, stem=False):
        dev, h16 = self.model.device, self.dtype != F32
        f = _Folded(torch.empty((K, taps, cpad), dtype=self.dtype, device=dev), torch.empty((K,), dtype=F32, device=dev),
                    torch.empty(lib().winograd_weight_floats(K, cin), dtype=F32, device=dev) if wino and not h16 else None,
                    torch.empty((64, 7, 8, 4), dtype=self.dtype, device=dev) if stem and h16 else None)
        self.folded[id(conv.weight)] = f
        self._folds.append((conv, bn, K, taps, cin, cpad, f))

    def _tensors(self):
        yield self._flat32
        yield self._flat16
        for f in self.folded.values():
            for t in f:
                if t is not None:
                    yield t

    @property
    def nbytes(self):
        """device bytes the snapshot holds"""
        return sum(t.numel() * t.element_size() for t in self._tensors())

    @torch.no_grad()
    def refresh(self):
        """Take a new snapshot of the model - parameters from wherever ``param.data`` points right now (an applied EMA
        shadow is honoured) and the BatchNorm running statistics - into the SAME device buffers (a graph captured by
        capture() sees the new weights).  Asynchronous on the current stream."""
        m = self.model
        if any(id(p) not in self.wtable and id(p) not in self.wtable16 and id(p) not in self._trunk_ids and
               id(p) not in self._own_ids for p in m.parameters()):
            raise RuntimeError("the model's Parameter objects were replaced after freeze_inference(); freeze it again")
        for p, seg in self._copies:
            if seg.dtype == F32:
                seg.view(p.shape).copy_(p.data)
            else:
                ops.cast_bf16(p.data.contiguous(), out=seg.view(p.shape))
        for conv, bn, K, taps, cin, cpad, f in self._folds:
            ops.bn_fold(_live_ptr(conv.weight), bn, K, taps, cin, cpad, out=(f.w, f.b))
            if f.u is not None:
                ops.winograd_weights(f.w.data_ptr(), K, cin, m.device, out=f.u)
            if f.wp is not None:
                ops.bf16_stem_pack_filter(f.w, out=f.wp)
        return self

    # ---------------------------------------------------------------- nn.Module-like surface ----
    training = False   # always the eval-mode forward: train.validate / train.test take the engine in place of the model

    def eval(self):
        return self

    def train(self, mode=True):
        """accepted and ignored (validate / test restore the flag they found): the engine has no training mode"""
        return self

    # ---------------------------------------------------------------- forward -------------------
    @torch.no_grad()
    def __call__(self, image_list, lidar_list=None, radar_list=None, gps=None, rebuild_modality_feat_list=None):
        m = self.model
        images, lidars, radars, gps = m._inputs(image_list, lidar_list, radar_list, gps)
        try:
            return m._run_forward_walk(self._walk, images, lidars, radars, gps)[0]
        finally:
            lib().set_dropout_salt(0)

    forward = __call__

    def capture(self, image_list, lidar_list, radar_list, gps):
        """Captures the engine's forward for inputs of these shapes into ONE HIP graph and returns
        ``run(image_list, lidar_list, radar_list, gps) -> logits`` as ``TransFuser.capture_inference`` does: static input
        buffers, one replay per call, the returned tensor overwritten by the next replay.  The graph reads the engine's
        snapshot buffers, which ``refresh()`` rewrites in place: the same ``run`` serves the refreshed weights."""
        return capture_forward(self, self.model.device, image_list, lidar_list, radar_list, gps)
