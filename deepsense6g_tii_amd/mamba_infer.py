"""Frozen inference engine of MambaFuser: ``freeze(model, storage)`` -> :class:`MambaFuserEngine`.

``model.eval()`` is MambaFuser's only other inference path.  It folds every BatchNorm and transforms every Winograd filter
again on each call, runs fp32 storage whenever BatchNorm is folded (so 16-bit inference does not exist there), and every
MambaBlock is a chain of about two dozen dependent launches.  A frozen model's weights do not change between calls and an
inference forward keeps no tape, so the engine prepares ONCE, in memory it owns and in the storage type asked for:

  trunks                  infer.InferenceEngine's folds, unchanged: BN-folded filter + bias of every conv, the Winograd
                          filter (fp32 storage), the packed stem filter (16-bit storage)
  per MambaBlock, in the  fc1.weight; the stacked [9C, C] weight (mamba_fusion.cat9_layout: in_proj of the forward Mamba, in_proj
  storage type (fp32      of the reverse Mamba, fc2) that turns the three GEMMs reading x1 into one; both x_proj.weight, on
  under "f32")            16-bit storage zero-padded to mamba.x_proj_rows16 rows (refresh() writes only the real rows: the
                          padding stays zero); both out_proj.weight
  always fp32             the stacked [9C] bias (zero but for fc2.bias), fc1.bias, ln1, conv1d.*, dt_proj.*, A_log, D, pos_emb,
                          ln_f, vel_emb*, the whole time_mamba head, join

The forward is the model's own walk (``TransFuser._run_forward_walk``) under a ``_Walk`` whose ``frozen`` slot carries the
per-stage operands: ``MambaFuser._stage_fwd`` then runs vel_emb{s} and ``mamba_fusion.stage_forward_frozen`` - per block six
GEMMs, one grouped conv, one grouped scan with dt_proj inside (csrc/mamba_infer.hip), the sample LayerNorm and the gate - and
``_head_fwd`` hands the temporal head the snapshot's parameters.  No per-forward shadow refresh, weight cast or x_proj copy.

The contract is the parent's (infer.py): a SNAPSHOT that never reads the model between ``refresh()`` calls; ``refresh()``
rewrites the same device buffers from wherever ``param.data`` points and from the BatchNorm running statistics, and refuses a
model whose Parameter objects were replaced; ``engine(image_list, lidar_list, radar_list, gps)`` takes what
``MambaFuser.forward`` takes (``data.PackedInputs`` included) and returns fp32 logits; ``training`` is False and
``eval()`` / ``train()`` are accepted, so ``train.validate`` / ``train.test`` take the engine in place of the model.

Refused: a model that is not a MambaFuser (TypeError), an unknown storage (ValueError), a CPU model (RuntimeError), a call
while the library is in a split compute mode "f32x3" / "f32x6" (RuntimeError: the Mamba kernels have no split-bf16 form),
``rebuild_modality_feat_list`` (NotImplementedError) and ``capture()`` (NotImplementedError: graph replay of the Mamba walk
has never been run).  ``MambaFuser.freeze_inference`` still raises and names this module; routing it here is a one-line change.
"""
from __future__ import annotations

import re
from types import SimpleNamespace

import torch

from . import ops
from ._lib import lib
from .infer import _STORAGE, F32, InferenceEngine
from .mamba import x_proj_rows16
from .mamba_fuser import MambaFuser
from .mamba_fusion import cat9_layout

# the block parameters the engine keeps in buffers of its own layout (the stacked weight and bias, the padded x_proj) ...
_OWN = re.compile(r"\.mambablocks\.\d+\.(fc2\.(weight|bias)|(forward|backward)_mamba\.(in_proj|x_proj)\.weight)$")
# ... and the remaining GEMM operands of a block: stored in the engine's 16-bit type under "bf16" / "f16"
_GEMM_WEIGHT = re.compile(r"\.mambablocks\.\d+\.(fc1|(forward|backward)_mamba\.out_proj)\.weight$")


class MambaFuserEngine(InferenceEngine):
    """See the module docstring."""

    def __init__(self, model, storage="f32"):
        if not isinstance(model, MambaFuser):
            raise TypeError(f"MambaFuserEngine freezes a MambaFuser, got {type(model).__name__} (TransFuser models: "
                            "model.freeze_inference(storage))")
        if storage not in _STORAGE:
            raise ValueError(f"storage must be one of {sorted(_STORAGE)}, got {storage!r}")
        super().__init__(model, storage)

    # ---------------------------------------------------------------- snapshot ------------------
    def _placement(self, name):
        if _OWN.search(name):
            return None
        return self.dtype != F32 and _GEMM_WEIGHT.search(name) is not None

    def _allocate_params(self):
        super()._allocate_params()
        m, dev, st = self.model, self.model.device, self.dtype
        seg = {id(p): s.view(p.shape) for p, s in self._copies}     # parameter -> its snapshot tensor, in the parameter's shape
        snap = lambda p: seg[id(p)]  # noqa: E731
        self._own, self._stacks, stages = [], [], []
        for s in range(1, 5):
            fus = getattr(m.encoder, f"mambafusion{s}")
            C = fus.n_embd
            lay = cat9_layout(C)
            blocks = []
            for blk in fus.mambablocks:
                cat_w = torch.zeros((lay.n, C), dtype=st, device=dev)
                cat_b = torch.zeros((lay.n,), dtype=F32, device=dev)
                rows = lay.rows
                self._stacks += [(blk.forward_mamba.in_proj.weight, cat_w[rows["in_proj_fwd"][0]:rows["in_proj_fwd"][1]]),
                                 (blk.backward_mamba.in_proj.weight, cat_w[rows["in_proj_bwd"][0]:rows["in_proj_bwd"][1]]),
                                 (blk.fc2.weight, cat_w[rows["fc2"][0]:rows["fc2"][1]]),
                                 (blk.fc2.bias, cat_b[rows["fc2"][0]:rows["fc2"][1]])]
                self._own += [cat_w, cat_b]
                dirs = []
                for mod in (blk.forward_mamba, blk.backward_mamba):
                    r = mod.dt_rank
                    n_x = r + 32 if st == F32 else x_proj_rows16(r)
                    x_w = torch.zeros((n_x, mod.d_inner), dtype=st, device=dev)     # rows past r + 32 stay zero for ever
                    self._stacks.append((mod.x_proj.weight, x_w[:r + 32]))
                    self._own.append(x_w)
                    dirs.append(SimpleNamespace(conv_w=snap(mod.conv1d.weight), conv_b=snap(mod.conv1d.bias), x_w=x_w,
                                                dt_w=snap(mod.dt_proj.weight), dt_b=snap(mod.dt_proj.bias),
                                                A_log=snap(mod.A_log), D=snap(mod.D), out_w=snap(mod.out_proj.weight)))
                blocks.append(SimpleNamespace(ln_w=snap(blk.ln1.weight), ln_b=snap(blk.ln1.bias), fc1_w=snap(blk.fc1.weight),
                                              fc1_b=snap(blk.fc1.bias), cat_w=cat_w, cat_b=cat_b, dirs=tuple(dirs)))
            stages.append(SimpleNamespace(pos_emb=snap(fus.pos_emb), ln_f_w=snap(fus.ln_f.weight), ln_f_b=snap(fus.ln_f.bias),
                                          blocks=blocks))
        self._frozen = SimpleNamespace(stages=stages, time_params=tuple(snap(p) for p in m.encoder.time_mamba._params()))

    def _make_walk(self):
        wk = super()._make_walk()
        wk.frozen = self._frozen
        return wk

    def _tensors(self):
        yield from super()._tensors()
        yield from self._own

    @torch.no_grad()
    def refresh(self):
        super().refresh()
        for p, dst in self._stacks:     # row blocks of the stacked weight / bias and the real rows of the padded x_proj
            if dst.dtype == F32:
                dst.copy_(p.data)
            else:
                ops.cast_bf16(p.data.contiguous(), out=dst)
        return self

    # ---------------------------------------------------------------- forward -------------------
    @torch.no_grad()
    def __call__(self, image_list, lidar_list=None, radar_list=None, gps=None, rebuild_modality_feat_list=None):
        if rebuild_modality_feat_list is not None:
            raise NotImplementedError("MambaFuserEngine: rebuild_modality_feat_list (feature injection) is not supported")
        if lib().get_compute_mode() not in (0, 1, 5):
            raise RuntimeError(f'MambaFuser runs in compute modes "f32", "bf16" and "f16" only, the library is in '
                               f'"{ops.get_compute_mode()}"')
        return super().__call__(image_list, lidar_list, radar_list, gps)

    forward = __call__

    def capture(self, image_list, lidar_list, radar_list, gps):
        raise NotImplementedError("MambaFuserEngine.capture: graph replay of the Mamba walk is not supported")


def freeze(model, storage="f32"):
    """-> MambaFuserEngine(model, storage): the frozen inference engine of a MambaFuser"""
    return MambaFuserEngine(model, storage)
