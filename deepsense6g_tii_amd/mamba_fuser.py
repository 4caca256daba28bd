"""MambaFuser, the reference's default model (mambafuser_seq.py:286-597), on the TransFuser kernel walk.

    EncoderWithMamba  three ResNet trunks, vel_emb1..4, mambafusion1..4 (the bi-branch Mamba fusion stage, mamba_fusion.py) in
                      place of the four GPTs, and time_mamba (the temporal head, time_mamba.py)
    MambaFuser        TransFuser with that encoder: same stems, BasicBlocks, join MLP, arenas, autograd boundary, optimizer
                      and data-parallel hooks; the four fusion stages and the fused-feature head are overridden

The walk is TransFuser's (model.py).  What differs, stage by stage: vel_emb{s} on the small-linear kernel, then
mamba_fusion.stage_forward / stage_backward (pool-swap token pack, the blocks, ln_f, grouped upsample-add), every parameter
gradient written straight into the gradient arena.  The head: with config.TFM the grouped head pool (ops.pool_rows3_fwd / _bwd,
csrc/time_mamba.hip) and time_mamba_forward / time_mamba_backward(gdst=), the gps rows read from the last stage's tokens by sample
stride; without it the parent's 17-token sum.  Parameter names and shapes equal the reference's state dict.

Storage: the compute modes "f32", "bf16" and "f16", as for TransFuser - the parent's _refresh_shadow16 decides the walk's
storage once per forward ("f16": train it under train.DynamicLossScaler).  On a 16-bit walk:

    tensor                                                          storage
    the trunks' maps, the stage's maps in and out, their gradients  16-bit (the parent's walk; mamba_fusion.py's stage map)
    gemb, dgemb, xo (a stage's output tokens, cap["mamba{s}"]),     fp32
    dgps_tok, vel_emb{s} and its gradients
    the stage's fc1 / fc2 / in_proj / x_proj / out_proj weights     read in place in the walk's 16-bit shadow of the arena
                                                                    (stage_forward(w16=)) where weight_route allows it; a copy
                                                                    cast once per forward, kept on the stage record, for the rest
                                                                    (stage 1's x_proj: 36 rows padded with zero rows to 40)
    head with TFM: rows, drows, the whole temporal head              fp32: ops.pool_rows3_fwd reads the 16-bit maps into fp32
                                                                    rows, time_mamba_forward / _backward are untouched,
                                                                    ops.pool_rows3_bwd writes 16-bit map gradients (one rounding)
    head without TFM, join, logits, loss, every parameter gradient  the parent's (fp32)
The walk falls back to fp32 storage where the parent's does: eval() with folded BatchNorm, parameters re-pointed away from the
arena (an applied EMA shadow); the stages then take fp32 maps and run as in mode "f32".  In mode "f32" the model makes the
launches it made before 16-bit storage existed, bit for bit.

Supported: compute modes "f32", "bf16", "f16"; config.n_views == 1, 8 x 8 anchors, no missing-modality options, any
seq_len >= 1 without TFM, seq_len == 5 with it (the head hard-wires Linear(5, 5)).  Anything else raises at construction, or at
the first forward for the compute mode ("f32x3" / "f32x6": the Mamba kernels have no split-bf16 form).  Not covered: TimeMamba
on 16-bit storage (its tensors are [3 B 5, 512] fp32 rows, 0.3 ms of a 115 ms step, and the last arithmetic before the logits),
the MambaFusion module form on 16-bit storage, hipGraph capture (capture_inference and train.CapturedTrainStep raise
NotImplementedError in every mode), missing-modality input replacement and feature injection, n_views > 1.

Serving: mamba_infer.freeze(model, storage) -> MambaFuserEngine, the frozen inference engine on f32 / bf16 / f16 storage (a
snapshot with BN-folded trunks and the stages' stacked GEMM weights; this model's walk under _Walk.frozen, where _stage_fwd
runs mamba_fusion.stage_forward_frozen).  MambaFuser.freeze_inference itself still raises NotImplementedError and names that
entry point.
"""
from __future__ import annotations

import torch
from torch import nn

from . import mamba_fusion, ops
from ._lib import lib
from .mamba import x_proj_rows16
from .mamba_fusion import MambaFusion
from .model import F32, STAGE_WIDTH, ImageCNN, LidarEncoder, TransFuser, _record
from .time_mamba import FRAMES, TimeMamba, time_mamba_backward, time_mamba_forward

# a Mamba fusion stage: C, T as the walk reads them; gps_src addresses the (B, 2, K) input of vel_emb{s}; tape = what
# mamba_fusion.stage_backward takes; fshapes = the shapes of the three maps; copies = the 16-bit weight copies the tape's
# pointers address (None on fp32 storage), alive until the backward has run
_MambaStageRec = _record("_MambaStageRec", "s C T gps_src tape fshapes copies")

# ---- where a stage's 16-bit GEMM weights come from ---------------------------------------------------------------------------
# The 16-bit GEMMs (csrc/bgemm.hip) read a weight [rows, cols] through a buffer descriptor in 16-byte pieces of one row: cols a
# multiple of 64 where the weight is the K-contiguous operand, rows a multiple of 8, and a base address that only has to be
# dword-aligned - the GPT stages and the trunk convolutions have always handed them shadow pointers that are 8-byte aligned
# and no better (arena segments are padded to 4 elements, so a shadow offset is a multiple of 8 bytes).
SHADOW_ALIGN = 8


def block_weights16(blk):
    """the eight weights of a MambaBlock that its 16-bit GEMMs read, in mamba_fusion.block_weight_copies16's order (fc1, fc2;
    in_proj, x_proj, out_proj of the forward Mamba, then of the reverse one), each with the rows its 16-bit operand must
    have: the weight's own, but mamba.x_proj_rows16 for x_proj (the added rows zero)"""
    out = [(blk.fc1.weight, blk.fc1.weight.shape[0]), (blk.fc2.weight, blk.fc2.weight.shape[0])]
    for mod in (blk.forward_mamba, blk.backward_mamba):
        out += [(mod.in_proj.weight, mod.in_proj.weight.shape[0]), (mod.x_proj.weight, x_proj_rows16(mod.dt_rank)),
                (mod.out_proj.weight, mod.out_proj.weight.shape[0])]
    return out


def weight_route(shadow_ptr, rows, rows16):
    """Pure host rule: "shadow" - the 16-bit GEMMs read the weight in place in the walk's 16-bit shadow of the arena - where the
    shadow holds exactly the operand they need (rows == rows16: nothing to pad) at an address they accept (SHADOW_ALIGN);
    "copy" otherwise: a separate buffer of rows16 rows, cast once per forward"""
    return "shadow" if rows == rows16 and int(shadow_ptr) % SHADOW_ALIGN == 0 else "copy"


class EncoderWithMamba(nn.Module):  # mambafuser_seq.py:286-359
    """parameter container under the reference's names; its forward() is never called"""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.image_encoder = ImageCNN(512, normalize=True)
        self.lidar_encoder = LidarEncoder(512, in_channels=1)
        self.radar_encoder = LidarEncoder(512, in_channels=2 if config.add_velocity else 1)
        self.vel_emb1 = nn.Linear(2, 64)
        self.vel_emb2 = nn.Linear(64, 128)
        self.vel_emb3 = nn.Linear(128, 256)
        self.vel_emb4 = nn.Linear(256, 512)
        T = 192 * config.seq_len + 2   # the reference hard-codes 962 (seq_len 5)
        for s, C in enumerate(STAGE_WIDTH, start=1):
            setattr(self, f"mambafusion{s}", MambaFusion(C, (T, C), 16, 4, 2, config.n_layer, config.vert_anchors,
                                                         config.horz_anchors, config.seq_len, config.embd_pdrop, config))
        self.time_mamba = TimeMamba(512, 16, 4, 2)   # constructed whether or not config.TFM is set, as the reference does


class MambaFuser(TransFuser):
    """Drop-in for mambafuser_seq.MambaFuser.  See the module docstring."""
    GRAPH_CAPTURE = False   # train.CapturedTrainStep refuses: graph replay of this walk has never been run

    def __init__(self, config, device, pretrain_weight=False):
        if getattr(config, "n_views", 1) != 1:
            raise ValueError(f"MambaFuser: config.n_views must be 1 (the reference's token cat only lines up then), got "
                             f"{config.n_views}")
        if (config.vert_anchors, config.horz_anchors) != (8, 8):
            raise ValueError(f"MambaFuser: 8 x 8 anchors only, got {config.vert_anchors} x {config.horz_anchors}")
        if getattr(config, "modality_missing", None) is not None:
            raise ValueError(f"MambaFuser: config.modality_missing = {config.modality_missing!r} is not supported (input "
                             "replacement and feature injection are not built)")
        if config.seq_len < 1:
            raise ValueError(f"MambaFuser: seq_len must be positive, got {config.seq_len}")
        if getattr(config, "TFM", 0) and config.seq_len != FRAMES:
            raise ValueError(f"MambaFuser: config.TFM needs seq_len == {FRAMES} (the temporal head hard-wires "
                             f"Linear({FRAMES}, {FRAMES})), got {config.seq_len}")
        super().__init__(config, device, pretrain_weight)
        # stage -> (weights read from the 16-bit shadow, weights copied) of the last forward on 16-bit storage (weight_route)
        self.w16_routes = {}

    def _make_encoder(self, config):
        return EncoderWithMamba(config)

    def load_pretrained_weight(self):  # mambafuser_seq.py:578-581
        self.load_state_dict(torch.load("fusion_model.pth", weights_only=True))

    @staticmethod
    def _milestone(name):
        """as the parent's; the Mamba stage s and vel_emb{s} finish with GPT stage s, time_mamba between the join and stage 4"""
        if "time_mamba." in name:
            return 1
        for s in (4, 3, 2, 1):
            if f"mambafusion{s}." in name or f"vel_emb{s}." in name:
                return 1 + 2 * (4 - s)
        return TransFuser._milestone(name)

    # ---------------------------------------------------------------- what is not built ---------
    def freeze_inference(self, storage="f32"):
        raise NotImplementedError("MambaFuser.freeze_inference is not routed to the frozen engine of the Mamba walk yet: "
                                  "use deepsense6g_tii_amd.mamba_infer.freeze(model, storage)")

    def capture_inference(self, image_list, lidar_list, radar_list, gps):
        raise NotImplementedError("MambaFuser.capture_inference: graph replay of the Mamba walk is not supported")

    def forward(self, image_list, lidar_list=None, radar_list=None, gps=None, rebuild_modality_feat_list=None):
        if rebuild_modality_feat_list is not None:
            raise NotImplementedError("MambaFuser: rebuild_modality_feat_list (feature injection) is not supported")
        return super().forward(image_list, lidar_list, radar_list, gps)

    def _inputs(self, image_list, lidar_list, radar_list, gps):
        out = super()._inputs(image_list, lidar_list, radar_list, gps)
        if self.config.n_views != 1:
            raise ValueError(f"MambaFuser: one camera frame per time step (n_views == 1), got {self.config.n_views}")
        return out

    def _new_walk(self, record):
        """the parent's walk: in compute modes "bf16" / "f16" the parent's _refresh_shadow16 decides the storage (16-bit from
        the arena's shadow; fp32 in eval() with folded BatchNorm or with re-pointed parameters, as for TransFuser).  The split
        modes have no Mamba kernels"""
        if lib().get_compute_mode() not in (0, 1, 5):
            raise RuntimeError(f'MambaFuser runs in compute modes "f32", "bf16" and "f16" only, the library is in '
                               f'"{ops.get_compute_mode()}"')
        return super()._new_walk(record)

    # ---------------------------------------------------------------- the stages ----------------
    def _mamba_ws(self, need):
        """the calling stream's scratch, the main one grown to `need` bytes where 1 GiB is too small"""
        ws = self._ws
        if ws.nbytes < need:
            if ws is not self._ws_main:
                raise RuntimeError(f"MambaFuser: a side stream's scratch has {ws.nbytes} bytes, {need} needed")
            self._ws_main = ws = ops.Workspace(self.device, need)
        return ws

    def _stage_w16(self, wk, fus, st):
        """the `w16` of mamba_fusion.stage_forward on 16-bit storage `st`, without the stage's own casts: a pointer into the
        walk's 16-bit shadow (refreshed once per forward) for every weight weight_route sends there, a copy cast now from the
        fp32 master for the rest.  -> (one block_weight_copies16 pointer tuple per block, the copies - they have to outlive
        the backward -, (weights read from the shadow, weights copied))"""
        ptrs, copies, n_shadow = [], [], 0
        for blk in fus.mambablocks:
            p = []
            for prm, rows16 in block_weights16(blk):
                rows, cols = prm.shape
                if weight_route(wk.w16(prm), rows, rows16) == "shadow":
                    p.append(wk.w16(prm))
                    n_shadow += 1
                    continue
                # the added rows must be zero (mamba.weight_copies16's layout, so also its bits)
                c = (torch.zeros if rows16 != rows else torch.empty)((rows16, cols), dtype=st, device=self.device)
                ops.cast_bf16(prm.detach(), out=c[:rows])
                copies.append(c)
                p.append(c.data_ptr())
            ptrs.append((p[0], p[1], tuple(p[2:5]), tuple(p[5:8])))
        return ptrs, copies, (n_shadow, len(copies))

    def _stage_fwd(self, wk, s, feats, gps_src, B):
        """Mamba fusion at scale s (1-based): vel_emb{s}, then the stage on the walk's conventions.  feats[0].dtype is the
        stage's storage (the walk's: fp32, bf16 or f16): the maps in and out have it; gemb, the returned tokens xo and
        vel_emb{s} are fp32 on every storage"""
        C = STAGE_WIDTH[s - 1]
        fus = getattr(self.encoder, f"mambafusion{s}")
        vel = getattr(self.encoder, f"vel_emb{s}")
        T = fus.n_tokens
        st = feats[0].dtype
        for m in range(3):
            assert feats[m].shape[0] == B * fus.seq_len and feats[m].shape[3] == C and feats[m].dtype == st
        pe = fus.embd_pdrop if wk.train else 0.0
        off_e = self._next_drop(B * T * C) if pe > 0 else 0
        _, gptr, rpg, gstride, K = gps_src
        gemb = torch.empty((B, 2, C), dtype=F32, device=self.device)
        lib().small_linear_fwd(gptr, wk.w(vel.weight), wk.w(vel.bias), gemb.data_ptr(), 2 * B, C, K, rpg, gstride, 0,
                               ops._stream())
        ws = self._mamba_ws(mamba_fusion.stage_workspace_bytes(fus, B))
        outs = [torch.empty_like(f) for f in feats]
        if wk.frozen is not None:     # a frozen engine's walk (mamba_infer.py): its own operands, no tape, no weight cast
            xo = mamba_fusion.stage_forward_frozen(fus, ws, feats, gemb, outs, B, wk.frozen.stages[s - 1])
            cap = getattr(self, "_capture", None)
            if cap is not None:
                cap[f"mamba{s}"] = xo.clone()
            return outs, xo, _MambaStageRec(s, C, T, gps_src, None, [f.shape for f in feats], None)
        w16 = copies = None
        if st != F32:
            assert st == wk.dtype and wk.w16 is not None, (st, wk.dtype)
            w16, copies, self.w16_routes[s] = self._stage_w16(wk, fus, st)
        xo, tape = mamba_fusion.stage_forward(fus, ws, wk.record, feats, gemb, outs, B, drop=(pe, self._seed, off_e), w16=w16)
        cap = getattr(self, "_capture", None)
        if cap is not None:
            cap[f"mamba{s}"] = xo.clone()
        return outs, xo, _MambaStageRec(s, C, T, gps_src, tape, [f.shape for f in feats], copies)

    def _stage_bwd(self, wk, rec, dfeats_out, dgps_tok, B):
        s, C, fshapes = rec.s, rec.C, rec.fshapes
        fus = getattr(self.encoder, f"mambafusion{s}")
        vel = getattr(self.encoder, f"vel_emb{s}")
        st = dfeats_out[0].dtype     # the forward's storage: stage_backward holds the tape to it
        for m in range(3):
            assert dfeats_out[m].shape == tuple(fshapes[m]) and dfeats_out[m].dtype == st
        dfeats = [torch.empty(tuple(fshapes[m]), dtype=st, device=self.device) for m in range(3)]
        dgemb = torch.empty((B, 2, C), dtype=F32, device=self.device)
        ws = self._mamba_ws(mamba_fusion.stage_workspace_bytes(fus, B))
        mamba_fusion.stage_backward(fus, ws, rec.tape, dfeats_out, dgps_tok, dfeats, dgemb, B, wk.g)
        _, gptr, rpg, gstride, K = rec.gps_src
        gw, aw = wk.g(vel.weight)
        gb, _ = wk.g(vel.bias)
        if s > 1:
            dprev = torch.empty((B, 2, K), dtype=F32, device=self.device)
            dptr = dprev.data_ptr()
        else:
            dprev, dptr = None, 0
        lib().small_linear_bwd(dgemb.data_ptr(), 0, gptr, wk.w(vel.weight), dptr, gw, gb, 2 * B, C, K, rpg, gstride, 2 * B, 0,
                               0, aw, ops._stream())
        return dfeats, dprev

    # ---------------------------------------------------------------- the head ------------------
    def _head_fwd(self, wk, feats, xo, B, T):
        if not getattr(self.config, "TFM", 0):
            return super()._head_fwd(wk, feats, xo, B, T)
        tm = self.encoder.time_mamba
        for f in feats:
            assert tuple(f.shape) == (B * FRAMES, 8, 8, 512) and f.dtype == feats[0].dtype, (tuple(f.shape), f.dtype)
        # the maps have the walk's storage; from the pooled rows on, the temporal head is fp32 on every storage
        rows = torch.empty((3 * B * FRAMES, 512), dtype=F32, device=self.device)
        ops.pool_rows3_fwd(feats, rows)
        gps = xo.view(-1)[(T - 2) * 512:]   # sample b's two gps rows start b * T * 512 floats further: no copy
        ws = self._mamba_ws(tm.mamba.workspace_bytes(3 * B, FRAMES))
        # a frozen engine's walk reads the head's parameters from its snapshot, every other walk where they live
        fused, tape = time_mamba_forward(tm, ws, wk.record, rows, gps, T * 512, B,
                                         params=None if wk.frozen is None else wk.frozen.time_params)
        return fused, (tape, gps, T)

    def _head_bwd(self, wk, head, dfused, B):
        tm = self.encoder.time_mamba
        params = tm._params()
        if head.hook is None:
            # the 17-token sum: time_mamba took no part in this forward.  Its gradients are exactly zero, not whatever an
            # earlier step left in the arena (they are one contiguous run of it; an accumulated gradient stays as it is)
            if all(wk.g(p)[1] == 0 for p in params):
                lo = min(self._pslice[n][0] for n, _ in self._plist if n.startswith("encoder.time_mamba."))
                hi = max(sum(self._pslice[n]) for n, _ in self._plist if n.startswith("encoder.time_mamba."))
                self._garena[lo:hi].zero_()
            return super()._head_bwd(wk, head, dfused, B)
        tape, gps, T = head.hook
        ws = self._mamba_ws(tm.mamba.workspace_bytes(3 * B, FRAMES))
        drows, dgps, _ = time_mamba_backward(tm, ws, tape, dfused, gps, T * 512, B, gdst=[wk.g(p) for p in params])
        dfeats = [torch.empty(tuple(head.fshapes[m]), dtype=head.fdtype, device=self.device) for m in range(3)]
        ops.pool_rows3_bwd(drows, None, dfeats)
        return dfeats, (dgps, False)
