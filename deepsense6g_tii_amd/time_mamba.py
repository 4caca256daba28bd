"""The temporal Mamba fusion head of the reference (TimeMamba, mambafuser_seq.py:233-284) on the gfx950 kernels: a drop-in
fp32 nn.Module whose state dict is interchangeable with the reference's.

    y_m  = mamba(x_m)  for image, lidar, radar (B, 5, 512): ONE layer, shared weights
    s[r] = max_c row[r][c] + mean_c row[r][c]            per row of y_m and of gps (B, 2, 512), which skips the layer
    a_m  = softmax(mlp.0(s_m)) over the 5 frames (mlp shared by the three), a_g = softmax(mlp_gps.0(s_g)) over the 2 gps rows
    out  = sum_m sum_t a_m[t] y_m[t] + sum_j a_g[j] gps[j]                                                      -> (B, 512)

The reference hard-wires the widths (kernel_size=512, expand(-1, -1, 512), Linear(5, 5), Linear(2, 2)): d_model must be 512
and every modality must bring exactly 5 frames (n_views == 1, seq_len == 5).  The gradient through the max goes to one
channel per row, the lowest one of a tie (torch's CPU pooling rule).

The whole head is ONE autograd node.  The three modalities go through mamba.layer_forward / layer_backward as one
(3 B, 5, 512) modality-major batch - one layer call, not three - so the layer's own fixed-order reductions sum the shared
weights' gradients over the modalities.  Everything behind the layer is one launch each way (csrc/time_mamba.hip:
ds6g_time_attn_fwd / _bwd) plus ds6g_batch_sum for the 36 mlp / mlp_gps gradient values.  The node's body is the pair
time_mamba_forward / time_mamba_backward, plain functions a model walk can call without autograd; they take the gps rows by
sample stride, so such a walk can point them at the last two token rows of a stage's (B, T, 512) output without a copy.

Parameters keep torch's and the Mamba layer's own initialisation (the reference applies no _init_weights here).  mlp and
mlp_gps are parameter holders: the arithmetic is the HIP kernels'.

Supported: fp32, HIP device only, d_model 512, d_state 16, d_conv 4, 5 frames.  Train and eval; no tape is kept when no
gradient is needed.  Not covered: 16-bit storage, the frozen inference engine.  The model that calls the pair is mamba_fuser.py.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .mamba import Mamba, _check_params, layer_forward, layer_backward

F32 = torch.float32
D_MODEL = 512
FRAMES = 5


def _gps_view(gps, ld_gps_sample, B):
    return torch.as_strided(gps, (B, 2, D_MODEL), (ld_gps_sample, D_MODEL, 1), gps.storage_offset())


def time_mamba_forward(mod, ws, save, rows, gps, ld_gps_sample, B, params=None):
    """rows [3*B*5, 512] (contiguous): the pooled frames, modality-major (image, lidar, radar; then sample, frame).  gps: a
    tensor whose first element is sample 0's first gps row; sample b's two rows start ld_gps_sample floats further each.
    `params`: the 13 parameters in TimeMamba._params() order (default: mod's); `ws`: a Workspace of at least
    mod.mamba.workspace_bytes(3 * B, 5).  -> (out [B, 512], tape or None)"""
    params = mod._params() if params is None else params
    y, ltape = layer_forward(mod.mamba, ws, False, save, rows, 3 * B, FRAMES, params[:9])
    out, attn, score, argmax = ops.time_attn_fwd(y, _gps_view(gps, ld_gps_sample, B), *params[9:], B)
    return out, ((*ltape, y, attn, score, argmax) if save else None)


def time_mamba_backward(mod, ws, tape, dout, gps, ld_gps_sample, B, params=None, gdst=None):
    """dout [B, 512] (contiguous) -> (drows [3*B*5, 512] in rows' layout, dgps [B, 2, 512], the 13 parameter gradients in
    TimeMamba._params() order).  gdst: 13 (device pointer, accumulate flag) pairs in that order - the gradients are written
    there in place (added where the flag is set) and None is returned in their stead (mamba.layer_backward's convention)."""
    params = mod._params() if params is None else params
    ltape, (y, attn, score, argmax) = tape[:8], tape[8:]
    gv = _gps_view(gps, ld_gps_sample, B)
    if gdst is None:
        dy, dgps, dp = ops.time_attn_bwd(dout, y, gv, attn, score, argmax, params[9], params[11], B)
        drows, g_layer = layer_backward(mod.mamba, ws, False, 3 * B, FRAMES, ltape, params[:9], dy)
        return drows, dgps, (*g_layer, dp[:25].view(5, 5), dp[25:30], dp[30:34].view(2, 2), dp[34:36])
    assert len(gdst) == 13, len(gdst)
    dy, dgps, _ = ops.time_attn_bwd(dout, y, gv, attn, score, argmax, params[9], params[11], B, dst=gdst[9:])
    drows, _ = layer_backward(mod.mamba, ws, False, 3 * B, FRAMES, ltape, params[:9], dy, gdst=gdst[:9])
    return drows, dgps, None


class _TimeFn(torch.autograd.Function):
    """the whole head; inputs after gps: the nine parameters of mamba, mlp.0.weight / bias, mlp_gps.0.weight / bias"""

    @staticmethod
    def forward(ctx, mod, save, image, lidar, radar, gps, *params):
        B = image.shape[0]
        ws = mod.mamba._workspace(image.device, 3 * B, FRAMES)
        rows = torch.cat([image.detach(), lidar.detach(), radar.detach()], 0).view(3 * B * FRAMES, D_MODEL)
        g = gps.detach().contiguous()
        out, tape = time_mamba_forward(mod, ws, save, rows, g, 2 * D_MODEL, B, params)
        if save:
            ctx.mod, ctx.B = mod, B
            ctx.save_for_backward(g, *tape, *params)
        return out

    @staticmethod
    def backward(ctx, dout):
        st = ctx.saved_tensors
        g, tape, params = st[0], st[1:13], st[13:]
        mod, B = ctx.mod, ctx.B
        ws = mod.mamba._workspace(dout.device, 3 * B, FRAMES)
        drows, dgps, grads = time_mamba_backward(mod, ws, tape, dout.contiguous(), g, 2 * D_MODEL, B, params)
        d = drows.view(3, B, FRAMES, D_MODEL)
        return (None, None, d[0], d[1], d[2], dgps, *grads)


class TimeMamba(nn.Module):
    """the reference's TimeMamba: constructor arguments, forward signature and state-dict names"""

    def __init__(self, d_model=512, d_state=16, d_conv=4, expand=2, device=None):
        super().__init__()
        if d_model != D_MODEL:
            raise ValueError(f"TimeMamba: d_model must be {D_MODEL} (the reference pools and expands over 512 channels), got "
                             f"{d_model}")
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.mamba = Mamba(d_model=d_model, d_state=d_state, d_conv=d_conv, expand=expand, device=device)
        kw = dict(device=device, dtype=F32)
        self.mlp = nn.Sequential(nn.Linear(FRAMES, FRAMES, **kw), nn.Softmax(dim=-1))     # parameter holders
        self.mlp_gps = nn.Sequential(nn.Linear(2, 2, **kw), nn.Softmax(dim=-1))

    def _params(self):
        return (*self.mamba._params(), self.mlp[0].weight, self.mlp[0].bias, self.mlp_gps[0].weight, self.mlp_gps[0].bias)

    def forward(self, image_features, lidar_features, radar_features, gps_features):
        """image / lidar / radar: (B, 5, 512), gps: (B, 2, 512), fp32 on the HIP device -> fused features (B, 512)"""
        ins = (image_features, lidar_features, radar_features, gps_features)
        for t in ins:
            if not t.is_cuda:
                raise RuntimeError("deepsense6g_tii_amd.TimeMamba runs on MI355X HIP kernels only (no CPU path)")
        dev = image_features.device
        B = image_features.shape[0] if image_features.dim() == 3 else 0
        for t in ins[:3]:
            if tuple(t.shape) != (B, FRAMES, D_MODEL) or t.dtype != F32 or t.device != dev or B < 1:
                raise ValueError(f"TimeMamba: expected three (B, {FRAMES}, {D_MODEL}) fp32 tensors, got {tuple(t.shape)} "
                                 f"{t.dtype}")
        if tuple(gps_features.shape) != (B, 2, D_MODEL) or gps_features.dtype != F32 or gps_features.device != dev:
            raise ValueError(f"TimeMamba: expected gps of shape ({B}, 2, {D_MODEL}) fp32, got {tuple(gps_features.shape)} "
                             f"{gps_features.dtype}")
        params = self._params()
        _check_params("TimeMamba", params, dev)
        needs = any(t.requires_grad for t in ins) or any(p.requires_grad for p in params)
        save = torch.is_grad_enabled() and self.training and needs
        with torch.cuda.device(dev):
            if save:
                return _TimeFn.apply(self, True, *ins, *params)
            with torch.no_grad():
                return _TimeFn.apply(self, False, *ins, *params)
