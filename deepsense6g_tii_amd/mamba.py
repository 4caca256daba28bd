"""The Mamba layer (mamba_ssm.Mamba, slow-path semantics) on the gfx950 kernels: a drop-in nn.Module whose state dict is
interchangeable with mamba_ssm.Mamba(d_model, d_state=16, d_conv=4, expand=2).

    xz    = in_proj(u);  x, z = halves of xz
    x     = silu(causal depthwise conv1d(x))
    x_dbl = x_proj(x);   dt, Bm, Cm = slices of x_dbl
    delta = softplus(dt_proj(dt))
    h_t   = exp(delta_t A) h_{t-1} + delta_t x_t Bm_t,  A = -exp(A_log);   y_t = <h_t, Cm_t> + D x_t
    out   = out_proj(y * silu(z))

The four projections are the fp32 implicit-GEMM linears (ops.linear_*); the conv and the scan are csrc/mamba.hip.  One
extension: forward(u, reverse=True) walks the sequence back to front (== flip(forward(flip(u))) without the copies), which
the reference's backward_mamba branch needs (mambafuser_seq.py:100-101).

Supported: d_state 16, d_conv 4, d_model % 64 == 0 (expand * d_model % 128 == 0, dt_rank % 4 == 0), bias=False,
conv_bias=True, fp32, any B, L >= 1.  Anything else raises ValueError at construction.  Not covered: bf16 / f16 storage, the
frozen inference engine, the single-step inference_params path.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops

F32 = torch.float32
_MIN_WS = 64 << 20   # room for the split-K slabs of the projection weight gradients


def layer_forward(mod, ws, reverse, save, u2, Bsz, L, params):
    """the layer on token rows u2 [B*L, d_model] (contiguous) -> (out [B*L, d_model], tape or None).  `params`: the nine
    parameters in Mamba._params() order; `ws`: a Workspace of at least mod.workspace_bytes(B, L).  Shared by _MambaFn and by
    the block-level Function of mamba_fusion.py, which runs two layers inside one autograd node."""
    w_in, conv_w, conv_b, w_x, w_dt, b_dt, A_log, Dp, w_out = params
    M, D, r, dm = Bsz * L, mod.d_inner, mod.dt_rank, mod.d_model
    xz = ops.linear_fwd(u2, w_in.data_ptr(), 0, 2 * D)
    z = xz[:, D:]
    xc = ops.causal_conv1d_silu_fwd(xz[:, :D], conv_w, conv_b, Bsz, L, reverse)
    x_dbl = ops.linear_fwd(xc, w_x.data_ptr(), 0, r + 32)
    dt = ops.copy_cols(x_dbl[:, :r], torch.empty((M, r), dtype=F32, device=u2.device))
    draw = ops.linear_fwd(dt, w_dt.data_ptr(), 0, D)       # dt_proj.bias is added inside the scan
    y, saved = ops.selective_scan_fwd(xc, draw, b_dt, A_log, x_dbl[:, r:r + 16], x_dbl[:, r + 16:], Dp, z, Bsz, L, ws,
                                      reverse, save)
    out = ops.linear_fwd(y, w_out.data_ptr(), 0, dm)
    return out, ((u2, xz, xc, x_dbl, dt, draw, y, saved) if save else None)


def grad_slots(shapes, device, gdst):
    """Where a backward writes its parameter gradients.  gdst None: fresh tensors of `shapes` (the autograd nodes return
    them).  gdst = one (device pointer, accumulate flag) per parameter (a model walk's gradient arena): the pointers
    themselves.  -> (slots: [(pointer, accumulate)], tensors or None)"""
    if gdst is None:
        ts = tuple(torch.empty(s, dtype=F32, device=device) for s in shapes)
        return [(t.data_ptr(), 0) for t in ts], ts
    assert len(gdst) == len(shapes), (len(gdst), len(shapes))
    return [(int(p), int(bool(a))) for p, a in gdst], None


def deliver_pair(fn, slot_a, slot_b, shape_a, shape_b, device, has_flag=True):
    """fn(ptr_a, ptr_b, accumulate) is a kernel that produces two gradients under ONE accumulate flag, or (has_flag False)
    can only write them.  Where the two destinations agree on a flag the kernel can honour: one call, in place.  Otherwise
    the pair goes through temporaries and ds6g_axpby writes or adds each one."""
    (pa, aa), (pb, ab) = slot_a, slot_b
    if aa == ab and (has_flag or not aa):
        fn(pa, pb, aa)
        return
    ta, tb = (torch.empty(s, dtype=F32, device=device) for s in (shape_a, shape_b))
    fn(ta.data_ptr(), tb.data_ptr(), 0)
    st = ops._stream()
    for t, p, a in ((ta, pa, aa), (tb, pb, ab)):
        ops.lib().axpby(t.data_ptr(), p if a else 0, p, t.numel(), 1.0, 1.0, st)


def layer_backward(mod, ws, reverse, Bsz, L, tape, params, dout2, du_out=None, gdst=None):
    """-> (du [B*L, d_model], the nine parameter gradients in Mamba._params() order).  du_out: an existing gradient of the
    layer's input that du is ADDED to (the in_proj data-gradient GEMM accumulates into it).  gdst: nine (device pointer,
    accumulate flag) pairs in the same order - the gradients are written there in place (added where the flag is set) and
    None is returned in their stead; the conv and scan kernels have no accumulate flag, so a set flag takes those four
    through a temporary and an add, a fresh gradient (the training case) does not."""
    u2, xz, xc, x_dbl, dt, draw, y, saved = tape
    w_in, conv_w, conv_b, w_x, w_dt, b_dt, A_log, Dp, w_out = params
    M, D, r, dm = Bsz * L, mod.d_inner, mod.dt_rank, mod.d_model
    dev = dout2.device

    def empty(*shape):
        return torch.empty(shape, dtype=F32, device=dev)

    shapes = ((2 * D, dm), (D, 1, 4), (D,), (r + 32, D), (D, r), (D,), (D, 16), (D,), (dm, D))
    (s_in, s_cw, s_cb, s_x, s_dtw, s_dtb, s_A, s_D, s_out), grads = grad_slots(shapes, dev, gdst)

    ops.linear_wgrad(y, dout2, s_out[0], ws, accumulate=bool(s_out[1]))
    dy = ops.linear_dgrad(dout2, w_out.data_ptr(), D)
    dxz, dxdbl, dxc, ddraw = empty(M, 2 * D), empty(M, r + 32), empty(M, D), empty(M, D)

    def scan(pa, pd, _acc):
        ops.selective_scan_bwd(xc, draw, b_dt, A_log, x_dbl[:, r:r + 16], x_dbl[:, r + 16:], Dp, xz[:, D:], dy, saved, dxc,
                               ddraw, dxdbl[:, r:r + 16], dxdbl[:, r + 16:], dxz[:, D:], Bsz, L, ws, reverse, out=(pa, pd))
    deliver_pair(scan, s_A, s_D, shapes[6], shapes[7], dev, has_flag=False)
    deliver_pair(lambda pw, pb, acc: ops.linear_wgrad(dt, ddraw, pw, ws, accumulate=bool(acc), dbias_ptr=pb), s_dtw, s_dtb,
                 shapes[4], shapes[5], dev)
    ops.copy_cols(ops.linear_dgrad(ddraw, w_dt.data_ptr(), r), dxdbl[:, :r])
    ops.linear_wgrad(xc, dxdbl, s_x[0], ws, accumulate=bool(s_x[1]))
    ops.linear_dgrad(dxdbl, w_x.data_ptr(), D, out=dxc, accumulate=True)

    def conv(pw, pb, _acc):
        ops.causal_conv1d_silu_bwd(xz[:, :D], conv_w, conv_b, dxc, dxz[:, :D], Bsz, L, ws, reverse, out=(pw, pb))
    deliver_pair(conv, s_cw, s_cb, shapes[1], shapes[2], dev, has_flag=False)
    ops.linear_wgrad(u2, dxz, s_in[0], ws, accumulate=bool(s_in[1]))
    if du_out is None:
        du = ops.linear_dgrad(dxz, w_in.data_ptr(), dm)
    else:
        du = ops.linear_dgrad(dxz, w_in.data_ptr(), dm, out=du_out, accumulate=True)
    return du, grads


class _MambaFn(torch.autograd.Function):
    """forward + backward of the whole layer; inputs after `reverse` are the nine parameters in _PARAMS order"""

    @staticmethod
    def forward(ctx, mod, reverse, save, u, *params):
        Bsz, L, dm = u.shape
        ws = mod._workspace(u.device, Bsz, L)
        u2 = u.detach().reshape(Bsz * L, dm).contiguous()
        out, tape = layer_forward(mod, ws, reverse, save, u2, Bsz, L, params)
        if save:
            ctx.mod, ctx.reverse, ctx.dims = mod, reverse, (Bsz, L, dm)
            ctx.save_for_backward(*tape, *params)
        return out.view(Bsz, L, dm)

    @staticmethod
    def backward(ctx, dout):
        tape, params = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        mod, reverse = ctx.mod, ctx.reverse
        Bsz, L, dm = ctx.dims
        ws = mod._workspace(dout.device, Bsz, L)
        dout2 = dout.reshape(Bsz * L, dm).contiguous()
        du, grads = layer_backward(mod, ws, reverse, Bsz, L, tape, params, dout2)
        return (None, None, None, du.view(Bsz, L, dm), *grads)


class Mamba(nn.Module):
    """mamba_ssm.Mamba's constructor keywords, parameter names, shapes and initialisation"""

    def __init__(self, d_model, d_state=16, d_conv=4, expand=2, dt_rank="auto", dt_min=0.001, dt_max=0.1, dt_init="random",
                 dt_scale=1.0, dt_init_floor=1e-4, conv_bias=True, bias=False, use_fast_path=True, layer_idx=None,
                 device=None, dtype=None):
        super().__init__()
        d_inner = int(expand * d_model)
        r = math.ceil(d_model / 16) if dt_rank == "auto" else int(dt_rank)
        if d_state != 16:
            raise ValueError(f"Mamba: d_state must be 16 (the scan kernels map one state per lane of a 16-lane row), got {d_state}")
        if d_conv != 4:
            raise ValueError(f"Mamba: d_conv must be 4, got {d_conv}")
        if d_model <= 0 or d_model % 64 != 0:
            raise ValueError(f"Mamba: d_model must be a positive multiple of 64, got {d_model}")
        if d_inner <= 0 or d_inner % 128 != 0:
            raise ValueError(f"Mamba: expand * d_model must be a multiple of 128, got {d_inner}")
        if r <= 0 or r % 4 != 0:
            raise ValueError(f"Mamba: dt_rank must be a positive multiple of 4, got {r}")
        if bias:
            raise ValueError("Mamba: bias=True (in_proj / out_proj bias) is not supported")
        if not conv_bias:
            raise ValueError("Mamba: conv_bias=False is not supported")
        if dtype not in (None, F32):
            raise ValueError(f"Mamba: fp32 only, got dtype {dtype}")
        if dt_init not in ("random", "constant"):
            raise ValueError(f"Mamba: dt_init must be 'random' or 'constant', got {dt_init!r}")
        self.d_model, self.d_state, self.d_conv, self.expand = d_model, d_state, d_conv, expand
        self.d_inner, self.dt_rank, self.layer_idx = d_inner, r, layer_idx
        kw = dict(device=device, dtype=F32)
        self.in_proj = nn.Linear(d_model, 2 * d_inner, bias=False, **kw)
        self.conv1d = nn.Conv1d(d_inner, d_inner, d_conv, groups=d_inner, padding=d_conv - 1, bias=True, **kw)
        self.x_proj = nn.Linear(d_inner, r + 2 * d_state, bias=False, **kw)
        self.dt_proj = nn.Linear(r, d_inner, bias=True, **kw)
        std = r ** -0.5 * dt_scale
        with torch.no_grad():
            if dt_init == "constant":
                self.dt_proj.weight.fill_(std)
            else:
                self.dt_proj.weight.uniform_(-std, std)
            dt = torch.exp(torch.rand(d_inner, **kw) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min))
            dt = dt.clamp(min=dt_init_floor)
            self.dt_proj.bias.copy_(dt + torch.log(-torch.expm1(-dt)))   # softplus^-1(dt)
        self.dt_proj.bias._no_reinit = True
        A = torch.arange(1, d_state + 1, **kw).repeat(d_inner, 1)
        self.A_log = nn.Parameter(torch.log(A))
        self.A_log._no_weight_decay = True
        self.D = nn.Parameter(torch.ones(d_inner, **kw))
        self.D._no_weight_decay = True
        self.out_proj = nn.Linear(d_inner, d_model, bias=False, **kw)
        self._ws = {}   # raw stream handle -> ops.Workspace (per instance; stream order makes the reuse safe)

    def workspace_bytes(self, B, L):
        from ._lib import lib
        D = self.d_inner
        return max(int(lib().selective_scan_workspace_bytes(B, L, D)), int(lib().causal_conv1d_workspace_bytes(B, L, D)),
                   _MIN_WS)

    def _workspace(self, device, B, L):
        need = self.workspace_bytes(B, L)
        key = (device.index, ops._stream())
        ws = self._ws.get(key)
        if ws is None or ws.nbytes < need:
            self._ws[key] = ws = ops.Workspace(device, need)
        return ws

    def _params(self):
        return (self.in_proj.weight, self.conv1d.weight, self.conv1d.bias, self.x_proj.weight, self.dt_proj.weight,
                self.dt_proj.bias, self.A_log, self.D, self.out_proj.weight)

    def forward(self, hidden_states, reverse=False):
        """hidden_states: (B, L, d_model) fp32 on the HIP device -> (B, L, d_model)"""
        u = hidden_states
        if not u.is_cuda:
            raise RuntimeError("deepsense6g_tii_amd.Mamba runs on MI355X HIP kernels only (no CPU path)")
        if u.dim() != 3 or u.shape[2] != self.d_model or u.dtype != F32 or u.shape[0] < 1 or u.shape[1] < 1:
            raise ValueError(f"Mamba: expected a (B, L, {self.d_model}) fp32 tensor, got {tuple(u.shape)} {u.dtype}")
        params = self._params()
        for p in params:
            if p.device != u.device:
                raise RuntimeError("Mamba: parameters and input must be on the same HIP device")
            if p.dtype != F32 or not p.is_contiguous():
                raise ValueError("Mamba: parameters must be contiguous fp32 tensors")
        save = torch.is_grad_enabled() and self.training and (u.requires_grad or any(p.requires_grad for p in params))
        with torch.cuda.device(u.device):
            if save:
                return _MambaFn.apply(self, bool(reverse), True, u, *params)
            with torch.no_grad():   # inference: no checkpoints, no graph
                return _MambaFn.apply(self, bool(reverse), False, u, *params)
