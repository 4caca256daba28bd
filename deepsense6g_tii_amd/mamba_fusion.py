"""The bi-branch Mamba fusion stage of the reference (mambafuser_seq.py:74-231) on the gfx950 kernels: MambaBlock and
MambaFusion, drop-in nn.Modules (fp32 parameters) whose state dicts are interchangeable with the reference's.

    MambaBlock      x1  = fc1(ln1(x))                    ln1 = LayerNorm((T, C)): one mean / variance per SAMPLE
                    fm  = forward_mamba(x1)
                    xf  = flip(x1, 1);  bm = backward_mamba(xf)
                    out = bm * LeakyReLU_0.2(fc2(xf)) + fm * bm
    There is no residual, and bm and fc2(xf) are never flipped back: token t of the output pairs fm[t] with the reversed
    branch at L-1-t.  Here bmN = backward_mamba(x1, reverse=True) and f2N = fc2(x1) stay in natural order and the gate kernel
    reads them back to front (out[b, t] = bmN[b, L-1-t] * (leaky(f2N[b, L-1-t]) + fm[b, t])): no flip copy, forward or backward.

    MambaFusion     tokens = drop(pos_emb + cat(channel-swapped image / lidar / radar tokens, gps))
                    tokens = ln_f(mambablocks(tokens));  unpack to the three NCHW maps and the two gps rows
    Token rows are modality-major (image, lidar, radar; then frame, h, w), the gps rows last.  Token channel c of modality m
    comes from modality (m + seg(c)) % 3, seg = 0 / 1 / 2 for c < C//3, c < C//3*2, the rest.

One block is ONE autograd node: the three gradients that reach x1 (forward Mamba, reverse Mamba, fc2) are summed by the
data-gradient GEMMs accumulating into one buffer, not by autograd.  The LayerNorm, gate, pack and unpack are
csrc/mamba_fusion.hip, the two Mamba layers csrc/mamba.hip (mamba.layer_forward / layer_backward), fc1 / fc2 the fp32
implicit-GEMM linears, ln_f the row LayerNorm kernel.

The node's body is the pair block_forward / block_backward, plain functions with an explicit tape; block_backward (like
mamba.layer_backward) can write the parameter gradients in place through (device pointer, accumulate flag) destinations.
stage_forward / stage_backward (end of the file) are the whole stage on a model walk's conventions: NHWC maps at full
resolution, the caller's workspace, gradients into the caller's arena, the pool-swap pack of csrc/mamba_fusion.hip in place
of pooling + swap_pack.

Initialisation follows the reference's self.apply(_init_weights) to the letter: EVERY nn.Linear under the stage is redrawn
N(0, 0.02) with a zero bias - also the four inside each Mamba, so dt_proj.bias ends up 0 and dt_proj.weight loses its
dt_rank**-0.5 scale - LayerNorm is (1, 0) and pos_emb zeros; A_log, D and conv1d keep the Mamba layer's own initialisation.
That is not what mamba_ssm intends for dt_proj (its _no_reinit mark is not honoured by the reference's hook), and it is what
the reference trains.

Storage: the dtype of a block's input (fp32, bf16 or f16), or of the stage's maps, is the type the wide activations are stored
in.  block_forward / block_backward and stage_forward / stage_backward state the launch sequence once; the
sample LayerNorm, gate and pool-swap wrappers pick their entry point by operand dtype, and the storage decides only which
linear triple runs (ops.linear_* / ops.bf16_linear_*), where the fc1 / fc2 weights come from (the masters / 16-bit copies:
block_weight_copies16, or the caller's w16=), the dtype of dx1 and one extra cast (block: dx1 to 16-bit; stage: the ln_f input
to fp32).  On 16-bit storage:

    tensor                                                        storage
    block input x, xl = ln1 output, x1, fm, bm, f2, block output  16-bit
    dout, dfm, dbm, df2, dxl, block dx                            16-bit
    dx1 (fc2's data gradient + the two layers' input gradients)   fp32 while it accumulates (bf16_linear_dgrad(out16=False),
                                                                  then du_out=), then ONE 16-bit copy (ops.cast_bf16) that
                                                                  fc1's weight and data gradients read
    ln1 mean / rstd, its double partials, every parameter and     fp32 / double as on fp32 storage
    parameter gradient, gdst= destinations
    fc1 / fc2 weights                                             16-bit copies, forward and data gradient; biases fp32
    stage: the three NHWC maps in and out, their gradients        the walk's storage (16-bit)
    stage: tokens out of the pack, the gradient into its backward 16-bit
    stage: gemb, dgemb, pos_emb, dpos_emb                         fp32
    stage: ln_f input (widened once: ops.cast_f32), xo (the       fp32; ln_f's backward is ops.layernorm_bwd_bf16, whose second
    returned tokens), dxo                                         output is the 16-bit dx the last block reads
The two Mamba layers inside a block follow mamba.py's map.  Without a caller's w16= the stage casts every block's weights once
in the forward and carries the copies on its tape; a MambaBlock module casts on every call, as Mamba does.

Supported: fp32 / bf16 / f16 activations for MambaBlock and the walk-form stage, fp32 only for the MambaFusion module (its NCHW
pack / unpack kernels are fp32); HIP device only, n_embd in {64, 128, 256, 512}, d_state 16, d_conv 4, 8 x 8 anchors,
config.n_views == 1 (the reference's cat of the three modalities only lines up then), ln_size == (T, n_embd).  Train and eval;
dropout is off in eval; no tape is kept when no gradient is needed.  Not covered: 16-bit storage of the MambaFusion module
form and of the head (TimeMamba, time_mamba.py; the model, MambaFuser of mamba_fuser.py, runs the walk-form stage on 16-bit
storage and keeps the head fp32), missing-modality options.

Frozen form (block_forward_frozen / stage_forward_frozen, end of the file): the stage of a frozen model
(mamba_infer.MambaFuserEngine), forward only and without a tape, on operands the engine prepared once - the three GEMMs that
read x1 as ONE GEMM on a [9C, C] weight (cat9_layout), the two directions' convs and scans as one grouped launch each
(csrc/mamba_infer.hip) with dt_proj inside the scan.  The activations follow the storage map above.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops
from .mamba import (Mamba, _check_params, deliver_pair, grad_slots, layer_forward, layer_backward, stream_workspace,
                    weight_copies16, x_proj_rows16)

F32 = torch.float32


def _empty(dev, *shape):
    return torch.empty(shape, dtype=F32, device=dev)


def block_weight_copies16(blk, params, dtype):
    """-> the `w16` of block_forward / block_backward: (device pointer of the 16-bit fc1.weight copy, of the fc2.weight copy,
    the forward Mamba's weight_copies16 pointers, the reverse Mamba's), cast from the fp32 masters now; the tensors ride along
    so the pointers stay valid"""
    c1, c2 = ops.cast_bf16(params[2], dtype=dtype), ops.cast_bf16(params[4], dtype=dtype)
    pf, tf = weight_copies16(blk.forward_mamba, params[6:15], dtype)
    pb, tb = weight_copies16(blk.backward_mamba, params[15:24], dtype)
    return (c1.data_ptr(), c2.data_ptr(), pf, pb), (c1, c2, *tf, *tb)


def block_forward(blk, ws, save, x2, B, T, params, w16=None):
    """one MambaBlock on x2 [B, T * C] (contiguous) -> (out [B * T, C], tape or None).  `params`: the 24 parameters in
    MambaBlock._params() order; `ws`: a Workspace of at least blk.workspace_bytes(B, T).  The body of _BlockFn, and what a
    model walk calls without autograd.
    x2's dtype is the storage type (the map of the module docstring), and `out`'s.  w16 (16-bit storage only): the pointers
    block_weight_copies16 returns, for a caller that keeps 16-bit weight copies of its own; None casts the weights here, on
    every call."""
    ln_w, ln_b, w1, b1, w2, b2 = params[:6]
    mp = params[6:]
    C = blk.n_embd
    M = B * T
    if x2.dtype == F32:
        linear, (p1, p2, w16_f, w16_b) = ops.linear_fwd, (w1.data_ptr(), w2.data_ptr(), None, None)
    else:
        if w16 is None:
            w16, _alive = block_weight_copies16(blk, params, x2.dtype)   # _alive: until the launches below are queued
        linear, (p1, p2, w16_f, w16_b) = ops.bf16_linear_fwd, w16
    xl, mean, rstd = ops.sample_layernorm_fwd(x2, ln_w, ln_b, ws)
    x1 = linear(xl.view(M, C), p1, b1.data_ptr(), C)
    fm, tape_f = layer_forward(blk.forward_mamba, ws, False, save, x1, B, T, mp[:9], w16=w16_f)
    bm, tape_b = layer_forward(blk.backward_mamba, ws, True, save, x1, B, T, mp[9:], w16=w16_b)
    f2 = linear(x1, p2, b2.data_ptr(), C)
    out = ops.bimamba_gate_fwd(fm, bm, f2, B, T)
    return out, ((x2, mean, rstd, xl, fm, bm, f2, *tape_f, *tape_b) if save else None)


def block_backward(blk, ws, tape, dout2, B, T, params, gdst=None, w16=None):
    """dout2 [B * T, C] (contiguous) -> (dx [B, T * C], the 24 parameter gradients in MambaBlock._params() order).  gdst: 24
    (device pointer, accumulate flag) pairs in that order - the gradients are written there in place and None is returned in
    their stead (mamba.layer_backward's convention).
    dout2's dtype is the storage type, the one of the forward that made the tape, and dx's; the parameter gradients and gdst
    are fp32; w16 as in block_forward."""
    x2, mean, rstd, xl, fm, bm, f2 = tape[:7]
    tape_f, tape_b = tape[7:15], tape[15:23]
    ln_w, w1, w2, mp = params[0], params[2], params[4], params[6:]
    C = blk.n_embd
    M, dev, st = B * T, dout2.device, dout2.dtype
    h16 = st != F32
    if not h16:
        wgrad, dgrad, dx1_kw = ops.linear_wgrad, ops.linear_dgrad, {}
        p1, p2, w16_f, w16_b = w1.data_ptr(), w2.data_ptr(), None, None
    else:
        if w16 is None:
            w16, _alive = block_weight_copies16(blk, params, st)   # _alive: until the launches below are queued
        wgrad, dgrad, dx1_kw = ops.bf16_linear_wgrad, ops.bf16_linear_dgrad, dict(out16=False)
        p1, p2, w16_f, w16_b = w16
    shapes = ((T, C), (T, C), (C, C), (C,), (C, C), (C,))
    (s_lw, s_lb, s_w1, s_b1, s_w2, s_b2), own = grad_slots(shapes, dev, None if gdst is None else gdst[:6])
    x1 = tape_f[0]
    dfm, dbm, df2 = ops.bimamba_gate_bwd(dout2, fm, bm, f2, B, T)
    deliver_pair(lambda pw, pb, acc: wgrad(x1, df2, pw, ws, accumulate=bool(acc), dbias_ptr=pb), s_w2, s_b2,
                 shapes[4], shapes[5], dev)
    # dx1 is fp32 on every storage while fc2's data gradient and the two Mamba layers' input gradients are summed into it
    dx1 = dgrad(df2, p2, C, **dx1_kw)
    _, g_f = layer_backward(blk.forward_mamba, ws, False, B, T, tape_f, mp[:9], dfm, du_out=dx1,
                            gdst=None if gdst is None else gdst[6:15], w16=w16_f)
    _, g_b = layer_backward(blk.backward_mamba, ws, True, B, T, tape_b, mp[9:], dbm, du_out=dx1,
                            gdst=None if gdst is None else gdst[15:24], w16=w16_b)
    dx1_st = ops.cast_bf16(dx1, dtype=st) if h16 else dx1       # 16-bit: ONE rounding of the sum, read by fc1's two GEMMs
    deliver_pair(lambda pw, pb, acc: wgrad(xl.view(M, C), dx1_st, pw, ws, accumulate=bool(acc), dbias_ptr=pb), s_w1,
                 s_b1, shapes[2], shapes[3], dev)
    dxl = dgrad(dx1_st, p1, C)
    dx = None

    def ln1_bwd(pw, pb, acc):
        nonlocal dx
        dx = ops.sample_layernorm_bwd(dxl.view(B, T * C), x2, mean, rstd, ln_w, pw, pb, ws, accumulate=bool(acc))
    deliver_pair(ln1_bwd, s_lw, s_lb, shapes[0], shapes[1], dev)
    return dx, (None if gdst is not None else (*own, *g_f, *g_b))


class _BlockFn(torch.autograd.Function):
    """the whole MambaBlock; inputs after x: ln1.weight, ln1.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, the nine
    parameters of forward_mamba, the nine of backward_mamba"""

    @staticmethod
    def forward(ctx, blk, save, x, *params):
        B, T, C = x.shape
        ws = blk._workspace(x.device, B, T)
        out, tape = block_forward(blk, ws, save, x.detach().reshape(B, T * C).contiguous(), B, T, params)
        if save:
            ctx.blk, ctx.dims = blk, (B, T, C)
            ctx.save_for_backward(*tape, *params)
        return out.view(B, T, C)

    @staticmethod
    def backward(ctx, dout):
        st = ctx.saved_tensors
        blk = ctx.blk
        B, T, C = ctx.dims
        ws = blk._workspace(dout.device, B, T)
        dx, grads = block_backward(blk, ws, st[:23], dout.reshape(B * T, C).contiguous(), B, T, st[23:])
        return (None, None, dx.view(B, T, C), *grads)


class MambaBlock(nn.Module):
    """a bi-branch Mamba block: the reference's constructor arguments, parameter names and shapes"""

    def __init__(self, n_embd, ln_size, d_state, d_conv, expand, device=None):
        super().__init__()
        ln_size = tuple(int(v) for v in ln_size)
        if len(ln_size) != 2 or ln_size[1] != n_embd or ln_size[0] < 1:
            raise ValueError(f"MambaBlock: ln_size must be (T, {n_embd}), got {ln_size}")
        kw = dict(device=device, dtype=F32)
        self.n_embd, self.ln_size = n_embd, ln_size
        self.ln1 = nn.LayerNorm(ln_size, **kw)       # parameter holders: the arithmetic is the HIP kernels'
        self.fc1 = nn.Linear(n_embd, n_embd, **kw)
        self.fc2 = nn.Linear(n_embd, n_embd, **kw)
        self.forward_mamba = Mamba(d_model=n_embd, d_state=d_state, d_conv=d_conv, expand=expand, device=device)
        self.backward_mamba = Mamba(d_model=n_embd, d_state=d_state, d_conv=d_conv, expand=expand, device=device)
        self._ws = {}

    def workspace_bytes(self, B, T):
        return max(self.forward_mamba.workspace_bytes(B, T), ops.sample_layernorm_workspace_bytes(B, T * self.n_embd))

    def _workspace(self, device, B, T):
        return stream_workspace(self._ws, device, self.workspace_bytes(B, T))

    def _params(self):
        return (self.ln1.weight, self.ln1.bias, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias,
                *self.forward_mamba._params(), *self.backward_mamba._params())

    def _check(self, x):
        if not x.is_cuda:
            raise RuntimeError("deepsense6g_tii_amd.MambaBlock runs on MI355X HIP kernels only (no CPU path)")
        if x.dim() != 3 or tuple(x.shape[1:]) != self.ln_size or x.dtype not in (F32, ops.BF16, ops.F16) or x.shape[0] < 1:
            raise ValueError(f"MambaBlock: expected a (B, {self.ln_size[0]}, {self.ln_size[1]}) fp32, bf16 or f16 tensor, got "
                             f"{tuple(x.shape)} {x.dtype}")
        params = self._params()
        _check_params("MambaBlock", params, x.device)
        return params

    def forward(self, x):
        """x: (B, T, n_embd) fp32, bf16 or f16 on the HIP device, (T, n_embd) == ln_size -> (B, T, n_embd) of the same dtype.
        A 16-bit input runs the 16-bit-storage path (module docstring): its gradient is 16-bit, the parameters and their
        gradients fp32, the weight copies are cast on every call"""
        params = self._check(x)
        save = torch.is_grad_enabled() and self.training and (x.requires_grad or any(p.requires_grad for p in params))
        with torch.cuda.device(x.device):
            if save:
                return _BlockFn.apply(self, True, x, *params)
            with torch.no_grad():
                return _BlockFn.apply(self, False, x, *params)


class _PackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, B, S, drop, image, lidar, radar, gps, pos_emb):
        ctx.args = (B, S, drop)
        return ops.swap_pack_fwd(image.detach().contiguous(), lidar.detach().contiguous(), radar.detach().contiguous(),
                                 gps.detach().contiguous(), pos_emb, B, S, *drop)

    @staticmethod
    def backward(ctx, dtok):
        B, S, drop = ctx.args
        di, dl, dr, dg, dpos = ops.swap_pack_bwd(dtok.contiguous(), B, S, *drop)
        return None, None, None, di, dl, dr, dg, dpos.unsqueeze(0)


class _LnFFn(torch.autograd.Function):
    """ln_f = LayerNorm(C) over token rows, on the row kernel"""

    @staticmethod
    def forward(ctx, mod, save, x, w, b):
        B, T, C = x.shape
        x2 = x.detach().reshape(B * T, C).contiguous()
        y, mean, rstd = ops.layernorm_fwd(x2, w.data_ptr(), b.data_ptr())
        if save:
            ctx.mod, ctx.dims = mod, (B, T, C)
            ctx.save_for_backward(x2, mean, rstd, w)
        return y.view(B, T, C)

    @staticmethod
    def backward(ctx, dy):
        x2, mean, rstd, w = ctx.saved_tensors
        B, T, C = ctx.dims
        ws = ctx.mod.mambablocks[0]._workspace(dy.device, B, T)
        g_w, g_b = _empty(dy.device, C), _empty(dy.device, C)
        dx = ops.layernorm_bwd(dy.reshape(B * T, C).contiguous(), x2, mean, rstd, w.data_ptr(), g_w.data_ptr(), g_b.data_ptr(),
                               ws)
        return None, None, dx.view(B, T, C), g_w, g_b


class _UnpackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, B, S, tokens):
        ctx.args = (B, S)
        return ops.token_unpack_fwd(tokens.detach().contiguous(), B, S)

    @staticmethod
    def backward(ctx, di, dl, dr, dg):
        B, S = ctx.args
        return None, None, ops.token_unpack_bwd(di.contiguous(), dl.contiguous(), dr.contiguous(), dg.contiguous(), B, S)


class MambaFusion(nn.Module):
    """the reference's MambaFusion: constructor arguments, forward signature, state-dict names and initialisation"""

    def __init__(self, n_embd, ln_size, d_state, d_conv, expand, n_layer, vert_anchors, horz_anchors, seq_len, embd_pdrop,
                 config, device=None):
        super().__init__()
        if getattr(config, "n_views", 1) != 1:
            raise ValueError(f"MambaFusion: config.n_views must be 1 (the reference's token cat only lines up then), got "
                             f"{config.n_views}")
        if vert_anchors != 8 or horz_anchors != 8:
            raise ValueError(f"MambaFusion: 8 x 8 anchors only, got {vert_anchors} x {horz_anchors}")
        if n_embd not in (64, 128, 256, 512):
            raise ValueError(f"MambaFusion: n_embd must be 64, 128, 256 or 512, got {n_embd}")
        if seq_len < 1 or n_layer < 1:
            raise ValueError(f"MambaFusion: seq_len and n_layer must be positive, got {seq_len}, {n_layer}")
        if not 0.0 <= float(embd_pdrop) < 1.0:
            raise ValueError(f"MambaFusion: embd_pdrop must be in [0, 1), got {embd_pdrop}")
        T = 3 * seq_len * 64 + 2
        if tuple(int(v) for v in ln_size) != (T, n_embd):
            raise ValueError(f"MambaFusion: ln_size must be ({T}, {n_embd}) for seq_len {seq_len}, got {tuple(ln_size)}")
        self.n_embd, self.seq_len, self.vert_anchors, self.horz_anchors, self.config = n_embd, seq_len, 8, 8, config
        self.embd_pdrop, self.n_tokens, self.block_size = float(embd_pdrop), T, seq_len
        self.pos_emb = nn.Parameter(torch.zeros(1, T, n_embd, device=device, dtype=F32))
        self.mambablocks = nn.Sequential(*[MambaBlock(n_embd, ln_size, d_state, d_conv, expand, device=device)
                                           for _ in range(n_layer)])
        self.ln_f = nn.LayerNorm(n_embd, device=device, dtype=F32)
        self.apply(self._init_weights)
        self._seed = int(torch.randint(0, 2 ** 31 - 1, ()).item())
        self._seed_off = 0

    def get_block_size(self):
        return self.block_size

    @staticmethod
    def _init_weights(module):
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.LayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)

    def set_dropout_seed(self, seed):
        """embd_drop masks are a pure function of (seed, counter): restart the counter under this seed.  Without a call the
        seed is one draw from torch's CPU generator at construction (so torch.manual_seed fixes it)"""
        self._seed, self._seed_off = int(seed), 0

    def forward(self, image_tensor, lidar_tensor, radar_tensor, gps):
        """image / lidar / radar: (B * seq_len, n_embd, 8, 8), gps: (B, 2, n_embd), fp32 on the HIP device ->
        (image_out, lidar_out, radar_out) of the input shapes and the two gps token rows (B, 2, n_embd)"""
        S, C, T = self.seq_len, self.n_embd, self.n_tokens
        ins = (image_tensor, lidar_tensor, radar_tensor, gps)
        for t in ins:
            if not t.is_cuda:
                raise RuntimeError("deepsense6g_tii_amd.MambaFusion runs on MI355X HIP kernels only (no CPU path)")
        dev = lidar_tensor.device
        B = lidar_tensor.shape[0] // S
        for t in ins[:3]:
            if tuple(t.shape) != (B * S, C, 8, 8) or t.dtype != F32 or t.device != dev or B < 1:
                raise ValueError(f"MambaFusion: expected three (B * {S}, {C}, 8, 8) fp32 maps, got {tuple(t.shape)} {t.dtype}")
        if tuple(gps.shape) != (B, 2, C) or gps.dtype != F32 or gps.device != dev:
            raise ValueError(f"MambaFusion: expected gps of shape ({B}, 2, {C}) fp32, got {tuple(gps.shape)} {gps.dtype}")
        params = (self.pos_emb, self.ln_f.weight, self.ln_f.bias)
        _check_params("MambaFusion", params, dev)
        bparams = [blk._params() for blk in self.mambablocks]
        for bp in bparams:
            _check_params("MambaFusion", bp, dev)
        needs = any(t.requires_grad for t in ins) or any(p.requires_grad for p in params) or \
            any(p.requires_grad for bp in bparams for p in bp)
        save = torch.is_grad_enabled() and self.training and needs
        p = self.embd_pdrop if self.training else 0.0
        drop = (p, self._seed, self._seed_off)
        if p > 0.0:
            self._seed_off += B * T * C          # the next training forward draws from the next counter range
        with torch.cuda.device(dev), torch.set_grad_enabled(save):
            x = _PackFn.apply(B, S, drop, image_tensor, lidar_tensor, radar_tensor, gps, self.pos_emb)
            for blk, bp in zip(self.mambablocks, bparams):
                x = _BlockFn.apply(blk, save, x, *bp)
            x = _LnFFn.apply(self, save, x, self.ln_f.weight, self.ln_f.bias)
            return _UnpackFn.apply(B, S, x)


# ---- the stage on a model walk's conventions ---------------------------------------------------------------------------
# The walk keeps the three modality maps NHWC [B * S, H, H, C] at full resolution and owns every buffer, the scratch and
# the gradient destinations.  stage_forward / stage_backward are MambaFusion.forward without autograd on those conventions:
# the pool-swap pack (csrc/mamba_fusion.hip) in place of adaptive pooling + swap_pack, the blocks, ln_f on the row kernel,
# and the grouped upsample-add of the GPT stages in place of unpack + interpolate + add (the unpack does not undo the swap,
# so that kernel is right as it stands; at H = 8 its weights are exactly 1 and it is the plain add).
def stage_workspace_bytes(fus, B):
    return fus.mambablocks[0].workspace_bytes(B, fus.n_tokens)


def _stage_ws(fus, ws, B):
    need = stage_workspace_bytes(fus, B)
    if ws.nbytes < need:
        raise ValueError(f"Mamba stage: the workspace has {ws.nbytes} bytes, B = {B} needs {need}")


def stage_forward(fus, ws, save, feats, gemb, outs, B, drop=(0.0, 0, 0), w=None, w16=None):
    """feats: the three NHWC maps [B * S, H, H, C]; gemb [B, 2, C]: the embedded gps rows; outs: three maps like feats that
    receive feats[m] + the bilinear upsampling of modality m's output tokens; drop = (p, seed, seed_off) of the embedding
    dropout; w(p): device pointer of parameter p (default: where p.data lives).  -> (tokens after ln_f [B * T, C], tape or
    None).
    feats[0].dtype is the storage type (fp32, bf16 or f16) of the maps, the tokens and the blocks; gemb, the pos_emb add and
    the returned tokens are fp32 on every storage.  w16 (16-bit storage): one block_weight_copies16 pointer tuple per block,
    for a caller that keeps the copies; None casts every block's weights once here and carries the copies on the tape, so the
    backward does not cast again."""
    _stage_ws(fus, ws, B)
    w = w or (lambda p: p.data_ptr())
    S, C, T = fus.seq_len, fus.n_embd, fus.n_tokens
    st = feats[0].dtype
    h16 = st != F32
    x = torch.empty((B, T, C), dtype=st, device=gemb.device)
    ops.pool_swap_tokens_fwd(feats, gemb, w(fus.pos_emb), x, S, *drop)
    x = x.view(B, T * C)
    alive = None
    if h16 and w16 is None:
        made = [block_weight_copies16(blk, blk._params(), st) for blk in fus.mambablocks]
        w16, alive = [m[0] for m in made], [m[1] for m in made]
    tapes = []
    for i, blk in enumerate(fus.mambablocks):
        x, tp = block_forward(blk, ws, save, x.view(B, T * C), B, T, blk._params(), w16=w16[i] if h16 else None)
        tapes.append(tp)
    x = x.view(B * T, C)
    if h16:
        x = ops.cast_f32(x)                                        # ln_f reads the last block's output widened once
    xo, mf, rf = ops.layernorm_fwd(x, w(fus.ln_f.weight), w(fus.ln_f.bias), fus.ln_f.eps)
    ops.upsample_add_fwd3(feats, xo, outs, (S, S, S), (0, S * 64, 2 * S * 64), T)
    return xo, ((tapes, x, mf, rf, drop, (st, w16, alive)) if save else None)


def stage_backward(fus, ws, tape, dfeats_out, dgps_tok, dfeats, dgemb, B, g, w=None):
    """dfeats_out: gradients of the three output maps; dgps_tok = (tensor, bcast): gradient of the two gps rows of the
    stage's output tokens, [B, 2, C] or (bcast) one [B, C] row for both; g(p) -> (device pointer, accumulate flag) of
    parameter p's gradient.  Writes dfeats (three maps: dfeats_out[m] + the pooled-token gradient; may be dfeats_out
    themselves) and dgemb [B, 2, C]; every parameter gradient of the stage goes to its g(p).
    The storage type is the forward's (dfeats_out and dfeats have it; dgps_tok, dgemb and every parameter gradient are fp32);
    the 16-bit weight copies are the ones the forward used."""
    _stage_ws(fus, ws, B)
    w = w or (lambda p: p.data_ptr())
    tapes, x_last, mf, rf, drop, (st, w16, _alive) = tape
    h16 = st != F32
    S, C, T = fus.seq_len, fus.n_embd, fus.n_tokens
    dxo = torch.empty((B * T, C), dtype=F32, device=dgemb.device)
    ops.upsample_add_bwd3(dfeats_out, dxo, (S, S, S), (0, S * 64, 2 * S * 64), T)
    gsrc, bcast = dgps_tok
    ops.lib().gps_rows(gsrc.data_ptr(), dxo.data_ptr(), B, C, T, 1, 0, int(bcast), ops._stream())
    (gfw, af), (gfb, ab) = g(fus.ln_f.weight), g(fus.ln_f.bias)
    assert af == ab, "ln_f.weight and ln_f.bias gradients must share one accumulate flag"
    if h16:     # the row kernel's second output is the 16-bit copy of dx the last block reads
        _, dx = ops.layernorm_bwd_bf16(dxo, x_last, mf, rf, w(fus.ln_f.weight), gfw, gfb, ws, accumulate=bool(af), dtype=st)
    else:
        dx = ops.layernorm_bwd(dxo, x_last, mf, rf, w(fus.ln_f.weight), gfw, gfb, ws, accumulate=bool(af))
    blocks = list(fus.mambablocks)
    for i in reversed(range(len(blocks))):
        blk = blocks[i]
        dx, _ = block_backward(blk, ws, tapes[i], dx.view(B * T, C), B, T, blk._params(), gdst=[g(p) for p in blk._params()],
                               w16=w16[i] if h16 else None)
    gpos, apos = g(fus.pos_emb)
    ops.pool_swap_tokens_bwd(dx.view(B, T, C), dfeats_out, dfeats, dgemb, gpos, apos, S, *drop)


# ---- the stage of a frozen model ----------------------------------------------------------------------------------------
# A frozen model's weights do not change between calls and an inference forward keeps no tape, so the block can take a shape
# the training walk cannot: in_proj of both directions and fc2 all read x1 - ONE GEMM on their weights stacked at freeze time;
# its output `cat` [M, 9C] holds x | z of the forward layer, x | z of the reverse layer and f2 as column blocks that the
# grouped conv, the grouped scan and the gate read in place.
def cat9_layout(C):
    """Pure host function: where the stacked [9C, C] weight (and its [9C] bias, zero but for fc2's) keeps what.  rows: name ->
    (first row, end row) of in_proj.weight of the forward Mamba, of the reverse Mamba, and of fc2.weight / fc2.bias; cols: the
    column blocks of the GEMM's output - a row block of the weight IS a column block of the output: x / z = the halves of each
    in_proj, f2 = fc2's"""
    D = 2 * C
    return SimpleNamespace(n=9 * C, D=D,
                           rows=dict(in_proj_fwd=(0, 2 * D), in_proj_bwd=(2 * D, 4 * D), fc2=(4 * D, 4 * D + C)),
                           cols=dict(x_fwd=(0, D), z_fwd=(D, 2 * D), x_bwd=(2 * D, 3 * D), z_bwd=(3 * D, 4 * D),
                                     f2=(4 * D, 4 * D + C)))


def frozen_plan(C, dtype):
    """Pure host rule: which form each step of a frozen block takes at width C on storage `dtype`, from the measured table
    (profiles/mamba_infer.txt, B = 12, T = 962, new form against what it replaces, both storages):
        grouped conv   wins at every width (1.04x .. 1.27x)                              -> always
        grouped scan   1.40x / 1.18x at C = 64 / 128, level at 256, LOSES at 512 (0.88x:  -> C <= 256; at 512 the layer's own
                       r = 32 there, and the dt_proj prologue costs more than the           sequence per direction (copy_cols,
                       delta_raw round trip it saves)                                        dt_proj GEMM, selective_scan_fwd)
        stacked GEMM   wins at every width on fp32 (1.04x .. 1.44x) and up to C = 256    -> everywhere but 16-bit C = 512: there
                       on 16-bit (1.09x .. 2.5x), LOSES at 16-bit C = 512 (0.94x)           three GEMMs on the row blocks of the
                                                                                             same stacked weight
    -> SimpleNamespace(grouped_scan, stacked_gemm)"""
    return SimpleNamespace(grouped_scan=C <= 256, stacked_gemm=not (C >= 512 and dtype != F32))


def block_forward_frozen(blk, ws, x2, B, T, fz):
    """one MambaBlock of a frozen model on x2 [B, T * C] (contiguous, the storage dtype) -> out [B * T, C] of that dtype.  fz:
    the block's frozen operands, tensors the caller owns: ln_w, ln_b [T, C], fc1_b [C], cat_b [9C] fp32; fc1_w [C, C] and
    cat_w [9C, C] (cat9_layout) in the storage dtype; dirs = (forward, reverse), each with conv_w, conv_b, dt_w, dt_b, A_log, D
    fp32 and x_w [n_x, 2C] (16-bit storage: zero-padded to mamba.x_proj_rows16 rows), out_w [C, 2C] in the storage dtype.
    Six GEMMs, one grouped conv, one grouped scan (three launches), the sample LayerNorm and the gate; no tape, no cast, no
    copy - except where frozen_plan(C, dtype) picks the older form of a step at C = 512, on the measured table."""
    C, M = blk.n_embd, B * T
    D, r = 2 * C, blk.forward_mamba.dt_rank
    if x2.dtype == F32:
        linear, xkw = ops.linear_fwd, {}
    else:
        linear, xkw = ops.bf16_linear_fwd, dict(out16=False)     # fp32 x_dbl from the zero-padded weight
    plan, lay = frozen_plan(C, x2.dtype), cat9_layout(C)
    xl, _, _ = ops.sample_layernorm_fwd(x2, fz.ln_w, fz.ln_b, ws)
    x1 = linear(xl.view(M, C), fz.fc1_w.data_ptr(), fz.fc1_b.data_ptr(), C)
    if plan.stacked_gemm:
        cat = linear(x1, fz.cat_w.data_ptr(), fz.cat_b.data_ptr(), lay.n)
        col = lambda name: cat[:, lay.cols[name][0]:lay.cols[name][1]]  # noqa: E731
    else:                                  # the same weight, one GEMM per row block (frozen_plan has the reason)
        part = {}
        for name, (lo, hi) in lay.rows.items():
            part[name] = linear(x1, fz.cat_w[lo:].data_ptr(), fz.cat_b[lo:].data_ptr() if name == "fc2" else 0, hi - lo)
        src = dict(x_fwd=("in_proj_fwd", 0), z_fwd=("in_proj_fwd", D), x_bwd=("in_proj_bwd", 0), z_bwd=("in_proj_bwd", D),
                   f2=("fc2", 0))
        col = lambda name: part[src[name][0]][:, src[name][1]:src[name][1] + (C if name == "f2" else D)]  # noqa: E731
    df, db = fz.dirs
    xc = ops.mamba_conv_fwd_grouped([(col("x_fwd"), df.conv_w, df.conv_b, False), (col("x_bwd"), db.conv_w, db.conv_b, True)],
                                    B, T)
    x_dbl = [linear(xc[k], d.x_w.data_ptr(), 0, d.x_w.shape[0], **xkw) for k, d in enumerate(fz.dirs)]
    zs = (col("z_fwd"), col("z_bwd"))
    if plan.grouped_scan:
        y = ops.mamba_scan_fwd_grouped([(xc[k], zs[k], x_dbl[k], d.dt_w, d.dt_b, d.A_log, d.D, bool(k))
                                        for k, d in enumerate(fz.dirs)], B, T, r, ws)
    else:                                  # the layer's own sequence per direction (frozen_plan has the reason)
        y = []
        for k, d in enumerate(fz.dirs):
            dt = ops.copy_cols(x_dbl[k][:, :r], torch.empty((M, r), dtype=F32, device=x2.device))
            raw = ops.linear_fwd(dt, d.dt_w.data_ptr(), 0, D)
            y.append(ops.selective_scan_fwd(xc[k], raw, d.dt_b, d.A_log, x_dbl[k][:, r:r + 16], x_dbl[k][:, r + 16:r + 32], d.D,
                                            zs[k], B, T, ws, bool(k), False)[0])
    fm = linear(y[0], df.out_w.data_ptr(), 0, C)
    bm = linear(y[1], db.out_w.data_ptr(), 0, C)
    return ops.bimamba_gate_fwd(fm, bm, col("f2"), B, T)


def stage_forward_frozen(fus, ws, feats, gemb, outs, B, fz):
    """stage_forward for a frozen model: the pool-swap pack without dropout, the frozen blocks, ln_f and the grouped
    upsample-add, as stage_forward runs them.  fz: pos_emb [1, T, C], ln_f_w, ln_f_b [C] fp32 tensors and blocks = one
    block_forward_frozen operand set per block.  -> xo, the tokens after ln_f [B * T, C] fp32"""
    _stage_ws(fus, ws, B)
    S, C, T = fus.seq_len, fus.n_embd, fus.n_tokens
    st = feats[0].dtype
    assert len(fz.blocks) == len(fus.mambablocks)
    assert ws.nbytes >= ops.mamba_scan_fwd_grouped_workspace_bytes(B, T, 2 * C, 2)
    x = torch.empty((B, T, C), dtype=st, device=gemb.device)
    ops.pool_swap_tokens_fwd(feats, gemb, fz.pos_emb.data_ptr(), x, S)
    for blk, bz in zip(fus.mambablocks, fz.blocks):
        x = block_forward_frozen(blk, ws, x.view(B, T * C), B, T, bz)
    x = x.view(B * T, C)
    if st != F32:
        x = ops.cast_f32(x)                                        # ln_f reads the last block's output widened once
    xo, _, _ = ops.layernorm_fwd(x, fz.ln_f_w.data_ptr(), fz.ln_f_b.data_ptr(), fus.ln_f.eps)
    ops.upsample_add_fwd3(feats, xo, outs, (S, S, S), (0, S * 64, 2 * S * 64), T)
    return xo


def freeze_block(blk, dtype=F32):
    """-> the `fz` of block_forward_frozen from the block's parameters as they are now, in fresh tensors: the GEMM weights in
    `dtype` (the storage), everything else fp32.  For a block on its own (tests, tools); the engine of a whole model
    (mamba_infer.MambaFuserEngine) lays the same operands out in the snapshot it owns."""
    C = blk.n_embd
    lay = cat9_layout(C)
    dev = blk.fc1.weight.device

    def gemm(ws, rows=None):     # the rows of `ws` stacked, zero rows added up to `rows`
        src = torch.cat([w.detach() for w in ws], 0).contiguous()
        out = torch.zeros((rows or src.shape[0], src.shape[1]), dtype=dtype, device=dev)
        if dtype == F32:
            out[:src.shape[0]].copy_(src)
        else:
            ops.cast_bf16(src, out=out[:src.shape[0]])
        return out

    f32 = lambda p: p.detach().clone().contiguous()  # noqa: E731
    cat_b = torch.zeros(lay.n, dtype=F32, device=dev)
    cat_b[lay.rows["fc2"][0]:lay.rows["fc2"][1]].copy_(blk.fc2.bias.detach())
    dirs = []
    for mod in (blk.forward_mamba, blk.backward_mamba):
        n_x = mod.dt_rank + 32 if dtype == F32 else x_proj_rows16(mod.dt_rank)
        dirs.append(SimpleNamespace(conv_w=f32(mod.conv1d.weight), conv_b=f32(mod.conv1d.bias), x_w=gemm([mod.x_proj.weight], n_x),
                                    dt_w=f32(mod.dt_proj.weight), dt_b=f32(mod.dt_proj.bias), A_log=f32(mod.A_log),
                                    D=f32(mod.D), out_w=gemm([mod.out_proj.weight])))
    return SimpleNamespace(ln_w=f32(blk.ln1.weight), ln_b=f32(blk.ln1.bias), fc1_w=gemm([blk.fc1.weight]), fc1_b=f32(blk.fc1.bias),
                           cat_w=gemm([blk.forward_mamba.in_proj.weight, blk.backward_mamba.in_proj.weight, blk.fc2.weight]),
                           cat_b=cat_b, dirs=tuple(dirs))
