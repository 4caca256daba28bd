"""Thin tensor-level wrappers over the C ABI (include/ds6g.h).

PyTorch is used for device memory and the current HIP stream only; every arithmetic operation is
a kernel in libds6g.so.  Tensors must be fp32, contiguous, on a HIP device; shapes are checked here
on the host because an out-of-bounds kernel can take the whole GPU node down.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import lib

F32 = torch.float32


def _p(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    """raw hipStream_t of the calling thread's current stream.  torch.cuda.current_stream() builds a Stream object per call
    (~8 us; the step makes ~2000 launches): the two C-level calls below return the same handle in well under a microsecond"""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


_STREAM_OBJS = {}


def current_stream_obj():
    """torch.cuda.current_stream() without its ~8 us of device-index plumbing: Stream objects are cached by raw handle (the
    walk switches streams ~400 times per step)"""
    raw = _stream()
    s = _STREAM_OBJS.get(raw)
    if s is None:
        s = torch.cuda.current_stream()
        _STREAM_OBJS[s.cuda_stream] = s
    return s


class on_stream:
    """`with torch.cuda.stream(s)` for the hot path: one C-level set-stream call each way, no Stream objects built"""
    __slots__ = ("s", "prev")

    def __init__(self, s):
        self.s = s
        _STREAM_OBJS.setdefault(s.cuda_stream, s)

    def __enter__(self):
        self.prev = current_stream_obj()
        s = self.s
        torch._C._cuda_setStream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type)
        return s

    def __exit__(self, *exc):
        p = self.prev
        torch._C._cuda_setStream(stream_id=p.stream_id, device_index=p.device_index, device_type=p.device_type)
        return False


def _chk(t, *shape):
    assert t.dtype == F32 and t.is_cuda and t.is_contiguous(), (t.dtype, t.device, t.stride())
    if shape:
        assert tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)


class Workspace:
    """One caller-owned scratch buffer shared by all kernels of a stream (split-K slabs, BN / LN /
    column-sum partials).  Stream order makes the reuse safe."""

    def __init__(self, device, nbytes=1 << 30):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.nbytes = nbytes

    @property
    def ptr(self):
        return self.buf.data_ptr()


# ------------------------------------------------------------------------------------------------
def conv_out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def conv2d_fwd(x, w_ohwi_ptr, K, R, S, stride, pad, out=None):
    N, H, W, C = x.shape
    _chk(x)
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    y = out if out is not None else torch.empty((N, Ho, Wo, K), dtype=F32, device=x.device)
    _chk(y, N, Ho, Wo, K)
    lib().conv2d_fwd(_p(x), w_ohwi_ptr, _p(y), N, H, W, C, K, R, S, stride, pad, _stream())
    return y


def conv2d_bias_act_fwd(x, w_ohwi_ptr, bias_ptr, K, R, S, stride, pad, relu=0, residual=None):
    """inference conv with folded BN: act(conv(x, w) + bias [+ residual]); relu 0 none / 1 before / 2 after the add"""
    N, H, W, C = x.shape
    _chk(x)
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    y = torch.empty((N, Ho, Wo, K), dtype=F32, device=x.device)
    if residual is not None:
        _chk(residual, N, Ho, Wo, K)
    lib().conv2d_bias_act_fwd(_p(x), w_ohwi_ptr, bias_ptr, _p(residual), _p(y), N, H, W, C, K, R, S, stride, pad,
                              int(relu), _stream())
    return y


def bn_fold(w_ohwi_ptr, bn, K, taps, cin, cpad=None, dtype=F32, out=None):
    """-> (w_folded [K, taps, cpad], bias [K]) of an eval-mode BatchNorm2d folded into the preceding conv.  dtype bf16 / f16:
    the folded filter is stored in that type (scaled in fp32, rounded once; the bias stays fp32).  out = (w_folded, bias):
    written in place (the frozen inference engine refreshes its snapshot into the same buffers)"""
    cpad = cin if cpad is None else cpad
    dev = bn.weight.device
    if out is not None:
        w_out, b_out = out
        dtype = w_out.dtype
        assert w_out.is_cuda and w_out.is_contiguous() and w_out.numel() == K * taps * cpad, (tuple(w_out.shape), K, taps, cpad)
        _chk(b_out, K)
    else:
        w_out = torch.empty((K, taps, cpad), dtype=dtype, device=dev)
        b_out = torch.empty((K,), dtype=F32, device=dev)
    assert dtype in (F32, BF16, F16), dtype
    _launch(lib().bn_fold, lib().bn_fold_h16, dtype, w_ohwi_ptr, bn.weight.data_ptr(), bn.bias.data_ptr(),
            bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.eps), w_out.data_ptr(), b_out.data_ptr(), K, taps,
            cin, cpad)
    return w_out, b_out


def winograd_ok(x_shape, K):
    """3x3 / stride 1 / pad 1 conv of an NHWC tensor of this shape to K channels can run as Winograd F(2x2, 3x3)"""
    N, H, W, C = x_shape
    # exact-fp32 products only: the default mode, f16 (whose fp32-storage kernels are those of "f32"), and f32x6 (fp32-grade: its direct kernels use the six-product split, its
    # 3x3 / stride-1 convs stay on the fp32 Winograd kernel, which is faster than the split direct form)
    return bool(lib().winograd_supported(N, H, W, C, K)) and lib().get_compute_mode() in (0, 3, 5)


def winograd_weights(w_ohwi_ptr, K, C, device, dgrad=False, both=False, out=None):
    """U = G g G^T of an OHWI [K, 3, 3, C] filter: [16, K, C] (forward) or, dgrad=True, [16, C, K] of the
    channel-swapped, 180-degree-rotated filter; both=True: (forward, dgrad) from one launch; out: written in place"""
    n = lib().winograd_weight_floats(K, C)
    if out is not None:
        _chk(out, 2 * n if both else n)
    u = out if out is not None else torch.empty(2 * n if both else n, dtype=F32, device=device)
    lib().winograd_weights(w_ohwi_ptr, _p(u), K, C, 2 if both else int(dgrad), _stream())
    return (u[:n], u[n:]) if both else u


def conv3x3_winograd(x, u, K, out=None, accumulate=False):
    """y (+)= conv3x3(x) (stride 1, pad 1) from the transformed filter u [16, K, C]"""
    N, H, W, C = x.shape
    _chk(x)
    y = out if out is not None else torch.empty((N, H, W, K), dtype=F32, device=x.device)
    _chk(y, N, H, W, K)
    lib().conv3x3_winograd_fwd(_p(x), _p(u), _p(y), N, H, W, C, K, int(accumulate), _stream())
    return y


def conv3x3_winograd_bias_act(x, u, bias_ptr, K, relu=0, residual=None):
    """inference 3x3 conv with folded BN in the Winograd domain: act(conv(x) + bias [+ residual])"""
    N, H, W, C = x.shape
    _chk(x)
    y = torch.empty((N, H, W, K), dtype=F32, device=x.device)
    if residual is not None:
        _chk(residual, N, H, W, K)
    lib().conv3x3_winograd_bias_act_fwd(_p(x), _p(u), bias_ptr, _p(residual), _p(y), N, H, W, C, K, int(relu), _stream())
    return y


def winograd_wgrad_ok(x_shape, K):
    N, H, W, C = x_shape
    return bool(lib().winograd_wgrad_supported(N, H, W, C, K)) and lib().get_compute_mode() in (0, 3, 5)


def conv3x3_winograd_wgrad(x, dy, dw_ohwi_ptr, ws: Workspace, accumulate=False):
    """dw [K, 3, 3, C] (+)= weight gradient of the 3x3 / stride 1 / pad 1 conv, computed in the Winograd domain"""
    N, H, W, C = x.shape
    K = dy.shape[3]
    _chk(x)
    _chk(dy, N, H, W, K)
    lib().conv3x3_winograd_wgrad(_p(x), _p(dy), dw_ohwi_ptr, N, H, W, C, K, int(accumulate), ws.ptr, ws.nbytes, _stream())


def conv2d_dgrad(dy, w_ohwi_ptr, x_shape, R, S, stride, pad, out=None, accumulate=False):
    N, H, W, C = x_shape
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    K = dy.shape[3]
    _chk(dy, N, Ho, Wo, K)
    dx = out if out is not None else torch.empty(x_shape, dtype=F32, device=dy.device)
    _chk(dx, *x_shape)
    lib().conv2d_dgrad(_p(dy), w_ohwi_ptr, _p(dx), N, H, W, C, K, R, S, stride, pad, int(accumulate), _stream())
    return dx


def conv2d_wgrad(x, dy, dw_ptr, R, S, stride, pad, ws: Workspace, accumulate=False):
    N, H, W, C = x.shape
    _chk(x)
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    K = dy.shape[3]
    _chk(dy, N, Ho, Wo, K)
    lib().conv2d_wgrad(_p(x), _p(dy), dw_ptr, N, H, W, C, K, R, S, stride, pad, int(accumulate), ws.ptr, ws.nbytes,
                       _stream())


def linear_fwd(x, w_ptr, b_ptr, N, relu=False, residual=None, drop_p=0.0, seed=0, seed_off=0, out=None):
    M, K = x.shape
    _chk(x)
    y = out if out is not None else torch.empty((M, N), dtype=F32, device=x.device)
    _chk(y, M, N)
    if residual is not None:
        _chk(residual, M, N)
    lib().linear_fwd(_p(x), w_ptr, b_ptr, _p(y), M, N, K, int(relu), _p(residual), float(drop_p), seed, seed_off,
                     _stream())
    return y


def linear_dgrad(dy, w_ptr, K, relu_mask_src=None, out=None, accumulate=False):
    M, N = dy.shape
    _chk(dy)
    dx = out if out is not None else torch.empty((M, K), dtype=F32, device=dy.device)
    _chk(dx, M, K)
    if relu_mask_src is not None:
        _chk(relu_mask_src, M, K)
    lib().linear_dgrad(_p(dy), w_ptr, _p(dx), M, N, K, _p(relu_mask_src), int(accumulate), _stream())
    return dx


def linear_wgrad(x, dy, dw_ptr, ws: Workspace, accumulate=False, dbias_ptr=0):
    """dw (+)= dy^T x and, when dbias_ptr is given, dbias (+)= column sums of dy from the same kernel."""
    M, K = x.shape
    M2, N = dy.shape
    assert M == M2
    _chk(x)
    _chk(dy)
    lib().linear_wgrad(_p(x), _p(dy), dw_ptr, dbias_ptr, M, N, K, int(accumulate), ws.ptr, ws.nbytes, _stream())


def colsum(x, out_ptr, ws: Workspace, accumulate=False):
    M, C = x.shape
    _chk(x)
    lib().colsum(_p(x), M, C, out_ptr, int(accumulate), ws.ptr, ws.nbytes, _stream())


# ------------------------------------------------------------------------------------------------
def bn_stats(x2d_rows, C, x, mean, invstd, rm_ptr, rv_ptr, ws: Workspace, eps=1e-5, momentum=0.1):
    lib().bn_stats(_p(x), x2d_rows, C, eps, momentum, _p(mean), _p(invstd), rm_ptr, rv_ptr, ws.ptr, ws.nbytes,
                   _stream())


def bn_eval_prepare(rm_ptr, rv_ptr, C, mean, invstd, eps=1e-5):
    lib().bn_eval_prepare(rm_ptr, rv_ptr, C, eps, _p(mean), _p(invstd), _stream())


def bn_apply(x, mean, invstd, gamma_ptr, beta_ptr, relu, residual=None, out=None):
    _chk(x)
    C = x.shape[-1]
    M = x.numel() // C
    y = out if out is not None else torch.empty_like(x)
    if residual is not None:
        _chk(residual, *x.shape)
    lib().bn_apply(_p(x), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(residual), _p(y), M, C, int(relu), _stream())
    return y


def bn_bwd(dy, y_mask, x, mean, invstd, gamma_ptr, dgamma_ptr, dbeta_ptr, ws: Workspace, want_dres=False,
           accumulate=False, dx_out=None, relu_beta_ptr=0):
    """y_mask: activation tensor whose sign gives the ReLU mask, or None; relu_beta_ptr (with y_mask None): BN -> ReLU
    without a residual in between - the mask is recomputed from x inside the kernels."""
    _chk(dy, *x.shape)
    _chk(x)
    C = x.shape[-1]
    M = x.numel() // C
    dx = dx_out if dx_out is not None else torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    lib().bn_bwd(_p(dy), _p(y_mask), _p(x), _p(mean), _p(invstd), gamma_ptr, relu_beta_ptr, _p(dx), dgamma_ptr, dbeta_ptr,
                 _p(dres), M, C, int(accumulate), ws.ptr, ws.nbytes, _stream())
    return dx, dres


def bn_relu_maxpool(x, mean, invstd, gamma_ptr, beta_ptr):
    """maxpool3x3/2(relu(BN(x))) in one pass (the stem) -> (pooled [N, Ho, Wo, C], argmax index uint8)"""
    N, H, W, C = x.shape
    _chk(x)
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((N, Ho, Wo, C), dtype=F32, device=x.device)
    idx = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    lib().bn_relu_maxpool3x3s2_fwd(_p(x), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(y), _p(idx), N, H, W, C, _stream())
    return y, idx


def bn_bwd_maxpool(dpool, idx, x, mean, invstd, gamma_ptr, beta_ptr, dgamma_ptr, dbeta_ptr, ws: Workspace, accumulate=False):
    """backward of bn_relu_maxpool: dx of the BN input from the gradient of the pooled tensor (ReLU mask recomputed from
    x, pool gradient gathered from (dpool, idx) inside the BN kernels)"""
    N, H, W, C = x.shape
    _chk(x)
    _chk(dpool, N, (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, C)
    dx = torch.empty_like(x)
    lib().bn_bwd_maxpool(_p(dpool), _p(idx), _p(x), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(dx), dgamma_ptr, dbeta_ptr,
                         N, H, W, C, int(accumulate), ws.ptr, ws.nbytes, _stream())
    return dx


def layernorm_fwd(x, gamma_ptr, beta_ptr, eps=1e-5):
    M, C = x.shape
    _chk(x)
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=F32, device=x.device)
    rstd = torch.empty(M, dtype=F32, device=x.device)
    lib().layernorm_fwd(_p(x), gamma_ptr, beta_ptr, _p(y), _p(mean), _p(rstd), M, C, eps, _stream())
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma_ptr, dgamma_ptr, dbeta_ptr, ws: Workspace, add=None, accumulate=False,
                  out=None, drop=None, partial=None):
    """-> dx, or (dx, dropout(dx)) when drop = (p, seed, seed_off) with p > 0 (fused second output).  partial = (ptr, nbytes)
    of the caller's own buffer: the deferred form - dgamma / dbeta are left as row-block partials there for
    layernorm_finalize_batched (dgamma_ptr, dbeta_ptr, accumulate and ws are not used)"""
    M, C = x.shape
    _chk(dy, M, C)
    _chk(x)
    dx = out if out is not None else torch.empty_like(x)
    if add is not None:
        _chk(add, M, C)
    dxd = torch.empty_like(x) if (drop is not None and drop[0] > 0) else None
    p, seed, off = drop if dxd is not None else (0.0, 0, 0)
    if partial is not None:
        lib().layernorm_bwd_partial(_p(dy), _p(x), _p(mean), _p(rstd), gamma_ptr, _p(add), _p(dx), M, C, _p(dxd), float(p),
                                    seed, off, partial[0], partial[1], _stream())
        return dx if drop is None else (dx, dxd if dxd is not None else dx)
    lib().layernorm_bwd(_p(dy), _p(x), _p(mean), _p(rstd), gamma_ptr, _p(add), _p(dx), dgamma_ptr, dbeta_ptr, M, C,
                        int(accumulate), _p(dxd), float(p), seed, off, ws.ptr, ws.nbytes, _stream())
    return dx if drop is None else (dx, dxd if dxd is not None else dx)


LN_BWD_ROWS = 16          # rows per row-block partial of the LayerNorm backward (csrc/norm.hip)
LN_FINALIZE_MAX = 24      # DS6G_LN_FINALIZE_MAX of include/ds6g.h


class _LnFinalizeDesc(ctypes.Structure):   # ds6g_ln_finalize_desc
    _fields_ = [("partial", ctypes.c_void_p), ("nblk", ctypes.c_int), ("C", ctypes.c_int), ("dgamma", ctypes.c_void_p),
                ("dbeta", ctypes.c_void_p), ("accumulate", ctypes.c_int)]


class _MapDesc(ctypes.Structure):          # ds6g_map_desc
    _fields_ = [("inp", ctypes.c_void_p), ("out", ctypes.c_void_p), ("frames_per_sample", ctypes.c_int),
                ("mod_off", ctypes.c_int)]


def layernorm_partial_bytes(M, C):
    return -(-M // LN_BWD_ROWS) * 2 * C * 4


def layernorm_finalize_batched(items):
    """items: (partial_ptr, M, C, dgamma_ptr, dbeta_ptr, accumulate) of 1 .. 24 deferred LayerNorm backwards (partial=...):
    dgamma / dbeta (+)= in one launch, bit-identical to the undeferred layernorm_bwd"""
    n = len(items)
    descs = (_LnFinalizeDesc * max(n, 1))()
    for d, (pp, M, C, gw, gb, acc) in zip(descs, items):
        d.partial, d.nblk, d.C, d.dgamma, d.dbeta, d.accumulate = pp, -(-M // LN_BWD_ROWS), C, gw, gb, int(bool(acc))
    lib().layernorm_finalize_batched(ctypes.addressof(descs), n, _stream())


# ------------------------------------------------------------------------------------------------
def _rows(t, M, C):
    """2-D fp32 operand whose rows may be a column block of a wider matrix -> row stride in floats"""
    assert t.dtype == F32 and t.is_cuda and tuple(t.shape) == (M, C) and t.stride(1) == 1 and t.stride(0) % 4 == 0, \
        (t.dtype, tuple(t.shape), t.stride())
    return t.stride(0)


def attention_fwd(q, k, v, B, T, nh, ws: Workspace, drop_p=0.0, seed=0, seed_off=0):
    """q, k, v: [B*T, C] each, contiguous or column blocks of one fused projection output (same row stride)."""
    M, C = q.shape
    assert M == B * T
    ldq = _rows(q, M, C)
    assert _rows(k, M, C) == ldq and _rows(v, M, C) == ldq
    o = torch.empty((M, C), dtype=F32, device=q.device)
    lse = torch.empty((B, nh, T), dtype=F32, device=q.device)
    lib().attention_fwd(_p(q), _p(k), _p(v), _p(o), _p(lse), B, T, nh, C // nh, ldq, C, float(drop_p), seed, seed_off,
                        ws.ptr, ws.nbytes, _stream())
    return o, lse


def attention_bwd(q, k, v, o, d_o, lse, B, T, nh, ws: Workspace, drop_p=0.0, seed=0, seed_off=0, out=None):
    """-> (dq, dk, dv); `out` = three [B*T, C] views with one common row stride (column blocks of a fused matrix)."""
    M, C = q.shape
    ldq = _rows(q, M, C)
    assert _rows(k, M, C) == ldq and _rows(v, M, C) == ldq
    for t in (o, d_o):
        _chk(t, M, C)
    _chk(lse, B, nh, T)
    delta = torch.empty_like(lse)
    if out is None:
        out = tuple(torch.empty((M, C), dtype=F32, device=q.device) for _ in range(3))
    dq, dk, dv = out
    ldd = _rows(dq, M, C)
    assert _rows(dk, M, C) == ldd and _rows(dv, M, C) == ldd
    lib().attention_bwd(_p(q), _p(k), _p(v), _p(o), _p(d_o), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), B, T, nh,
                        C // nh, ldq, C, ldd, float(drop_p), seed, seed_off, ws.ptr, ws.nbytes, _stream())
    return dq, dk, dv


# ------------------------------------------------------------------------------------------------
def dropout(src, drop_p, seed, seed_off, out=None):
    _chk(src)
    dst = out if out is not None else torch.empty_like(src)
    lib().dropout(_p(src), _p(dst), src.numel(), float(drop_p), seed, seed_off, _stream())
    return dst


def axpby(a, b, alpha=1.0, beta=1.0, out=None):
    _chk(a)
    o = out if out is not None else torch.empty_like(a)
    lib().axpby(_p(a), _p(b), _p(o), a.numel(), float(alpha), float(beta), _stream())
    return o


_MODES = {"f32": 0, "bf16": 1, "f32x3": 2, "f32x6": 3, "f16": 5}


def set_compute_mode(mode: str):
    """Process-wide matrix-core mode of the GEMM-shaped kernels (ds6g_set_compute_mode):
    "f32"   - exact fp32 MFMA, the parity path (default);
    "bf16"  - operands rounded to bf16 on the way into the MFMA, fp32 accumulate and storage (throughput mode; the
              reference has no mixed precision, tolerances for it are declared in tests/test_bf16_gpu.py);
    "f32x3" - split bf16: a*b = hi*hi + hi*lo + lo*hi on the bf16 matrix cores, fp32 accumulate and storage; relative
              product error <= ~2^-16 (tests/test_bf16_gpu.py holds it to the 1e-3 bar of the exact path);
    "f16"   - the bf16 configuration's 16-bit STORAGE with IEEE half instead of bf16 (3 more significand bits, same matrix-core
              cycles); everything that is not 16-bit storage runs exactly as in "f32" (eval, the small linears, the fp32
              stems).  A training-storage mode: train it with train.DynamicLossScaler."""
    if mode not in _MODES:
        raise ValueError(f"compute mode must be one of {sorted(_MODES)}, got {mode!r}")
    lib().set_compute_mode(_MODES[mode])


def get_compute_mode() -> str:
    return {v: k for k, v in _MODES.items()}[lib().get_compute_mode()]


# ------------------------------------------------------------------------------------------------
# 16-bit stored operands (csrc/bgemm.hip): activations / weight shadow bf16 or f16, accumulation fp32.  Each kernel has one
# entry point (ds6g_h16_*, *_h16*) whose first argument names the storage type; the bf16_* wrappers below pass the code of
# their 16-bit operand's dtype, and outputs take that dtype.
BF16 = torch.bfloat16
F16 = torch.float16
_ST16 = {BF16: 1, F16: 2}   # DS6G_ST_BF16 / DS6G_ST_F16 of include/ds6g.h


def _launch(f32_entry, h16_entry, dtype, *args):
    """a kernel that exists for all three storages, on the current stream: its fp32 entry point, or the 16-bit one with the
    storage code of `dtype` in front"""
    if dtype == F32:
        f32_entry(*args, _stream())
    else:
        h16_entry(_ST16[dtype], *args, _stream())


def _chk16(t, *shape, dtype=None):
    """a contiguous bf16 / f16 device tensor (of `dtype` when given: every 16-bit operand of one call shares one dtype)"""
    assert t.dtype in (BF16, F16) and t.is_cuda and t.is_contiguous(), (t.dtype, t.device, t.stride())
    assert dtype is None or t.dtype == dtype, (t.dtype, dtype)
    if shape:
        assert tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)


def bf16_linear_fwd(x, w16_ptr, b_ptr, N, relu=False, residual=None, drop_p=0.0, seed=0, seed_off=0, out16=True):
    """y = residual + dropout(act(x w^T + b)): x [M, K] bf16, w [N, K] bf16; y bf16, or fp32 (always with a residual)"""
    M, K = x.shape
    _chk16(x)
    out16 = bool(out16) and residual is None
    y = torch.empty((M, N), dtype=x.dtype if out16 else F32, device=x.device)
    if residual is not None:
        _chk(residual, M, N)
    lib().h16_linear_fwd(_ST16[x.dtype], _p(x), w16_ptr, b_ptr, _p(y), int(out16), M, N, K, int(relu), _p(residual), float(drop_p), seed,
                         seed_off, _stream())
    return y


def bf16_linear_dgrad(dy, w16_ptr, K, relu_mask_src=None, out16=True, out=None, accumulate=False):
    """dx (+)= (dy w) * (mask > 0): dy [M, N] bf16, w [N, K] bf16; mask bf16 or fp32 [M, K]"""
    M, N = dy.shape
    _chk16(dy)
    dx = out if out is not None else torch.empty((M, K), dtype=dy.dtype if out16 else F32, device=dy.device)
    assert dx.dtype == (dy.dtype if out16 else F32) and tuple(dx.shape) == (M, K) and dx.is_contiguous()
    mask16 = 0
    if relu_mask_src is not None:
        assert tuple(relu_mask_src.shape) == (M, K) and relu_mask_src.is_contiguous() and out16
        mask16 = int(relu_mask_src.dtype != F32)
        assert relu_mask_src.dtype in (F32, dy.dtype)
    lib().h16_linear_dgrad(_ST16[dy.dtype], _p(dy), w16_ptr, _p(dx), int(out16), M, N, K, _p(relu_mask_src), mask16, int(accumulate), _stream())
    return dx


def bf16_linear_wgrad(x, dy, dw_ptr, ws: Workspace, accumulate=False, dbias_ptr=0):
    """dw (fp32) (+)= dy^T x, dbias (+)= column sums of dy: x [M, K], dy [M, N] bf16"""
    M, K = x.shape
    M2, N = dy.shape
    assert M == M2
    _chk16(x)
    _chk16(dy, dtype=x.dtype)
    lib().h16_linear_wgrad(_ST16[x.dtype], _p(x), _p(dy), dw_ptr, dbias_ptr, M, N, K, int(accumulate), ws.ptr, ws.nbytes, _stream())


def bf16_conv2d_fwd(x, w16_ptr, K, R, S, stride, pad, out16=True):
    N, H, W, C = x.shape
    _chk16(x)
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    y = torch.empty((N, Ho, Wo, K), dtype=x.dtype if out16 else F32, device=x.device)
    lib().h16_conv2d_fwd(_ST16[x.dtype], _p(x), w16_ptr, _p(y), int(out16), N, H, W, C, K, R, S, stride, pad, _stream())
    return y


def bf16_conv2d_bias_act_fwd(x, w16_ptr, bias_ptr, K, R, S, stride, pad, relu=0, residual=None):
    """inference conv on 16-bit storage with folded BN: act(conv(x, w) + bias [+ residual]) -> 16-bit; relu 0 none / 1 before /
    2 after the add; bias fp32, residual of x's dtype, added in fp32 before the one rounding"""
    N, H, W, C = x.shape
    _chk16(x)
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    assert Ho > 0 and Wo > 0 and C % 64 == 0 and K % 8 == 0, (x.shape, K, R, S, stride, pad)
    y = torch.empty((N, Ho, Wo, K), dtype=x.dtype, device=x.device)
    if residual is not None:
        _chk16(residual, N, Ho, Wo, K, dtype=x.dtype)
    lib().h16_conv2d_bias_act_fwd(_ST16[x.dtype], _p(x), w16_ptr, bias_ptr, _p(residual), _p(y), N, H, W, C, K, R, S, stride, pad,
                                  int(relu), _stream())
    return y


def bf16_conv2d_fwd_bnstats(x, w16_ptr, K, R, S, stride, pad, mean, invstd, rm_ptr, rv_ptr, ws: Workspace, eps=1e-5,
                            momentum=0.1):
    """y = conv(x, w) (bf16) and the train-mode BatchNorm statistics of y from the conv's own epilogue (no pass over y)"""
    N, H, W, C = x.shape
    _chk16(x)
    _chk(mean, K)
    _chk(invstd, K)
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    y = torch.empty((N, Ho, Wo, K), dtype=x.dtype, device=x.device)
    lib().h16_conv2d_fwd_bnstats(_ST16[x.dtype], _p(x), w16_ptr, _p(y), N, H, W, C, K, R, S, stride, pad, eps, momentum, _p(mean),
                                 _p(invstd), rm_ptr, rv_ptr, ws.ptr, ws.nbytes, _stream())
    return y


def bf16_conv2d_dgrad(dy, w16_ptr, x_shape, R, S, stride, pad, out16=True, out=None, accumulate=False):
    N, H, W, C = x_shape
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    K = dy.shape[3]
    _chk16(dy, N, Ho, Wo, K)
    dx = out if out is not None else torch.empty(x_shape, dtype=dy.dtype if out16 else F32, device=dy.device)
    assert dx.dtype == (dy.dtype if out16 else F32) and tuple(dx.shape) == tuple(x_shape) and dx.is_contiguous()
    lib().h16_conv2d_dgrad(_ST16[dy.dtype], _p(dy), w16_ptr, _p(dx), int(out16), N, H, W, C, K, R, S, stride, pad, int(accumulate), _stream())
    return dx


def bf16_conv2d_wgrad(x, dy, dw_ptr, R, S, stride, pad, ws: Workspace, accumulate=False):
    N, H, W, C = x.shape
    _chk16(x)
    Ho, Wo = conv_out_hw(H, W, R, S, stride, pad)
    K = dy.shape[3]
    _chk16(dy, N, Ho, Wo, K, dtype=x.dtype)
    lib().h16_conv2d_wgrad(_ST16[x.dtype], _p(x), _p(dy), dw_ptr, N, H, W, C, K, R, S, stride, pad, int(accumulate), ws.ptr, ws.nbytes, _stream())


def cast_bf16(src, out=None, dtype=BF16):
    """bf16 (or f16: dtype / out.dtype) copy (RNE) of a contiguous fp32 tensor whose numel is a multiple of 4"""
    _chk(src)
    dst = out if out is not None else torch.empty(src.shape, dtype=dtype, device=src.device)
    assert dst.dtype in (BF16, F16) and dst.numel() == src.numel() and dst.is_contiguous()
    lib().cast_f32_h16(_ST16[dst.dtype], _p(src), _p(dst), src.numel(), _stream())
    return dst


def layernorm_fwd_bf16(x, gamma_ptr, beta_ptr, eps=1e-5, dtype=BF16):
    """LayerNorm of fp32 rows, output written as bf16 / f16 (dtype; a GEMM operand) -> (y16, mean, rstd)"""
    M, C = x.shape
    _chk(x)
    y = torch.empty((M, C), dtype=dtype, device=x.device)
    mean = torch.empty(M, dtype=F32, device=x.device)
    rstd = torch.empty(M, dtype=F32, device=x.device)
    lib().layernorm_fwd_h16out(_ST16[dtype], _p(x), gamma_ptr, beta_ptr, _p(y), _p(mean), _p(rstd), M, C, eps, _stream())
    return y, mean, rstd


def layernorm_bwd_bf16(dy, x, mean, rstd, gamma_ptr, dgamma_ptr, dbeta_ptr, ws: Workspace, add=None, accumulate=False,
                       drop=None, want_drop=True, dtype=BF16, partial=None):
    """dy 16-bit (dtype: bf16 / f16) or fp32 -> (dx fp32, dropout(dx) as dtype); drop = (p, seed, seed_off) or None (= plain
    16-bit copy of dx); want_drop False: no second output (-> (dx, None))"""
    M, C = x.shape
    assert tuple(dy.shape) == (M, C) and dy.is_contiguous() and dy.dtype in (dtype, F32)
    _chk(x)
    if add is not None:
        _chk(add, M, C)
    dx = torch.empty_like(x)
    dxd = torch.empty((M, C), dtype=dtype, device=x.device) if want_drop else None
    p, seed, off = drop if drop is not None else (0.0, 0, 0)
    if partial is not None:   # deferred dgamma / dbeta: see layernorm_bwd
        lib().layernorm_bwd_h16_partial(_ST16[dtype], _p(dy), int(dy.dtype != F32), _p(x), _p(mean), _p(rstd), gamma_ptr,
                                        _p(add), _p(dx), M, C, _p(dxd), float(p), seed, off, partial[0], partial[1],
                                        _stream())
        return dx, dxd
    lib().layernorm_bwd_h16(_ST16[dtype], _p(dy), int(dy.dtype != F32), _p(x), _p(mean), _p(rstd), gamma_ptr, _p(add), _p(dx), dgamma_ptr,
                            dbeta_ptr, M, C, int(accumulate), _p(dxd), float(p), seed, off, ws.ptr, ws.nbytes, _stream())
    return dx, dxd


def attention_fwd_bf16out(q, k, v, B, T, nh, ws: Workspace, drop_p=0.0, seed=0, seed_off=0):
    """as attention_fwd, the output written as bf16 (operand of the projection GEMM)"""
    M, C = q.shape
    assert M == B * T
    ldq = _rows(q, M, C)
    assert _rows(k, M, C) == ldq and _rows(v, M, C) == ldq
    o = torch.empty((M, C), dtype=BF16, device=q.device)
    lse = torch.empty((B, nh, T), dtype=F32, device=q.device)
    lib().attention_fwd_bf16out(_p(q), _p(k), _p(v), _p(o), _p(lse), B, T, nh, C // nh, ldq, C, float(drop_p), seed, seed_off,
                                ws.ptr, ws.nbytes, _stream())
    return o, lse


def attention_bwd_bf16(q, k, v, o16, d_o, lse, B, T, nh, ws: Workspace, drop_p=0.0, seed=0, seed_off=0, out=None):
    """o16: the bf16 forward output; d_o fp32; -> dq, dk, dv as bf16 (`out`: three [B*T, C] bf16 views of one row stride)"""
    M, C = q.shape
    ldq = _rows(q, M, C)
    assert _rows(k, M, C) == ldq and _rows(v, M, C) == ldq
    _chk16(o16, M, C)
    _chk(d_o, M, C)
    _chk(lse, B, nh, T)
    assert ws.nbytes >= int(lib().attention_workspace_bytes(B, T, nh, C // nh, C)), "attention_bwd_bf16 needs the hand-over workspace"
    delta = torch.empty_like(lse)
    if out is None:
        out = tuple(torch.empty((M, C), dtype=BF16, device=q.device) for _ in range(3))
    dq, dk, dv = out
    for t in out:
        assert t.dtype == BF16 and tuple(t.shape) == (M, C) and t.stride(1) == 1 and t.stride(0) % 4 == 0
    ldd = dq.stride(0)
    assert dk.stride(0) == ldd and dv.stride(0) == ldd
    lib().attention_bwd_bf16(_p(q), _p(k), _p(v), _p(o16), _p(d_o), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), B, T, nh,
                             C // nh, ldq, C, ldd, float(drop_p), seed, seed_off, ws.ptr, ws.nbytes, _stream())
    return dq, dk, dv


# ---- bf16-storage path: BatchNorm / pooling / resampling on bf16 feature maps (statistics and arithmetic fp32) ----
def bf16_bn_stats(x2d_rows, C, x, mean, invstd, rm_ptr, rv_ptr, ws: Workspace, eps=1e-5, momentum=0.1):
    _chk16(x)
    lib().h16_bn_stats(_ST16[x.dtype], _p(x), x2d_rows, C, eps, momentum, _p(mean), _p(invstd), rm_ptr, rv_ptr, ws.ptr, ws.nbytes, _stream())


def bf16_bn_apply(x, mean, invstd, gamma_ptr, beta_ptr, relu, residual=None):
    _chk16(x)
    C = x.shape[-1]
    y = torch.empty_like(x)
    if residual is not None:
        _chk16(residual, *x.shape, dtype=x.dtype)
    lib().h16_bn_apply(_ST16[x.dtype], _p(x), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(residual), _p(y), x.numel() // C, C, int(relu),
                       _stream())
    return y


def bf16_bn_bwd(dy, y_mask, x, mean, invstd, gamma_ptr, dgamma_ptr, dbeta_ptr, ws: Workspace, want_dres=False,
                accumulate=False, relu_beta_ptr=0):
    _chk16(dy, *x.shape, dtype=x.dtype)
    _chk16(x)
    if y_mask is not None:
        _chk16(y_mask, *x.shape, dtype=x.dtype)
    C = x.shape[-1]
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    lib().h16_bn_bwd(_ST16[x.dtype], _p(dy), _p(y_mask), _p(x), _p(mean), _p(invstd), gamma_ptr, relu_beta_ptr, _p(dx), dgamma_ptr, dbeta_ptr,
                     _p(dres), x.numel() // C, C, int(accumulate), ws.ptr, ws.nbytes, _stream())
    return dx, dres


def bn_relu_maxpool_bf16out(x, mean, invstd, gamma_ptr, beta_ptr, dtype=BF16):
    """the stem's BN -> ReLU -> MaxPool of the fp32 conv output, pooled tensor written as bf16 / f16 (dtype)"""
    N, H, W, C = x.shape
    _chk(x)
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((N, Ho, Wo, C), dtype=dtype, device=x.device)
    idx = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    lib().bn_relu_maxpool3x3s2_fwd_h16out(_ST16[dtype], _p(x), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(y), _p(idx), N, H, W, C, _stream())
    return y, idx


def bn_bwd_maxpool_bf16in(dpool, idx, x, mean, invstd, gamma_ptr, beta_ptr, dgamma_ptr, dbeta_ptr, ws: Workspace, accumulate=False):
    N, H, W, C = x.shape
    _chk(x)
    _chk16(dpool, N, (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, C)
    dx = torch.empty_like(x)
    lib().bn_bwd_maxpool_h16in(_ST16[dpool.dtype], _p(dpool), _p(idx), _p(x), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(dx), dgamma_ptr,
                               dbeta_ptr, N, H, W, C, int(accumulate), ws.ptr, ws.nbytes, _stream())
    return dx


# ---- the 7x7 / 2 stem convolutions of the bf16 configuration (csrc/stem.hip) -------------------------------------------
def bf16_stem_ok(H, W):
    return H % 16 == 0 and W % 32 == 0


def bf16_stem_fwd(x16, w_ohwi_ptr, cin, ws: Workspace, stats=None, rm_ptr=0, rv_ptr=0, eps=1e-5, momentum=0.1):
    """y = conv7x7/2(x) for x [N, H, W, 4] bf16 and the fp32 master filter [64, 7, 7, cin]; stats = (mean, invstd) fp32 [64]
    tensors: also the train-mode BatchNorm statistics of y (running statistics updated in place)"""
    N, H, W, C4 = x16.shape
    _chk16(x16)
    assert C4 == 4 and bf16_stem_ok(H, W) and ws.nbytes >= int(lib().h16_stem_workspace_bytes())
    y = torch.empty((N, H // 2, W // 2, 64), dtype=x16.dtype, device=x16.device)
    mean, invstd = stats if stats is not None else (None, None)
    lib().h16_stem_fwd(_ST16[x16.dtype], _p(x16), w_ohwi_ptr, cin, _p(y), N, H, W, eps, momentum, _p(mean), _p(invstd), rm_ptr, rv_ptr, ws.ptr,
                       ws.nbytes, _stream())
    return y


def bf16_stem_pack_filter(w16, out=None):
    """BN-folded 16-bit stem filter [64, 49, 4] (bn_fold with cpad 4) -> the stem kernel's layout [64, 7, 8, 4]"""
    _chk16(w16, 64, 49, 4)
    wp = out if out is not None else torch.empty((64, 7, 8, 4), dtype=w16.dtype, device=w16.device)
    _chk16(wp, 64, 7, 8, 4, dtype=w16.dtype)
    lib().h16_stem_pack_filter(_ST16[w16.dtype], _p(w16), _p(wp), _stream())
    return wp


def bf16_stem_bias_relu_fwd(x16, w_packed, bias):
    """inference stem: relu(conv7x7/2(x, w) + bias) for x [N, H, W, 4] and the packed folded filter of x's dtype, bias fp32"""
    N, H, W, C4 = x16.shape
    _chk16(x16)
    _chk16(w_packed, 64, 7, 8, 4, dtype=x16.dtype)
    _chk(bias, 64)
    assert C4 == 4 and bf16_stem_ok(H, W), tuple(x16.shape)
    y = torch.empty((N, H // 2, W // 2, 64), dtype=x16.dtype, device=x16.device)
    lib().h16_stem_bias_relu_fwd(_ST16[x16.dtype], _p(x16), _p(w_packed), _p(bias), _p(y), N, H, W, _stream())
    return y


def bf16_maxpool3x3s2_fwd(x16):
    """3x3 / stride 2 / pad 1 max-pool of a 16-bit NHWC map, no arg-max index (inference)"""
    N, H, W, C = x16.shape
    _chk16(x16)
    assert C % 8 == 0, C
    y = torch.empty((N, (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, C), dtype=x16.dtype, device=x16.device)
    lib().h16_maxpool3x3s2_fwd(_ST16[x16.dtype], _p(x16), _p(y), N, H, W, C, _stream())
    return y


def bf16_stem_wgrad(x16, dy16, dw_ptr, cin, ws: Workspace, accumulate=False):
    N, H, W, C4 = x16.shape
    _chk16(x16)
    _chk16(dy16, N, H // 2, W // 2, 64, dtype=x16.dtype)
    assert C4 == 4 and bf16_stem_ok(H, W) and ws.nbytes >= int(lib().h16_stem_workspace_bytes())
    lib().h16_stem_wgrad(_ST16[x16.dtype], _p(x16), _p(dy16), dw_ptr, cin, N, H, W, int(accumulate), ws.ptr, ws.nbytes, _stream())


def bf16_stem_bn_relu_maxpool(x16, mean, invstd, gamma_ptr, beta_ptr):
    N, H, W, C = x16.shape
    _chk16(x16)
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((N, Ho, Wo, C), dtype=x16.dtype, device=x16.device)
    idx = torch.empty((N, Ho, Wo, C), dtype=torch.uint8, device=x16.device)
    lib().h16_stem_bn_relu_maxpool_fwd(_ST16[x16.dtype], _p(x16), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(y), _p(idx), N, H, W, C, _stream())
    return y, idx


def bf16_stem_bn_bwd_maxpool(dpool, idx, x16, mean, invstd, gamma_ptr, beta_ptr, dgamma_ptr, dbeta_ptr, ws: Workspace, accumulate=False):
    N, H, W, C = x16.shape
    _chk16(x16)
    _chk16(dpool, N, (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1, C, dtype=x16.dtype)
    dx = torch.empty_like(x16)
    lib().h16_stem_bn_bwd_maxpool(_ST16[x16.dtype], _p(dpool), _p(idx), _p(x16), _p(mean), _p(invstd), gamma_ptr, beta_ptr, _p(dx), dgamma_ptr,
                                  dbeta_ptr, N, H, W, C, int(accumulate), ws.ptr, ws.nbytes, _stream())
    return dx


def _rows16(t, M, C):
    assert t.dtype in (BF16, F16) and t.is_cuda and tuple(t.shape) == (M, C) and t.stride(1) == 1 and t.stride(0) % 8 == 0, \
        (t.dtype, tuple(t.shape), t.stride())
    return t.stride(0)


def attention_fwd_bf16(q, k, v, B, T, nh, ws: Workspace, drop_p=0.0, seed=0, seed_off=0):
    """all-bf16 attention: q, k, v [B*T, C] bf16 (column blocks of one fused projection output allowed) -> (o bf16, lse fp32)"""
    M, C = q.shape
    assert M == B * T
    ldq = _rows16(q, M, C)
    assert _rows16(k, M, C) == ldq and _rows16(v, M, C) == ldq and q.dtype == k.dtype == v.dtype
    o = torch.empty((M, C), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, nh, T), dtype=F32, device=q.device)
    lib().attention_fwd_h16(_ST16[q.dtype], _p(q), _p(k), _p(v), _p(o), _p(lse), B, T, nh, C // nh, ldq, C, float(drop_p), seed, seed_off,
                            ws.ptr, ws.nbytes, _stream())
    return o, lse


def attention_bwd_bf16io(q, k, v, o, d_o, lse, B, T, nh, ws: Workspace, drop_p=0.0, seed=0, seed_off=0, out=None):
    """all-bf16 backward: q, k, v, o, d_o bf16 -> dq, dk, dv bf16 (`out`: three [B*T, C] bf16 views of one row stride)"""
    M, C = q.shape
    ldq = _rows16(q, M, C)
    assert _rows16(k, M, C) == ldq and _rows16(v, M, C) == ldq and q.dtype == k.dtype == v.dtype
    _chk16(o, M, C, dtype=q.dtype)
    _chk16(d_o, M, C, dtype=q.dtype)
    _chk(lse, B, nh, T)
    assert ws.nbytes >= int(lib().attention_workspace_bytes(B, T, nh, C // nh, C)), "attention_bwd_bf16io needs the hand-over workspace"
    delta = torch.empty_like(lse)
    if out is None:
        out = tuple(torch.empty((M, C), dtype=q.dtype, device=q.device) for _ in range(3))
    dq, dk, dv = out
    for t in out:
        assert t.dtype == q.dtype and tuple(t.shape) == (M, C) and t.stride(1) == 1 and t.stride(0) % 4 == 0
    ldd = dq.stride(0)
    assert dk.stride(0) == ldd and dv.stride(0) == ldd
    lib().attention_bwd_h16io(_ST16[q.dtype], _p(q), _p(k), _p(v), _p(o), _p(d_o), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), B, T, nh,
                              C // nh, ldq, C, ldd, float(drop_p), seed, seed_off, ws.ptr, ws.nbytes, _stream())
    return dq, dk, dv


# ---- feature-map kernels of the model walk (csrc/spatial.hip): NHWC maps of the walk's storage (fp32 / bf16 / f16, one dtype per
# call), tokens (B * T * C elements) and pooled vectors fp32; every output is the caller's tensor ----
def _chkmap(t, *shape, dtype=None):
    (_chk if t.dtype == F32 else _chk16)(t, *shape)
    assert dtype is None or t.dtype == dtype, (t.dtype, dtype)


def pack_input(src, dst, t, normalize):
    """NCHW fp32 frames src [B, cin, H, W] -> frame slot t of the stem input dst [B * S, H, W, 4], normalize_imagenet fused"""
    B, cin, H, W = src.shape
    S = dst.shape[0] // B
    _chkmap(dst, B * S, H, W, 4)
    assert src.dtype == F32 and src.is_cuda and 0 <= t < S, (src.dtype, src.device, t, S)
    if dst.dtype == F32:
        lib().pack_input(_p(src), _p(dst), B, cin, H, W, 4, S, t, int(normalize), _stream())
    else:
        lib().pack_input_h16(_ST16[dst.dtype], _p(src), _p(dst), B, cin, H, W, S, t, int(normalize), _stream())


def avgpool_tokens_fwd(feat, pos_emb_ptr, tokens, frames_per_sample, mod_off, T, drop_p=0.0, seed=0, seed_off=0):
    """token rows mod_off.. of each sample = embd_drop(8 x 8 average pool of its frames in feat [N, H, H, C] + pos_emb)"""
    N, H, _, C = feat.shape
    _chkmap(feat, N, H, H, C)
    _chk(tokens, N // frames_per_sample, T, C)
    _launch(lib().avgpool_tokens_fwd, lib().h16_avgpool_tokens_fwd, feat.dtype, _p(feat), pos_emb_ptr, _p(tokens), N, H, C,
            frames_per_sample, mod_off, T, float(drop_p), seed, seed_off)


def avgpool_tokens_bwd(dtok, dfeat_in, dfeat, frames_per_sample, mod_off, T):
    """dfeat = dfeat_in + the token gradient dtok spread back over the pooling windows"""
    N, H, _, C = dfeat.shape
    _chkmap(dfeat, N, H, H, C)
    _chkmap(dfeat_in, N, H, H, C, dtype=dfeat.dtype)
    _chk(dtok)
    assert dtok.numel() == N // frames_per_sample * T * C, (tuple(dtok.shape), N, frames_per_sample, T, C)
    _launch(lib().avgpool_tokens_bwd, lib().h16_avgpool_tokens_bwd, dfeat.dtype, _p(dtok), _p(dfeat_in), _p(dfeat), N, H, C,
            frames_per_sample, mod_off, T)


def upsample_add_fwd(feat, tokens, out, frames_per_sample, mod_off, T):
    """out = feat [N, H, H, C] + the bilinear upsampling of each frame's 8 x 8 token block"""
    N, H, _, C = feat.shape
    _chkmap(feat, N, H, H, C)
    _chkmap(out, N, H, H, C, dtype=feat.dtype)
    _chk(tokens)
    assert tokens.numel() == N // frames_per_sample * T * C, (tuple(tokens.shape), N, frames_per_sample, T, C)
    _launch(lib().upsample_add_fwd, lib().h16_upsample_add_fwd, feat.dtype, _p(feat), _p(tokens), _p(out), N, H, C,
            frames_per_sample, mod_off, T)


def upsample_add_bwd(dout, dtok, frames_per_sample, mod_off, T):
    """the token gradient of upsample_add_fwd, written to the token rows of dtok that the forward read"""
    N, H, _, C = dout.shape
    _chkmap(dout, N, H, H, C)
    _chk(dtok)
    assert dtok.numel() == N // frames_per_sample * T * C, (tuple(dtok.shape), N, frames_per_sample, T, C)
    _launch(lib().upsample_add_bwd, lib().h16_upsample_add_bwd, dout.dtype, _p(dout), _p(dtok), N, H, C, frames_per_sample,
            mod_off, T)


def _map_group(ins, outs, fps, offs, ntok, T, C, dtype):
    """the descriptor array of a grouped glue launch over the three modality maps of a stage -> (descs, st, B, H)"""
    assert len(ins) == len(fps) == len(offs) == 3 and (outs is None or len(outs) == 3)
    ref = ins[0] if ins[0] is not None else outs[0]
    _, H, _, _ = ref.shape
    assert ref.shape[0] % fps[0] == 0 and ntok % (T * C) == 0
    B = ref.shape[0] // fps[0]
    assert ntok == B * T * C, (ntok, B, T, C)
    descs = (_MapDesc * 3)()
    for m in range(3):
        for t in (ins[m], outs[m] if outs is not None else None):
            if t is not None:
                _chkmap(t, B * fps[m], H, H, C, dtype=dtype)
        assert 0 <= offs[m] and offs[m] + fps[m] * 64 <= T, (offs[m], fps[m], T)
        descs[m].inp, descs[m].out = _p(ins[m]), _p(outs[m]) if outs is not None else 0
        descs[m].frames_per_sample, descs[m].mod_off = fps[m], offs[m]
    return descs, (0 if dtype == F32 else _ST16[dtype]), B, H


def avgpool_tokens_fwd3(feats, pos_emb_ptr, tokens, fps, offs, T, drop_p=0.0, seed=0, seed_off=0):
    """avgpool_tokens_fwd of the three modality maps feats (frames per sample fps[m], first token row offs[m]) in one launch"""
    C = feats[0].shape[3]
    _chk(tokens)
    descs, st, B, H = _map_group(feats, None, fps, offs, tokens.numel(), T, C, feats[0].dtype)
    lib().avgpool_tokens_fwd3(st, ctypes.addressof(descs), pos_emb_ptr, _p(tokens), B, H, C, T, float(drop_p), seed, seed_off,
                              _stream())


def avgpool_tokens_bwd3(dtok, dfeats_in, dfeats, fps, offs, T):
    """avgpool_tokens_bwd of the three modality maps in one launch"""
    C = dfeats[0].shape[3]
    _chk(dtok)
    descs, st, B, H = _map_group(dfeats_in, dfeats, fps, offs, dtok.numel(), T, C, dfeats[0].dtype)
    lib().avgpool_tokens_bwd3(st, ctypes.addressof(descs), _p(dtok), B, H, C, T, _stream())


def upsample_add_fwd3(feats, tokens, outs, fps, offs, T):
    """upsample_add_fwd of the three modality maps in one launch"""
    C = feats[0].shape[3]
    _chk(tokens)
    descs, st, B, H = _map_group(feats, outs, fps, offs, tokens.numel(), T, C, feats[0].dtype)
    lib().upsample_add_fwd3(st, ctypes.addressof(descs), _p(tokens), B, H, C, T, _stream())


def upsample_add_bwd3(douts, dtok, fps, offs, T):
    """upsample_add_bwd of the three modality maps in one launch"""
    C = douts[0].shape[3]
    _chk(dtok)
    descs, st, B, H = _map_group(douts, None, fps, offs, dtok.numel(), T, C, douts[0].dtype)
    assert 5 * (H // 8) <= 64, H
    lib().upsample_add_bwd3(st, ctypes.addressof(descs), _p(dtok), B, H, C, T, _stream())


def global_pool(feat, pooled):
    """pooled [N, C] = mean over the positions of feat [N, 8, 8, C]"""
    N, C = pooled.shape
    _chkmap(feat, N, 8, 8, C)
    _chk(pooled)
    _launch(lib().global_pool, lib().h16_global_pool, feat.dtype, _p(feat), _p(pooled), N, C)


def head_bwd(dfused, dfeat, frames_per_sample):
    """dfeat [N, 8, 8, C] = backward of global_pool + the sum over frames, from dfused [B, C]"""
    N, _, _, C = dfeat.shape
    _chkmap(dfeat, N, 8, 8, C)
    _chk(dfused, N // frames_per_sample, C)
    _launch(lib().head_bwd, lib().h16_head_bwd, dfeat.dtype, _p(dfused), _p(dfeat), N, C, frames_per_sample)


# ------------------------------------------------------------------------------------------------
# Mamba layer (csrc/mamba.hip): token-major [B*L, D] operands that may be column blocks of a wider matrix.  The conv and the
# scan run on fp32, bf16 or f16 storage, named by the dtype of their first wide operand (x / u): the operands that follow it
# (conv: x, y, dy, dx; scan: u, z, y, dy, dz) all have that dtype, every other operand, the parameters and their gradients
# are fp32 (the storage map of include/ds6g.h).  Each operand is checked against the dtype that map gives it, so no 16-bit
# buffer is read as fp32 or the other way round.
def _rows_al(t, M, C, dtype=F32):
    """[M, C] operand of `dtype` (fp32, bf16 or f16) whose rows may be a column block of a wider matrix -> its row stride in
    elements of that type: whole 16-byte pieces (4 fp32, 8 16-bit elements) from a 16-byte aligned base"""
    assert dtype == F32 or dtype in _ST16, dtype
    assert t.dtype == dtype and t.is_cuda and tuple(t.shape) == (M, C) and t.stride(1) == 1, \
        (t.dtype, dtype, tuple(t.shape), (M, C), t.stride())
    s0 = t.stride(0)
    if dtype == F32:   # fp32 rows also have to be whole pieces apart, and more than one row may not overlap
        assert s0 % 4 == 0 and (M == 1 or s0 >= C), (s0, C)
    ld = max(s0, C)   # a one-row view reports an arbitrary stride
    assert t.data_ptr() % 16 == 0 and ld % (16 // t.element_size()) == 0, (t.data_ptr(), ld)
    return ld


def _vec(t, *shape):
    assert t.dtype == F32 and t.is_cuda and t.is_contiguous() and t.numel() == _prod(shape) and t.data_ptr() % 16 == 0, \
        (t.dtype, t.device, tuple(t.shape), shape)
    return t.data_ptr()


def _dst(t, *shape):
    """a gradient destination: the caller's fp32 tensor of this many elements, or a raw 16-byte aligned device pointer (a
    slice of a gradient arena) -> the pointer"""
    if isinstance(t, int):
        assert t and t % 16 == 0, t
        return t
    return _vec(t, *shape)


def _prod(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def selective_scan_chunk():
    return int(lib().selective_scan_chunk())


def copy_cols(src, dst):
    """dst[:, :] = src[:, :] for two [M, C] views of different row strides (C % 4 == 0)"""
    M, C = src.shape
    assert C % 4 == 0 and M > 0
    lib().copy_cols(_p(src), _rows_al(src, M, C), _p(dst), _rows_al(dst, M, C), M, C, _stream())
    return dst


def causal_conv1d_silu_fwd(x, w, bias, B, L, reverse=False):
    """silu(causal depthwise conv1d(x) + bias): x [B*L, D] (a column block allowed), w conv1d.weight (D, 1, 4) -> [B*L, D] of
    x's dtype"""
    M, D = x.shape
    assert M == B * L and D % 128 == 0
    st = x.dtype
    y = torch.empty((M, D), dtype=st, device=x.device)
    _launch(lib().causal_conv1d_silu_fwd, lib().h16_causal_conv1d_silu_fwd, st, _p(x), _rows_al(x, M, D, st),
            _vec(w, D, 1, 4), _vec(bias, D), _p(y), D, B, L, D, int(reverse))
    return y


def causal_conv1d_silu_bwd(x, w, bias, dy, dx, B, L, ws: Workspace, reverse=False, out=None):
    """-> (dw (D, 1, 4), dbias (D,)), fp32; dx [B*L, D] is written in place (a column block allowed); dy and dx have x's dtype.
    out: the caller's (dw, dbias) tensors or device pointers, written (not added to) instead of two fresh tensors"""
    M, D = x.shape
    assert M == B * L and D % 128 == 0
    assert ws.nbytes >= int(lib().causal_conv1d_workspace_bytes(B, L, D)), "workspace too small for causal_conv1d_silu_bwd"
    if out is None:
        out = (torch.empty((D, 1, 4), dtype=F32, device=x.device), torch.empty((D,), dtype=F32, device=x.device))
    dw, db = out
    st = x.dtype
    _launch(lib().causal_conv1d_silu_bwd, lib().h16_causal_conv1d_silu_bwd, st, _p(x), _rows_al(x, M, D, st),
            _vec(w, D, 1, 4), _vec(bias, D), _p(dy), _rows_al(dy, M, D, st), _p(dx), _rows_al(dx, M, D, st), _dst(dw, D, 1, 4),
            _dst(db, D), B, L, D, int(reverse), ws.ptr, ws.nbytes)
    return dw, db


def selective_scan_fwd(u, delta_raw, dt_bias, A_log, Bm, Cm, Dp, z, B, L, ws: Workspace, reverse=False, save=False):
    """-> (y [B*L, D] of u's dtype, saved or None).  u / z: [B*L, D] of one dtype, delta_raw: [B*L, D], Bm / Cm: [B*L, 16]
    fp32 (column blocks allowed); dt_bias, Dp: (D,), A_log: (D, 16).  save: also return the fp32 chunk-start states
    selective_scan_bwd needs."""
    M, D = u.shape
    assert M == B * L and D % 128 == 0
    assert ws.nbytes >= int(lib().selective_scan_workspace_bytes(B, L, D)), "workspace too small for selective_scan_fwd"
    st = u.dtype
    y = torch.empty((M, D), dtype=st, device=u.device)
    saved = torch.empty(int(lib().selective_scan_saved_floats(B, L, D)), dtype=F32, device=u.device) if save else None
    _launch(lib().selective_scan_fwd, lib().h16_selective_scan_fwd, st, _p(u), _rows_al(u, M, D, st), _p(delta_raw),
            _rows_al(delta_raw, M, D), _vec(dt_bias, D), _vec(A_log, D, 16), _p(Bm), _rows_al(Bm, M, 16), _p(Cm),
            _rows_al(Cm, M, 16), _vec(Dp, D), _p(z), _rows_al(z, M, D, st), _p(y), D, _p(saved), B, L, D, int(reverse), ws.ptr,
            ws.nbytes)
    return y, saved


def selective_scan_bwd(u, delta_raw, dt_bias, A_log, Bm, Cm, Dp, z, dy, saved, du, ddelta, dBm, dCm, dz, B, L,
                       ws: Workspace, reverse=False, out=None):
    """writes dz [B*L, D] of u's dtype (as are z and dy), fp32 du, ddelta (= d delta_raw) [B*L, D] and dBm, dCm [B*L, 16] in
    place (column blocks allowed) -> fp32 (dA_log (D, 16), dD (D,)).  out: the caller's (dA_log, dD) tensors or device
    pointers, written (not added to)"""
    M, D = u.shape
    assert M == B * L and D % 128 == 0
    assert ws.nbytes >= int(lib().selective_scan_workspace_bytes(B, L, D)), "workspace too small for selective_scan_bwd"
    assert saved.dtype == F32 and saved.is_cuda and saved.is_contiguous() and \
        saved.numel() == int(lib().selective_scan_saved_floats(B, L, D)), tuple(saved.shape)
    if out is None:
        out = (torch.empty((D, 16), dtype=F32, device=u.device), torch.empty((D,), dtype=F32, device=u.device))
    dA, dD = out
    st = u.dtype
    _launch(lib().selective_scan_bwd, lib().h16_selective_scan_bwd, st, _p(u), _rows_al(u, M, D, st), _p(delta_raw),
            _rows_al(delta_raw, M, D), _vec(dt_bias, D), _vec(A_log, D, 16), _p(Bm), _rows_al(Bm, M, 16), _p(Cm),
            _rows_al(Cm, M, 16), _vec(Dp, D), _p(z), _rows_al(z, M, D, st), _p(dy), _rows_al(dy, M, D, st), _p(saved), _p(du),
            _rows_al(du, M, D), _p(ddelta), _rows_al(ddelta, M, D), _p(dBm), _rows_al(dBm, M, 16), _p(dCm),
            _rows_al(dCm, M, 16), _p(dz), _rows_al(dz, M, D, st), _dst(dA, D, 16), _dst(dD, D), B, L, D, int(reverse), ws.ptr,
            ws.nbytes)
    return dA, dD


# The layer's conv and scan for a frozen model (csrc/mamba_infer.hip): forward only, no tape, one launch for ndir = 1 or 2
# directions.  The operand rules are the ones above; x_dbl and every parameter are fp32 on every storage.
class _MambaConvDir(ctypes.Structure):     # ds6g_mamba_conv_dir
    _fields_ = [("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("ld_x", ctypes.c_int), ("reverse", ctypes.c_int)]


class _MambaScanDir(ctypes.Structure):     # ds6g_mamba_scan_dir
    _fields_ = [("u", ctypes.c_void_p), ("z", ctypes.c_void_p), ("x_dbl", ctypes.c_void_p), ("dt_w", ctypes.c_void_p),
                ("dt_b", ctypes.c_void_p), ("A_log", ctypes.c_void_p), ("D", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("ld_u", ctypes.c_int), ("ld_z", ctypes.c_int), ("ld_x", ctypes.c_int), ("reverse", ctypes.c_int)]


def mamba_scan_fwd_grouped_workspace_bytes(B, L, D, ndir):
    return int(lib().mamba_scan_fwd_grouped_workspace_size(B, L, D, ndir))


def mamba_conv_fwd_grouped(dirs, B, L):
    """dirs: one or two (x, w, bias, reverse) - x [B*L, D] (a column block allowed), conv1d.weight (D, 1, 4), conv1d.bias (D,) -
    of one D and one dtype -> the list of silu(causal depthwise conv1d(x) + bias) [B*L, D], one per direction, from ONE launch;
    each equals causal_conv1d_silu_fwd on the same operands bit for bit"""
    n = len(dirs)
    assert n in (1, 2), n
    M, D = dirs[0][0].shape
    st = dirs[0][0].dtype
    assert M == B * L and D % 128 == 0
    descs = (_MambaConvDir * n)()
    ys = []
    for d, (x, w, bias, reverse) in zip(descs, dirs):
        y = torch.empty((M, D), dtype=st, device=x.device)
        d.x, d.ld_x, d.w, d.bias, d.y, d.reverse = _p(x), _rows_al(x, M, D, st), _vec(w, D, 1, 4), _vec(bias, D), _p(y), \
            int(bool(reverse))
        ys.append(y)
    _launch(lib().mamba_conv_fwd_grouped, lib().h16_mamba_conv_fwd_grouped, st, descs, n, B, L, D)
    return ys


def mamba_scan_fwd_grouped(dirs, B, L, r, ws: Workspace):
    """dirs: one or two (u, z, x_dbl, dt_w, dt_b, A_log, Dp, reverse): u / z [B*L, D] of one dtype (column blocks allowed);
    x_dbl [B*L, >= r + 32] fp32, read in place as dt | Bm | Cm; dt_proj.weight (D, r), dt_proj.bias (D,), A_log (D, 16),
    D (D,) fp32 -> the list of y [B*L, D] of u's dtype.  The selective scan with dt_proj evaluated in its staging prologue, no
    tape; three launches for all directions, one when L fits a chunk"""
    n = len(dirs)
    assert n in (1, 2), n
    M, D = dirs[0][0].shape
    st = dirs[0][0].dtype
    assert M == B * L and D % 128 == 0 and r % 4 == 0 and 4 <= r <= 32, (M, B, L, D, r)
    assert ws.nbytes >= mamba_scan_fwd_grouped_workspace_bytes(B, L, D, n), "workspace too small for mamba_scan_fwd_grouped"
    descs = (_MambaScanDir * n)()
    ys = []
    for d, (u, z, x_dbl, dt_w, dt_b, A_log, Dp, reverse) in zip(descs, dirs):
        y = torch.empty((M, D), dtype=st, device=u.device)
        n_x = x_dbl.shape[1]
        assert n_x >= r + 32, (n_x, r)
        d.u, d.ld_u, d.z, d.ld_z = _p(u), _rows_al(u, M, D, st), _p(z), _rows_al(z, M, D, st)
        d.x_dbl, d.ld_x = _p(x_dbl), _rows_al(x_dbl, M, n_x)
        d.dt_w, d.dt_b, d.A_log, d.D = _vec(dt_w, D, r), _vec(dt_b, D), _vec(A_log, D, 16), _vec(Dp, D)
        d.y, d.reverse = _p(y), int(bool(reverse))
        ys.append(y)
    _launch(lib().mamba_scan_fwd_grouped, lib().h16_mamba_scan_fwd_grouped, st, descs, n, B, L, D, r, ws.ptr, ws.nbytes)
    return ys


def cast_f32(src, out=None):
    """fp32 copy (exact) of a contiguous bf16 / f16 tensor whose numel is a multiple of 8"""
    _chk16(src)
    dst = out if out is not None else torch.empty(src.shape, dtype=F32, device=src.device)
    _chk(dst)
    assert dst.numel() == src.numel()
    lib().cast_h16_f32(_ST16[src.dtype], _p(src), _p(dst), src.numel(), _stream())
    return dst


# ------------------------------------------------------------------------------------------------
# Mamba fusion stage (csrc/mamba_fusion.hip)
def sample_layernorm_workspace_bytes(B, n):
    return int(lib().sample_layernorm_workspace_bytes(B, n))


def _chk_st(t, st, *shape):
    """a contiguous device tensor of the storage dtype `st` (fp32, bf16 or f16), of `shape` when given"""
    assert st == F32 or st in _ST16, st
    assert t.dtype == st and t.is_cuda and t.is_contiguous(), (t.dtype, st, t.device, t.stride())
    if shape:
        assert tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)


# The sample LayerNorm, the gate and the pool-swap pack run on fp32, bf16 or f16 storage, named by the dtype of their first wide
# operand; every other operand is checked against the stage's storage map (mamba_fusion.py): the wide operands share that
# dtype, parameters, statistics and parameter gradients are fp32.  A 16-bit piece is 8 elements: n % 8, C % 8.
def sample_layernorm_fwd(x, gamma, beta, ws: Workspace, eps=1e-5):
    """LayerNorm over ALL n values of each sample: x [B, n] (fp32 / bf16 / f16), gamma / beta n fp32 elements -> (y of x's
    dtype, fp32 mean [B], rstd [B])"""
    B, n = x.shape
    st = x.dtype
    _chk_st(x, st)
    assert n % (16 // x.element_size()) == 0 and ws.nbytes >= sample_layernorm_workspace_bytes(B, n), (B, n, ws.nbytes)
    y = torch.empty_like(x)
    mean = torch.empty(B, dtype=F32, device=x.device)
    rstd = torch.empty(B, dtype=F32, device=x.device)
    _launch(lib().sample_layernorm_fwd, lib().h16_sample_layernorm_fwd, st, _p(x), _vec(gamma, n), _vec(beta, n), _p(y),
            _p(mean), _p(rstd), B, n, eps, ws.ptr, ws.nbytes)
    return y, mean, rstd


def sample_layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, ws: Workspace, accumulate=False):
    """-> dx [B, n] of dy's dtype (x has it too); dgamma / dbeta (n fp32 elements each, the caller's tensors or device
    pointers) are written, or added to when accumulate"""
    B, n = x.shape
    st = dy.dtype
    _chk_st(dy, st, B, n)
    _chk_st(x, st)
    _chk(mean, B)
    _chk(rstd, B)
    assert n % (16 // x.element_size()) == 0 and ws.nbytes >= sample_layernorm_workspace_bytes(B, n), (B, n, ws.nbytes)
    dx = torch.empty_like(x)
    _launch(lib().sample_layernorm_bwd, lib().h16_sample_layernorm_bwd, st, _p(dy), _p(x), _p(mean), _p(rstd), _vec(gamma, n),
            _p(dx), _dst(dgamma, n), _dst(dbeta, n), B, n, int(accumulate), ws.ptr, ws.nbytes)
    return dx


def bimamba_gate_fwd(fm, bm, f2, B, L, out=None):
    """out[b, t] = bm[b, L-1-t] * (leaky_relu_0.2(f2[b, L-1-t]) + fm[b, t]); operands [B*L, C] of fm's dtype, column blocks
    allowed"""
    M, C = fm.shape
    st = fm.dtype
    assert M == B * L and C % 4 == 0
    o = out if out is not None else torch.empty((M, C), dtype=st, device=fm.device)
    _launch(lib().bimamba_gate_fwd, lib().h16_bimamba_gate_fwd, st, _p(fm), _rows_al(fm, M, C, st), _p(bm),
            _rows_al(bm, M, C, st), _p(f2), _rows_al(f2, M, C, st), _p(o), _rows_al(o, M, C, st), B, L, C)
    return o


def bimamba_gate_bwd(dout, fm, bm, f2, B, L, out=None):
    """-> (dfm, dbm, df2), each in its producer's token order and of dout's dtype (as are fm, bm, f2); `out`: three
    [B*L, C] destinations (column blocks allowed)"""
    M, C = fm.shape
    st = dout.dtype
    assert M == B * L and C % 4 == 0
    if out is None:
        out = tuple(torch.empty((M, C), dtype=st, device=fm.device) for _ in range(3))
    dfm, dbm, df2 = out
    _launch(lib().bimamba_gate_bwd, lib().h16_bimamba_gate_bwd, st, _p(dout), _rows_al(dout, M, C, st), _p(fm),
            _rows_al(fm, M, C, st), _p(bm), _rows_al(bm, M, C, st), _p(f2), _rows_al(f2, M, C, st), _p(dfm),
            _rows_al(dfm, M, C, st), _p(dbm), _rows_al(dbm, M, C, st), _p(df2), _rows_al(df2, M, C, st), B, L, C)
    return dfm, dbm, df2


def _chk_maps(maps, gps, B, S, C):
    assert C % 64 == 0 and B >= 1 and S >= 1, (B, S, C)
    for t in maps:
        _chk(t, B * S, C, 8, 8)
    _chk(gps, B, 2, C)


def swap_pack_fwd(image, lidar, radar, gps, pos_emb, B, S, drop_p=0.0, seed=0, seed_off=0):
    """three NCHW [B*S, C, 8, 8] maps + gps [B, 2, C] + pos_emb (T * C elements) -> tokens [B, T, C] = dropout(pos_emb +
    channel-swapped tokens), T = 192 S + 2"""
    C = image.shape[1]
    _chk_maps((image, lidar, radar), gps, B, S, C)
    T = 192 * S + 2
    tokens = torch.empty((B, T, C), dtype=F32, device=image.device)
    lib().swap_pack_fwd(_p(image), _p(lidar), _p(radar), _p(gps), _vec(pos_emb, T, C), _p(tokens), B, S, C, float(drop_p), seed,
                        seed_off, _stream())
    return tokens


def swap_pack_bwd(dtokens, B, S, drop_p=0.0, seed=0, seed_off=0):
    """-> (dimage, dlidar, dradar, dgps, dpos_emb (T, C)) of swap_pack_fwd from the token gradient [B, T, C]"""
    T, C = dtokens.shape[1], dtokens.shape[2]
    _chk(dtokens, B, 192 * S + 2, C)
    assert C % 64 == 0
    dev = dtokens.device
    dmaps = tuple(torch.empty((B * S, C, 8, 8), dtype=F32, device=dev) for _ in range(3))
    dgps = torch.empty((B, 2, C), dtype=F32, device=dev)
    dpos = torch.empty((T, C), dtype=F32, device=dev)
    lib().swap_pack_bwd(_p(dtokens), _p(dmaps[0]), _p(dmaps[1]), _p(dmaps[2]), _p(dgps), _p(dpos), B, S, C, float(drop_p), seed,
                        seed_off, _stream())
    return (*dmaps, dgps, dpos)


def _pool_swap_descs(ins, outs, S, C, st=F32):
    """descriptor array of the pool-swap pack: three NHWC maps [B * S, H, H, C] of the storage dtype `st` (ins[m] may be
    None) -> (descs, B, H)"""
    ref = outs[0] if outs is not None else ins[0]
    N, H, _, _ = ref.shape
    assert len(ins) == 3 and (outs is None or len(outs) == 3) and S >= 1 and N % S == 0, (len(ins), N, S)
    piece = 4 if st == F32 else 8
    assert H % 8 == 0 and 8 <= H <= 64 and C % piece == 0 and piece <= C <= 512, (H, C)
    descs = (_MapDesc * 3)()
    for m in range(3):
        for t in (ins[m], outs[m] if outs is not None else None):
            if t is not None:
                _chk_st(t, st, N, H, H, C)
                assert t.data_ptr() % 16 == 0
        descs[m].inp, descs[m].out = _p(ins[m]), _p(outs[m]) if outs is not None else 0
        descs[m].frames_per_sample, descs[m].mod_off = S, m * S * 64
    return descs, N // S, H


def pool_swap_tokens_fwd(feats, gemb, pos_emb_ptr, tokens, S, drop_p=0.0, seed=0, seed_off=0):
    """the Mamba stage's token pack on the walk's layout: tokens [B, T, C] (T = 192 S + 2) = embd_drop(pos_emb + the 8 x 8
    average pool of the three NHWC maps feats[m] [B * S, H, H, C] with swap_pack_fwd's channel swap; the two gps rows from
    gemb [B, 2, C]), one launch.  The maps' dtype (fp32 / bf16 / f16) is the tokens'; gemb and pos_emb are fp32"""
    C = feats[0].shape[3]
    st = feats[0].dtype
    descs, B, H = _pool_swap_descs(feats, None, S, C, st)
    _chk(gemb, B, 2, C)
    _chk_st(tokens, st, B, 192 * S + 2, C)
    _launch(lib().pool_swap_tokens_fwd, lib().h16_pool_swap_tokens_fwd, st, ctypes.addressof(descs), _p(gemb), pos_emb_ptr,
            _p(tokens), B, S, H, C, float(drop_p), seed, seed_off)


def pool_swap_tokens_bwd(dtokens, dfeats_in, dfeats, dgemb, dpos_ptr, accumulate, S, drop_p=0.0, seed=0, seed_off=0):
    """backward of pool_swap_tokens_fwd from dtokens [B, T, C], the mask regenerated: dfeats[q] = dfeats_in[q] (None: zero;
    may be dfeats[q] itself) + the token gradient spread back over its windows through the inverse swap; dgemb [B, 2, C]
    written; the (T, C) gradient of pos_emb at dpos_ptr written, or added to when `accumulate`.  dtokens' dtype is the maps';
    dgemb and the pos_emb gradient are fp32"""
    C = dfeats[0].shape[3]
    st = dtokens.dtype
    descs, B, H = _pool_swap_descs(dfeats_in if dfeats_in is not None else (None,) * 3, dfeats, S, C, st)
    _chk_st(dtokens, st, B, 192 * S + 2, C)
    _chk(dgemb, B, 2, C)
    _launch(lib().pool_swap_tokens_bwd, lib().h16_pool_swap_tokens_bwd, st, ctypes.addressof(descs), _p(dtokens), _p(dgemb),
            dpos_ptr, int(bool(accumulate)), B, S, H, C, float(drop_p), seed, seed_off)


def token_unpack_fwd(tokens, B, S):
    """tokens [B, T, C] -> (image, lidar, radar [B*S, C, 8, 8], gps rows [B, 2, C]), no channel swap"""
    C = tokens.shape[2]
    _chk(tokens, B, 192 * S + 2, C)
    assert C % 64 == 0
    dev = tokens.device
    maps = tuple(torch.empty((B * S, C, 8, 8), dtype=F32, device=dev) for _ in range(3))
    gps = torch.empty((B, 2, C), dtype=F32, device=dev)
    lib().token_unpack_fwd(_p(tokens), _p(maps[0]), _p(maps[1]), _p(maps[2]), _p(gps), B, S, C, _stream())
    return (*maps, gps)


def token_unpack_bwd(dimage, dlidar, dradar, dgps, B, S):
    """-> dtokens [B, T, C] from the gradients of token_unpack_fwd's four outputs"""
    C = dimage.shape[1]
    _chk_maps((dimage, dlidar, dradar), dgps, B, S, C)
    dtok = torch.empty((B, 192 * S + 2, C), dtype=F32, device=dimage.device)
    lib().token_unpack_bwd(_p(dimage), _p(dlidar), _p(dradar), _p(dgps), _p(dtok), B, S, C, _stream())
    return dtok


# ------------------------------------------------------------------------------------------------
# Temporal Mamba fusion head (csrc/time_mamba.hip)
TIME_ROWS = 17          # rows of a sample: 3 modalities x 5 frames, then the 2 gps rows
TIME_PARAM_VALUES = 36  # mlp.0.weight 25, mlp.0.bias 5, mlp_gps.0.weight 4, mlp_gps.0.bias 2


def _gps_rows(gps, B):
    """gps rows [B, 2, 512] whose samples may be strided (the last two token rows of a [B, T, 512] tensor) -> sample stride"""
    assert gps.dtype == F32 and gps.is_cuda and tuple(gps.shape) == (B, 2, 512) and gps.stride(2) == 1 and \
        gps.stride(1) == 512 and (B == 1 or (gps.stride(0) >= 1024 and gps.stride(0) % 4 == 0)), \
        (gps.dtype, tuple(gps.shape), gps.stride())
    return max(gps.stride(0), 1024) if B == 1 else gps.stride(0)   # a one-sample view reports an arbitrary stride


def time_attn_fwd(y, gps, w5, b5, w2, b2, B):
    """y [3*B*5, 512]: the shared Mamba layer's output on the modality-major batch; gps [B, 2, 512] (samples may be strided);
    w5 / b5: mlp.0, w2 / b2: mlp_gps.0 -> (out [B, 512], attn [B, 17], score [B, 17], argmax [B, 17] int32)"""
    _chk(y, 3 * B * 5, 512)
    ld = _gps_rows(gps, B)
    dev = y.device
    out = torch.empty((B, 512), dtype=F32, device=dev)
    attn = torch.empty((B, TIME_ROWS), dtype=F32, device=dev)
    score = torch.empty((B, TIME_ROWS), dtype=F32, device=dev)
    argmax = torch.empty((B, TIME_ROWS), dtype=torch.int32, device=dev)
    lib().time_attn_fwd(_p(y), _p(gps), ld, _vec(w5, 5, 5), _vec(b5, 5), _vec(w2, 2, 2), _vec(b2, 2), _p(out), _p(attn),
                        _p(score), _p(argmax), B, 5, 512, _stream())
    return out, attn, score, argmax


def time_attn_bwd(dout, y, gps, attn, score, argmax, w5, w2, B, dparams=None, accumulate=False, dst=None):
    """-> (dy [3*B*5, 512], dgps [B, 2, 512], dparams): dparams is ONE 36-float tensor (the caller's when given; added to when
    accumulate) holding dmlp.0.weight [:25], dmlp.0.bias [25:30], dmlp_gps.0.weight [30:34], dmlp_gps.0.bias [34:36], the
    per-sample shares summed over b in index order.  dst: four (device pointer, accumulate flag) pairs in that order - the
    same sums go straight to those destinations (one launch) and dparams is None"""
    _chk(dout, B, 512)
    _chk(y, 3 * B * 5, 512)
    _chk(attn, B, TIME_ROWS)
    _chk(score, B, TIME_ROWS)
    assert argmax.dtype == torch.int32 and argmax.is_cuda and argmax.is_contiguous() and tuple(argmax.shape) == (B, TIME_ROWS)
    ld = _gps_rows(gps, B)
    dev = y.device
    dy = torch.empty((3 * B * 5, 512), dtype=F32, device=dev)
    dgps = torch.empty((B, 2, 512), dtype=F32, device=dev)
    part = torch.empty((B, TIME_PARAM_VALUES), dtype=F32, device=dev)
    if dst is not None:
        assert dparams is None and not accumulate and len(dst) == 4 and all(int(p) and int(p) % 4 == 0 for p, _ in dst), dst
    elif dparams is None:
        assert not accumulate
        dparams = torch.empty(TIME_PARAM_VALUES, dtype=F32, device=dev)
    st = _stream()
    lib().time_attn_bwd(_p(dout), _p(y), _p(gps), ld, _p(attn), _p(score), _p(argmax), _vec(w5, 5, 5), _vec(w2, 2, 2), _p(dy),
                        _p(dgps), 1024, _p(part), B, 5, 512, st)
    if dst is not None:
        lib().temporal_param_grads(_p(part), B, *(v for p, a in dst for v in (int(p), int(bool(a)))), st)
        return dy, dgps, None
    lib().batch_sum(_p(part), _vec(dparams, TIME_PARAM_VALUES), TIME_PARAM_VALUES, B, TIME_PARAM_VALUES, int(accumulate), st)
    return dy, dgps, dparams


def _pool_rows3_dtype(name, maps):
    """the one storage dtype (fp32, bf16 or f16) of the maps of a head-pool call; a mixed set is refused here, on the host"""
    dts = {t.dtype for t in maps if t is not None}
    if len(dts) != 1 or not (dts <= {F32, BF16, F16}):
        raise ValueError(f"{name}: the maps must share one dtype out of fp32, bf16 and f16, got "
                         f"{[None if t is None else t.dtype for t in maps]}")
    return dts.pop()


def pool_rows3_fwd(feats, rows):
    """rows [3 * N, C] fp32 (modality-major: map m's frame n is row m * N + n) = the mean over the 64 positions of the three
    NHWC maps feats[m] [N, 8, 8, C], one launch.  The maps' dtype (fp32, bf16 or f16, one for the three) picks the kernel; a
    16-bit map needs C % 8 == 0"""
    assert len(feats) == 3
    dt = _pool_rows3_dtype("pool_rows3_fwd", feats)
    N, _, _, C = feats[0].shape
    for f in feats:
        _chkmap(f, N, 8, 8, C, dtype=dt)
    _chk(rows, 3 * N, C)
    assert C % (4 if dt == F32 else 8) == 0 and N >= 1, (N, C, dt)
    _launch(lib().pool_rows3_fwd, lib().h16_pool_rows3_fwd, dt, _p(feats[0]), _p(feats[1]), _p(feats[2]), _p(rows), N, C)
    return rows


def pool_rows3_bwd(drows, dfeats_in, dfeats):
    """backward of pool_rows3_fwd: dfeats[m] [N, 8, 8, C] = (dfeats_in[m] or 0) + drows[m * N + n] / 64 at every position, one
    launch; dfeats_in: None, or three maps each of which may be None or dfeats[m] itself.  drows is fp32; dfeats and dfeats_in
    share one dtype (fp32, bf16 or f16), which picks the kernel: on 16-bit maps the sum is formed in fp32 and rounded once"""
    assert len(dfeats) == 3
    dfeats_in = (None,) * 3 if dfeats_in is None else dfeats_in
    assert len(dfeats_in) == 3
    dt = _pool_rows3_dtype("pool_rows3_bwd", (*dfeats, *dfeats_in))
    N, _, _, C = dfeats[0].shape
    for t in (*dfeats, *dfeats_in):
        if t is not None:
            _chkmap(t, N, 8, 8, C, dtype=dt)
    _chk(drows, 3 * N, C)
    assert C % (4 if dt == F32 else 8) == 0 and N >= 1, (N, C, dt)
    _launch(lib().pool_rows3_bwd, lib().h16_pool_rows3_bwd, dt, _p(drows), *(_p(t) for t in dfeats_in),
            *(_p(t) for t in dfeats), N, C)
    return dfeats


# ---- radar cube -> range-angle / range-velocity maps (csrc/radar.hip).  The caller owns every buffer; the C side gets each
# one's length in floats and refuses a short one before any launch ----
RADAR_SAMPLES, RADAR_CHIRPS, RADAR_BINS, RADAR_MAX_ANTENNAS = 256, 128, 256, 8


def radar_scratch(N, A, device):
    """-> (R, raw, part): the scratch of the three radar launches for N frames of A antennas"""
    return (torch.empty((N, A, RADAR_SAMPLES, RADAR_CHIRPS, 2), dtype=F32, device=device),
            torch.empty((N, 2, RADAR_BINS, RADAR_BINS), dtype=F32, device=device),
            torch.empty((N, RADAR_BINS, 2, 2), dtype=F32, device=device))


def _chk_cube(cube):
    """cube: [N, A, 256, 128, 2] fp32 = torch.view_as_real of the complex64 cubes"""
    _chk(cube)
    N, A = cube.shape[:2]
    assert tuple(cube.shape) == (N, A, RADAR_SAMPLES, RADAR_CHIRPS, 2) and N >= 1 and 1 <= A <= RADAR_MAX_ANTENNAS, tuple(cube.shape)
    return N, A


def radar_range_fft(cube, R):
    """R[n, a, r, k] = FFT over the 256 samples of cube[n, a, :, k] (complex64 as interleaved floats, [N, A, 256, 128, 2])"""
    N, A = _chk_cube(cube)
    _chk(R, N, A, RADAR_SAMPLES, RADAR_CHIRPS, 2)
    lib().radar_range_fft(_p(cube), cube.numel(), _p(R), R.numel(), N, A, RADAR_SAMPLES, RADAR_CHIRPS, _stream())
    return R


def radar_maps_raw(R, raw, part, add_velocity=True):
    """raw[n, 0] = un-normalised range-angle map, raw[n, 1] = range-velocity map (only with add_velocity) of the range spectra
    R [N, A, 256, 128, 2]; part [N, 256, 2, 2] = (min, max) of every map row"""
    N, A = _chk_cube(R)
    _chk(raw, N, 2, RADAR_BINS, RADAR_BINS)
    _chk(part, N, RADAR_BINS, 2, 2)
    lib().radar_maps_raw(_p(R), R.numel(), _p(raw), raw.numel(), _p(part), part.numel(), N, A, RADAR_SAMPLES, RADAR_CHIRPS,
                         2 if add_velocity else 1, _stream())
    return raw, part


def radar_finish(raw, part, dst, t=0, add_velocity=True, flip=False):
    """min-max normalise each map of each frame and write it out.  dst [N * S, 256, 256, Cd] (NHWC): frame n goes to row
    n * S + t, channel 0 angle, 1 velocity, the other channels zero.  dst [N, 1 | 2, 256, 256] (NCHW, as many channels as maps):
    the reference's own stacked map format"""
    N = raw.shape[0]
    nch = 2 if add_velocity else 1
    _chk(raw, N, 2, RADAR_BINS, RADAR_BINS)
    _chk(part, N, RADAR_BINS, 2, 2)
    _chk(dst)
    assert dst.dim() == 4, tuple(dst.shape)
    if tuple(dst.shape[2:]) == (RADAR_BINS, RADAR_BINS):
        assert tuple(dst.shape[:2]) == (N, nch) and t == 0, (tuple(dst.shape), N, nch, t)
        Cd, S, planar = nch, 1, 1
    else:
        Cd, S, planar = dst.shape[3], dst.shape[0] // N, 0
        assert tuple(dst.shape) == (N * S, RADAR_BINS, RADAR_BINS, Cd) and Cd >= nch and 0 <= t < S, (tuple(dst.shape), N, nch, t)
    lib().radar_finish(_p(raw), raw.numel(), _p(part), part.numel(), _p(dst), dst.numel(), N, nch, Cd, S, t, int(bool(flip)),
                       planar, _stream())
    return dst
