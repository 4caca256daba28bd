/* libds6g.so - C ABI of the MI355X (gfx950) kernel library for the DeepSense6G fusion hot path.
 *
 * The reference (szy4017/DeepSense6G_TII) has no FFI: its boundary is the Python class
 * model2_seq.TransFuser (model2_seq.py:850-894).  deepsense6g_tii_amd/model.py mirrors that class
 * and binds these entry points with ctypes; every function below states the reference op
 * (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions: all pointers are DEVICE pointers (fp32 unless noted); activations are NHWC,
 * conv weights OHWI (= torch channels_last storage of an OIHW parameter), Linear weights [N][K]
 * (torch layout); `stream` is a hipStream_t; every call is asynchronous on that stream, performs
 * no allocation and no synchronisation (hipGraph-capturable).  Return 0 on success, non-zero on
 * bad arguments (1) / launch failure (2) (message on stderr).  `ws` arguments are caller-owned scratch.  Where an entry
 * point states a minimum for it (its *_workspace_bytes query, or a size in its comment), a smaller ws_bytes is refused with 3
 * (DS6G_ERR_WORKSPACE) after the argument checks and before anything is launched.  Exceptions: the fp32 ds6g_attention_fwd /
 * _bwd and ds6g_attention_fwd_bf16out / _fwd_h16 take ANY size (their query is the size that allows every split; the 16-bit
 * backwards need all of it); ds6g_grad_norm_clip refuses below the 8 + 8 * min(1024, ceil(n / 1024)) bytes that its n uses
 * (8 KiB + 8 covers every n).
 * Dropout masks are a pure function of (seed, seed_off + element index): backward regenerates
 * them, nothing is stored.
 */
#ifndef DS6G_H
#define DS6G_H
#include <stddef.h>
#include <stdint.h>
#include "ds6g_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 16-bit storage: a ds6g_h16_* / *_h16* entry point is ONE kernel over the type of its 16-bit tensors, named by its first
 * argument st16; any other value (0, fp32, has entry points of its own) returns DS6G_ERR_ARG before anything is launched.  Their
 * comments say "bf16"; with DS6G_ST_F16 read IEEE half: same layouts, v_mfma_f32_32x32x16_f16 for ..._bf16, round to nearest
 * even, beyond 65504 +-inf (never clamped: the loss scaler of step.hip finds it in the fp32 gradients and skips the step). */
#define DS6G_ST_BF16 1
#define DS6G_ST_F16 2
int ds6g_version(void);
/* which implicit-GEMM instantiation the last conv/linear call launched: 10000*wide + 1000*epilogue + 100*walk +
 * 10*mode + tile (wide 1 = 32-column k-tiles, 0 = 16; epilogue 1 = fused bias/ReLU/dropout/residual epilogue, 0 = plain
 * store; walk 1 = wave-uniform k walk, 0 = general walk; mode 0 fwd, 1 dgrad, 2 wgrad; tile 0 128x128, 1 128x64,
 * 2 64x64), i.e. the template arguments of igemm_kernel<mode, BM, BN, epilogue, BK, bf16, walk> as rocprofv3 prints
 * them.  Bench instrumentation only. */
int ds6g_last_igemm_variant(void);
/* bench instrumentation: between profile_begin and profile_end every implicit-GEMM KERNEL launch (not the split-K
 * reduction that may follow it) is bracketed by HIP events on its launch stream.  profile_end synchronises and returns
 * the number of records written to the three arrays (variant code as above, GEMM flops 2*M*N*K as launched, elapsed
 * milliseconds).  Not thread-safe; bench.py only. */
int ds6g_profile_begin(int max_records);
int ds6g_profile_end(int* variants, double* flops, float* ms, int cap);
/* test instrumentation: the number of slab-sum launches the calling thread's last attention backward made (0: no split; 1: the
 * dK, dV and dQ slabs reduced by one launch; 2: dK / dV and dQ apart; 3: the two-pass hd = 128 form) */
int ds6g_last_attention_bwd_slab_sums(void);
/* test instrumentation, host arithmetic only (no GPU needed): the launch plan that the attention forward (backward = 0) or
 * backward of storage `kind` (DS6G_ATTN_KIND_*, ds6g_types.h) would run for this shape and workspace size (0 for a null ws)
 * under the process's current compute mode, debug flags and environment - the entry points run what this very planner
 * returns - or the refusal of that call: DS6G_ERR_WORKSPACE where a 16-bit backward gets less than
 * ds6g_attention_workspace_bytes, DS6G_ERR_ARG where it meets the switched-off hand-over form (or for a bad shape). */
int ds6g_attention_plan(int backward, int kind, int B, int T, int nh, int hd, int ld, size_t ws_bytes, ds6g_attn_plan* plan);
/* test instrumentation, host arithmetic only (no GPU needed): the launch that the conv / linear entry point `op` (DS6G_GEMM_CONV_FWD
 * ..., ds6g_types.h) of storage `family` (DS6G_GEMM_F32: ds6g_conv2d_* / ds6g_linear_*; DS6G_GEMM_H16: ds6g_h16_*) would make for
 * this shape - a linear over M rows as N = H = 1, W = M, C = in features, K = out features, R = S = stride = 1, pad = 0 - these
 * `flags` (DS6G_GEMM_EPILOGUE | _OUT16 | _ACCUMULATE | _DBIAS) and this workspace size under the process's current compute mode,
 * debug flags and environment - the entry points run what this very planner (csrc/gemm_plan.h) returns - or the refusal of
 * that call: DS6G_ERR_ARG for a shape the entry point does not take, a size beyond the 2 GiB buffer limit, a 16-bit weight
 * gradient without a uniform k walk, or a split-K reduction whose slabs do not fit ws_bytes; DS6G_ERR_WORKSPACE for
 * ds6g_h16_conv2d_fwd_bnstats below its workspace query.  The type is named with its tag: the function has the same name. */
int ds6g_gemm_plan(int family, int op, int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int flags,
                   size_t ws_bytes, struct ds6g_gemm_plan* plan);
/* ablation switches for kernel timing experiments (results become wrong); 0 = normal operation.  0x08000000 keeps results
 * bit-identical: the hand-over attention backward reduces its dK / dV slabs and its dQ slabs in two launches, not one. */
int ds6g_set_debug_flags(int flags);
/* multi-GPU rehearsal on one GPU: keep `workgroups` (<= 256) workgroups of 256 threads with `lds_bytes` (<= 64 KiB) of LDS
 * each resident for `microseconds` (<= 2 s; every wave leaves on time) on `stream` - a stand-in for the channel workgroups an
 * RCCL all-reduce keeps on a few CUs while the backward pass runs (train2_seq.py:538 -> dist.py). */
int ds6g_debug_occupy_cus(int workgroups, int lds_bytes, int microseconds, void* stream);
/* matrix-core mode of the conv / linear / attention kernels (process-wide).  Everything else (BN, LN, softmax, loss,
 * AdamW, every accumulator) stays fp32 in every mode.  Returns DS6G_ERR_ARG for any other value.
 *   0 (default) "f32"   exact fp32 MFMA (v_mfma_f32_32x32x2_f32) - the parity path, 1e-3 bar against the reference.
 *   1           "bf16"  the "bf16 forward/backward" throughput configuration of BASELINE.json configs[1] / [4]: the
 *                       fp32-storage entry points round their operands to bf16 (RNE) between the LDS fragment and the
 *                       matrix core; the host (model.py) additionally routes every conv / linear but the 4-channel
 *                       stems, and attention, to the 16-bit-STORAGE entry points (ds6g_h16_*, *_h16*) with DS6G_ST_BF16:
 *                       activations, their gradients and a per-step weight shadow are bf16 in HBM; fp32 master weights.
 *   2           "f32x3" split bf16: each fp32 operand a = hi + lo with hi = bf16(a), lo = bf16(a - hi); a*b is
 *                       evaluated as hi*hi + hi*lo + lo*hi on the bf16 matrix cores with fp32 accumulation - relative
 *                       product error <= ~2^-16 (between fp32 and TF32), fp32 storage.
 *   3           "f32x6" three-way truncating split (a == hi + mid + lo exactly), the six products above 2^-24 summed
 *                       smallest first: fp32-grade products on the bf16 matrix cores, fp32 storage; the 3x3 / stride-1
 *                       convs keep the fp32 Winograd kernels.
 *   4                   unused (refused).
 *   5           "f16"   f16 storage: the host routes the same convs / linears / attention / BN / LN / pooling as in "bf16" to
 *                       the same entry points with st16 = DS6G_ST_F16; every fp32-storage kernel runs exactly as in mode 0
 *                       (their operand mode stays 0), so eval, the small linears and the fp32 stems are exact fp32. */
int ds6g_set_compute_mode(int mode);
int ds6g_get_compute_mode(void);

/* Dropout masks are a pure function of (seed, counter).  Elementwise sites (embd_drop, resid_drop: ds6g_dropout, the
 * linear epilogues, ds6g_layernorm_bwd's dx_drop, the token-pool kernels) use counter = seed_off + element index, one
 * hash (lowbias32 finalizer on the keyed counter) per element, dropped when hash < floor(p * 2^32).  The attention kernels
 * (attn_drop on the [B * nh][T][T] probabilities) draw FOUR decisions per hash: element (row, key), row = (b * nh + h) * T +
 * query, uses counter = seed_off + row * ceil(T / 4) + (key >> 2) and the 16-bit half (key & 3) of the two words derived
 * from that counter, dropped when the half < floor(p * 2^16) (csrc/common.h Ds6gKeep4Base; numpy restatement in
 * tests/test_bench_shapes_gpu.py::_keep_bits_attn); kept probabilities are scaled by 1 / (1 - floor(p * 2^16) / 2^16), the
 * probability the 16-bit decisions realise (p < 2^-16: no dropout); the elementwise sites scale by 1 / (1 - p).  seed_off is a launch argument, frozen when a
 * training step is captured into a hipGraph; ds6g_set_dropout_salt(dev_ptr) makes every kernel that draws a mask add the
 * uint64 at dev_ptr to seed_off when it RUNS (the caller advances that value on the device once per step), so replays draw
 * fresh masks.  Applies to the launches of the calling thread from now on (thread-local); NULL switches it off. */
int ds6g_set_dropout_salt(const uint64_t* dev_ptr);

/* ---- igemm.hip : Conv2d / Linear as implicit GEMM on v_mfma_f32_32x32x2_f32 -------------------
 * Conv2d(bias=False) of the ResNet trunks: model2_seq.py:495,500,505 (7x7/2 stems), :510-512,
 * 528-530,546-548,565-567 (BasicBlock 3x3 and 1x1/2 downsample).  C and K multiples of 4. */
int ds6g_conv2d_fwd(const float* x, const float* w, float* y, int N, int H, int W, int C, int K, int R, int S,
                    int stride, int pad, void* stream);
int ds6g_conv2d_dgrad(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int K, int R, int S,
                      int stride, int pad, int accumulate, void* stream);
int ds6g_conv2d_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K, int R, int S,
                      int stride, int pad, int accumulate, float* ws, size_t ws_bytes, void* stream);
/* inference form of Conv2d + eval-mode BatchNorm2d (+ identity) (+ ReLU) of the torchvision BasicBlock / stem
 * (call sites model2_seq.py:495-512,528-530,546-548,565-567 under model.eval(), train2_seq.py:161): the BN is folded
 * into w / bias by ds6g_bn_fold, y = act(conv(x, w) + bias [+ residual]); relu: 0 none, 1 before the residual add,
 * 2 after it. */
int ds6g_conv2d_bias_act_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y, int N,
                             int H, int W, int C, int K, int R, int S, int stride, int pad, int relu, void* stream);
/* w_out[o][tap][c] = w[o][tap][c] * gamma[o]/sqrt(running_var[o]+eps) (c >= cin: zero padding up to cpad channels),
 * bias_out[o] = beta[o] - running_mean[o] * gamma[o]/sqrt(running_var[o]+eps);  w: [K][taps][cin] (OHWI). */
int ds6g_bn_fold(const float* w, const float* gamma, const float* beta, const float* running_mean,
                 const float* running_var, float eps, float* w_out, float* bias_out, int K, int taps, int cin, int cpad,
                 void* stream);
/* the same fold for the frozen inference engine's 16-bit filters (TransFuser.freeze_inference): the scale is applied in
 * fp32 and the product rounded ONCE (nearest even) on the store to w_out [K][taps][cpad] bf16 / f16; bias_out stays fp32. */
int ds6g_bn_fold_h16(int st16, const float* w, const float* gamma, const float* beta, const float* running_mean,
                     const float* running_var, float eps, void* w_out, float* bias_out, int K, int taps, int cin, int cpad,
                     void* stream);
/* ---- winograd.hip : Winograd F(2x2, 3x3) for the 3x3 / stride 1 / pad 1 convolutions of the BasicBlocks
 * (model2_seq.py:510-512,528-530,546-548,565-567): 16 GEMMs on transformed 4x4 tiles, 2.25x fewer MFMA FLOPs.
 * winograd_weights builds U[16][K][C] = G g G^T from the OHWI filter (transpose_flip = 1: the dgrad filter, i.e.
 * U[16][C][K] of the channel-swapped, 180-degree-rotated filter; 2: both in one launch, forward first, into 2x the
 * floats), stored in MFMA fragment order; conv3x3_winograd_fwd computes
 * y[N][H][W][K] (+)= conv(x[N][H][W][C]) from it (call it with dy and the dgrad filter to obtain dx).
 * winograd_supported: H, W even, C % 16 == 0, K % 32 == 0, W/2 a multiple of 8 or a divisor of 32. */
size_t ds6g_winograd_weight_floats(int K, int C);
int ds6g_winograd_weights(const float* w, float* u, int K, int C, int transpose_flip, void* stream);
int ds6g_winograd_supported(int N, int H, int W, int C, int K);
int ds6g_conv3x3_winograd_fwd(const float* x, const float* u, float* y, int N, int H, int W, int C, int K, int accumulate,
                              void* stream);
/* inference form: eval-mode BN folded into the filter (ds6g_bn_fold, then ds6g_winograd_weights), epilogue fused into the
 * output transform: y = act(conv(x) + bias [+ residual]); relu 0 none / 1 before / 2 after the residual add. */
int ds6g_conv3x3_winograd_bias_act_fwd(const float* x, const float* u, const float* bias, const float* residual, float* y,
                                       int N, int H, int W, int C, int K, int relu, void* stream);
/* weight gradient of the same convs in the Winograd domain (dU = sum_tiles (A dY A^T) (B^T d B), dW = G^T dU G): 4 MFMA
 * FLOPs per pixel / channel pair / filter instead of 9.  ws: scratch for the per-split dU slabs (>= 16*K*C floats; more
 * allows more splits).  Supported: H, W even, C and K multiples of 64. */
int ds6g_winograd_wgrad_supported(int N, int H, int W, int C, int K);
int ds6g_conv3x3_winograd_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int C, int K,
                                int accumulate, float* ws, size_t ws_bytes, void* stream);
/* test instrumentation, host arithmetic only: the launch that the Winograd entry point `op` (DS6G_WINO_FWD / _BIAS_ACT / _WGRAD,
 * ds6g_types.h) would make for this shape, `accumulate` and workspace size on a device of n_cu compute units (<= 0: the calling
 * thread's current device, the one case that makes a HIP call) under the process's current debug flags and environment - the
 * entry points run what this very planner (csrc/wino_plan.h) returns - or the refusal of that call: DS6G_ERR_ARG for a shape
 * ds6g_winograd_supported / _wgrad_supported refuses, DS6G_ERR_WORKSPACE for a weight gradient with less than one slab of
 * 16*K*C floats, DS6G_ERR_LAUNCH where the persistent kernel is planned and no CU count is known. */
int ds6g_winograd_plan(int op, int N, int H, int W, int C, int K, int accumulate, int n_cu, size_t ws_bytes,
                       struct ds6g_wino_plan* plan);
/* nn.Linear of the GPT blocks with fused epilogue y = residual + dropout(act(x w^T + b)):
 * model2_seq.py:97-99 (q,k,v), :109 (proj + resid_drop), :121-126 (MLP, ReLU), :131-132 (residuals). */
int ds6g_linear_fwd(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int relu,
                    const float* residual, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_linear_dgrad(const float* dy, const float* w, float* dx, int M, int N, int K, const float* relu_mask_src,
                      int accumulate, void* stream);
int ds6g_linear_wgrad(const float* x, const float* dy, float* dw, float* dbias, int M, int N, int K, int accumulate,
                      float* ws, size_t ws_bytes, void* stream);

/* ---- bgemm.hip : the same Conv2d / Linear products on bf16-STORED operands (the bf16 configuration of BASELINE configs[1]
 * and [4]: bf16 activations, a bf16 shadow of the weights refreshed by ds6g_adamw_step, fp32 accumulation; the reference has
 * no mixed precision, train2_seq.py:111-116).  x / dy / w: bf16; y / dx: bf16 when out16 else fp32; dw / dbias / bias /
 * residual: fp32.  Tiles travel HBM -> LDS as bf16 by LDS-DMA and feed v_mfma_f32_32x32x16_bf16 without conversion.
 * Shape limits (every layer of the model but the 4-channel stems): the reduction channel count is a multiple of 64, the
 * other a multiple of 8; dgrad: stride 1, or 2 with even H, W; wgrad: Wo % 64 == 0, or 64 % Wo == 0 with Ho % (64 / Wo) == 0, or a Linear. */
int ds6g_h16_conv2d_fwd(int st16, const void* x, const void* w, void* y, int out16, int N, int H, int W, int C, int K, int R,
                        int S, int stride, int pad, void* stream);
/* inference form of Conv2d + eval-mode BatchNorm2d (+ identity) (+ ReLU) on 16-bit storage (the BasicBlock convs under
 * model.eval(), model2_seq.py:510-512,528-530,546-548,565-567): the BN is folded into w (bf16, ds6g_bn_fold_h16) and bias
 * (fp32); y = act(conv(x, w) + bias [+ residual]); relu: 0 none, 1 before the residual add, 2 after it - the contract of
 * ds6g_conv2d_bias_act_fwd.  x, w, residual (nullable), y: bf16; bias and the residual are added to the fp32 accumulator
 * and the result is rounded once.  Shape limits of ds6g_h16_conv2d_fwd. */
int ds6g_h16_conv2d_bias_act_fwd(int st16, const void* x, const void* w, const float* bias, const void* residual, void* y,
                                 int N, int H, int W, int C, int K, int R, int S, int stride, int pad, int relu, void* stream);
/* conv (bf16 output) + the train-mode BatchNorm statistics of its output in one call (the BasicBlock pairs conv1 / bn1,
 * conv2 / bn2, downsample.0 / .1 of torchvision's ResNet, model2_seq.py:510-512,528-530,546-548,565-567): the conv's epilogue
 * writes per-tile column sums / sums of squares of the STORED bf16 tile, a small finalize kernel turns them into mean /
 * invstd and updates the running statistics - what ds6g_h16_bn_stats(y) computes, without its pass over y. */
size_t ds6g_h16_conv_bnstats_workspace_bytes(long M, int K);
int ds6g_h16_conv2d_fwd_bnstats(int st16, const void* x, const void* w, void* y, int N, int H, int W, int C, int K, int R,
                                int S, int stride, int pad, float eps, float momentum, float* mean, float* invstd,
                                float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream);
int ds6g_h16_conv2d_dgrad(int st16, const void* dy, const void* w, void* dx, int out16, int N, int H, int W, int C, int K,
                          int R, int S, int stride, int pad, int accumulate, void* stream);
int ds6g_h16_conv2d_wgrad(int st16, const void* x, const void* dy, float* dw, int N, int H, int W, int C, int K, int R, int S,
                          int stride, int pad, int accumulate, float* ws, size_t ws_bytes, void* stream);
/* nn.Linear of the GPT blocks (model2_seq.py:97-99,109,121-126,131-132) on bf16 operands; a fused residual add writes the
 * fp32 residual stream (out16 must be 0 then); mask_src [M][K]: bf16 (mask16) or fp32, with a bf16 dx only. */
int ds6g_h16_linear_fwd(int st16, const void* x, const void* w, const float* bias, void* y, int out16, int M, int N, int K,
                        int relu, const float* residual, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_h16_linear_dgrad(int st16, const void* dy, const void* w, void* dx, int out16, int M, int N, int K,
                          const void* mask_src, int mask16, int accumulate, void* stream);
int ds6g_h16_linear_wgrad(int st16, const void* x, const void* dy, float* dw, float* dbias, int M, int N, int K, int accumulate,
                          float* ws, size_t ws_bytes, void* stream);

/* ---- stem.hip : the 7x7 / stride 2 / pad 3 stem convs (torchvision ResNet conv1 via model2_seq.py:495,500,505) of the
 * bf16 configuration.  x [N][H][W][4] bf16 (ds6g_pack_input_h16; channels >= cin zero), w: the fp32 master filter
 * [64][7][7][cin] (OHWI), y / dy [N][H/2][W/2][64] bf16; H % 16 == 0, W % 32 == 0.  The forward also delivers the train-mode
 * BatchNorm statistics of y (mean == NULL: convolution only); ws >= ds6g_h16_stem_workspace_bytes().  The BN -> ReLU ->
 * MaxPool pass over the bf16 conv output and its backward: ds6g_h16_stem_bn_relu_maxpool_fwd / ds6g_h16_stem_bn_bwd_maxpool. */
size_t ds6g_h16_stem_workspace_bytes(void);
int ds6g_h16_stem_fwd(int st16, const void* x, const float* w, int cin, void* y, int N, int H, int W, float eps, float momentum,
                      float* mean, float* invstd, float* running_mean, float* running_var, void* ws, size_t ws_bytes,
                      void* stream);
int ds6g_h16_stem_wgrad(int st16, const void* x, const void* dy, float* dw, int cin, int N, int H, int W, int accumulate,
                        void* ws, size_t ws_bytes, void* stream);
int ds6g_h16_stem_bn_relu_maxpool_fwd(int st16, const void* x, const float* mean, const float* invstd, const float* gamma,
                                      const float* beta, void* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int ds6g_h16_stem_bn_bwd_maxpool(int st16, const void* dpool, const uint8_t* idx, const void* x, const float* mean,
                                 const float* invstd, const float* gamma, const float* relu_beta, void* dx, float* dgamma,
                                 float* dbeta, int N, int H, int W, int C, int accumulate_param_grads, void* ws,
                                 size_t ws_bytes, void* stream);
/* inference stem (conv1 + bn1 + relu + maxpool under model.eval(), model2_seq.py:495-507): the filter is prepared once per
 * snapshot - ds6g_bn_fold_h16 with cpad = 4 gives w [64][7][7][4] bf16 and the fp32 bias, ds6g_h16_stem_pack_filter lays
 * it out as the forward reads it, w_packed [64][7][8][4] - then y = relu(conv7x7/2(x, w_packed) + bias) in one launch with
 * the bias added before the one rounding (no workspace, no statistics), and ds6g_h16_maxpool3x3s2_fwd is the 3x3 / 2 /
 * pad 1 max-pool of a bf16 NHWC map without an arg-max index (C % 8 == 0). */
int ds6g_h16_stem_pack_filter(int st16, const void* w, void* w_packed, void* stream);
int ds6g_h16_stem_bias_relu_fwd(int st16, const void* x, const void* w_packed, const float* bias, void* y, int N, int H, int W,
                                void* stream);
int ds6g_h16_maxpool3x3s2_fwd(int st16, const void* x, void* y, int N, int H, int W, int C, void* stream);

/* ---- norm.hip ----------------------------------------------------------------------------------
 * BatchNorm2d in train mode (+ReLU, +residual add of BasicBlock): torchvision BasicBlock via
 * model2_seq.py:496-497,501-502,506-507 and the layer calls above; eval mode uses running stats. */
size_t ds6g_bn_workspace_bytes(long M, int C);
int ds6g_bn_stats(const float* x, long M, int C, float eps, float momentum, float* mean, float* invstd,
                  float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream);
int ds6g_bn_eval_prepare(const float* running_mean, const float* running_var, int C, float eps, float* mean,
                         float* invstd, void* stream);
int ds6g_bn_apply(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                  const float* residual, float* y, long M, int C, int relu, void* stream);
/* relu_beta (nullable, y_mask then NULL): the BN fed a ReLU with no residual in between (bn1 of a BasicBlock, stem
 * bn1): the ReLU mask is re-derived from x as (gamma * xhat + relu_beta > 0) with the forward's own arithmetic instead of
 * reading the activation tensor - one tensor read less in each of the two backward passes. */
int ds6g_bn_bwd(const float* dy, const float* y_mask, const float* x, const float* mean, const float* invstd,
                const float* gamma, const float* relu_beta, float* dx, float* dgamma, float* dbeta, float* dres, long M,
                int C, int accumulate_param_grads, void* ws, size_t ws_bytes, void* stream);
/* nn.LayerNorm(C), eps 1e-5: model2_seq.py:118-119,131-132,199,274.  C in {64,128,256,512}. */
int ds6g_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                       int M, int C, float eps, void* stream);
size_t ds6g_layernorm_bwd_workspace_bytes(int M, int C);
/* dx = add? + LN'(dy); dgamma / dbeta (+)=.  dx_drop (nullable): also writes dropout(dx; drop_p, seed, seed_off), the
 * gradient the resid_drop branch of the block below consumes (model2_seq.py:109,126), saving a separate pass. */
int ds6g_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                       const float* add, float* dx, float* dgamma, float* dbeta, int M, int C,
                       int accumulate_param_grads, float* dx_drop, float drop_p, uint64_t seed, uint64_t seed_off,
                       void* ws, size_t ws_bytes, void* stream);
/* bf16-storage path of BatchNorm2d: conv outputs, activations and their gradients are bf16 in HBM (x / residual / y /
 * dy / y_mask / dx / dres), the statistics, running stats, parameter gradients and every reduction stay fp32 / fp64. */
int ds6g_h16_bn_stats(int st16, const void* x, long M, int C, float eps, float momentum, float* mean, float* invstd,
                      float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream);
int ds6g_h16_bn_apply(int st16, const void* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      const void* residual, void* y, long M, int C, int relu, void* stream);
int ds6g_h16_bn_bwd(int st16, const void* dy, const void* y_mask, const void* x, const float* mean, const float* invstd,
                    const float* gamma, const float* relu_beta, void* dx, float* dgamma, float* dbeta, void* dres, long M,
                    int C, int accumulate_param_grads, void* ws, size_t ws_bytes, void* stream);
/* bf16-storage path (GEMM-facing tensors are bf16; statistics, the residual stream and all arithmetic stay fp32):
 * layernorm_fwd_h16out writes y as bf16; layernorm_bwd_h16 reads dy as bf16 (dy16) or fp32, writes dx fp32 and dx_drop
 * (nullable) = dropout(dx) as bf16 (drop_p = 0: a bf16 copy of dx, the next GEMM's operand). */
int ds6g_layernorm_fwd_h16out(int st16, const float* x, const float* gamma, const float* beta, void* y, float* mean,
                              float* rstd, int M, int C, float eps, void* stream);
int ds6g_layernorm_bwd_h16(int st16, const void* dy, int dy16, const float* x, const float* mean, const float* rstd,
                           const float* gamma, const float* add, float* dx, float* dgamma, float* dbeta, int M, int C,
                           int accumulate_param_grads, void* dx_drop, float drop_p, uint64_t seed, uint64_t seed_off, void* ws,
                           size_t ws_bytes, void* stream);
/* Deferred parameter gradients of LayerNorm: dgamma / dbeta feed nothing but the optimizer, so on a serial chain of
 * LayerNorms (a GPT stage's backward) their reduction need not be launched once per layer.  The *_partial forms of the two
 * backward entry points write dx (and dx_drop) as usual and leave the row-block partials of dgamma / dbeta in `partial`, the
 * caller's own buffer of >= ds6g_layernorm_bwd_workspace_bytes(M, C) bytes (less is refused with DS6G_ERR_WORKSPACE);
 * ds6g_layernorm_finalize_batched then reduces the buffers of 1 .. DS6G_LN_FINALIZE_MAX LayerNorms in ONE launch, with the
 * arithmetic and summation order of the undeferred entry points (bit-identical dgamma / dbeta).  descs is a host array
 * read during the call (the descriptors travel in the kernel's arguments: safe under stream capture); nblk =
 * cdiv(M, 16), C as for ds6g_layernorm_bwd; a count outside 1 .. 24, a null pointer or another C is DS6G_ERR_ARG and
 * launches nothing. */
/* ds6g_ln_finalize_desc {partial, nblk, C, dgamma, dbeta, accumulate} and DS6G_LN_FINALIZE_MAX: ds6g_types.h */
int ds6g_layernorm_bwd_partial(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                               const float* add, float* dx, int M, int C, float* dx_drop, float drop_p, uint64_t seed,
                               uint64_t seed_off, float* partial, size_t partial_bytes, void* stream);
int ds6g_layernorm_bwd_h16_partial(int st16, const void* dy, int dy16, const float* x, const float* mean, const float* rstd,
                                   const float* gamma, const float* add, float* dx, int M, int C, void* dx_drop, float drop_p,
                                   uint64_t seed, uint64_t seed_off, float* partial, size_t partial_bytes, void* stream);
int ds6g_layernorm_finalize_batched(const ds6g_ln_finalize_desc* descs, int count, void* stream);
/* bias gradients: out[c] (+)= sum_r x[r][c] */
size_t ds6g_colsum_workspace_bytes(long M, int C);
int ds6g_colsum(const float* x, long M, int C, float* out, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---- attention.hip : SelfAttention core, model2_seq.py:101-106 (softmax(q k^T/sqrt(hd)), attn_drop,
 * att @ v, head merge).  Head h lives at columns h*hd of every operand.  q/k/v: [B*T][ld_qkv] (ld_qkv = 3C when
 * they are column blocks of ONE fused key|query|value projection output, model2_seq.py:97-99); o / d_o: [B*T][ld];
 * dq/dk/dv: [B*T][ld_dqkv] (again 3C to write one fused gradient matrix).  hd in {16,32,64,128}.
 * ws: scratch for the split-loop partial results (any size; more allows more splits, see *_workspace_bytes).  With the
 * full *_workspace_bytes the backward hands its dS (and, hd = 128, dropped-P) tiles from the dK/dV kernel to the dQ / dV
 * kernels through ws (5 matrix products); with less it recomputes the scores in every kernel (7-8 products, same results
 * up to summation order).
 * ds6g_attention_workspace_bytes = hand-over tiles + 16 slabs of B*T*ld floats + 8 (max, sum) arrays of the split forward.
 * It is the size at which every FORM of the backward is available (and the one size the 16-bit backwards accept as a
 * minimum) - NOT the size at which every split count is: the launch plan goes on depending on ws_bytes beyond it.  The
 * hand-over backward reduces its dK, dV and dQ slabs in one launch only where all three sets fit side by side behind the
 * tiles, and at 6 or more splits each those are more than 16 slabs: B = 12, T = 642 takes 7 + 7 + 7, so that call makes
 * two slab-sum launches at the queried size and one on a larger scratch (the model passes its whole arena).
 * The split counts of the kernels, and with them the bits of the results, are the same either way. */
size_t ds6g_attention_workspace_bytes(int B, int T, int nh, int hd, int ld);
int ds6g_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int T, int nh,
                       int hd, int ld_qkv, int ld, float drop_p, uint64_t seed, uint64_t seed_off, void* ws,
                       size_t ws_bytes, void* stream);
int ds6g_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                       const float* lse, float* delta, float* dq, float* dk, float* dv, int B, int T, int nh, int hd,
                       int ld_qkv, int ld, int ld_dqkv, float drop_p, uint64_t seed, uint64_t seed_off, void* ws,
                       size_t ws_bytes, void* stream);

/* bf16-storage path: q / k / v / d_o stay fp32 (column blocks of fp32 GEMM outputs); the forward output o is written -
 * and read back by the backward - as bf16 [B*T][ld], dq / dk / dv are written as bf16 [B*T][ld_dqkv] (operands of the
 * projection GEMMs).  The backward needs the full ds6g_attention_workspace_bytes (hand-over form). */
int ds6g_attention_fwd_bf16out(const float* q, const float* k, const float* v, void* o, float* lse, int B, int T, int nh,
                               int hd, int ld_qkv, int ld, float drop_p, uint64_t seed, uint64_t seed_off, void* ws,
                               size_t ws_bytes, void* stream);
int ds6g_attention_bwd_bf16(const float* q, const float* k, const float* v, const void* o, const float* d_o,
                            const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int T, int nh, int hd,
                            int ld_qkv, int ld, int ld_dqkv, float drop_p, uint64_t seed, uint64_t seed_off, void* ws,
                            size_t ws_bytes, void* stream);

/* all operands bf16 in HBM (q / k / v [B*T][ld_qkv], o / d_o [B*T][ld], dq / dk / dv [B*T][ld_dqkv]): K / V / Q / dO tiles are
 * staged as bf16 LDS images by LDS-DMA and reach v_mfma_f32_32x32x16_bf16 unconverted (row reads: ds_read_b128, transposed
 * reads for the P.V / dS^T.Q / P^T.dO / dS.K products: ds_read_b64_tr_b16); lse, delta, the split slabs and the dS / P
 * hand-over tiles stay fp32.  ld_qkv and ld multiples of 8. */
int ds6g_attention_fwd_h16(int st16, const void* q, const void* k, const void* v, void* o, float* lse, int B, int T, int nh,
                           int hd, int ld_qkv, int ld, float drop_p, uint64_t seed, uint64_t seed_off, void* ws,
                           size_t ws_bytes, void* stream);
int ds6g_attention_bwd_h16io(int st16, const void* q, const void* k, const void* v, const void* o, const void* d_o,
                             const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int T, int nh, int hd,
                             int ld_qkv, int ld, int ld_dqkv, float drop_p, uint64_t seed, uint64_t seed_off, void* ws,
                             size_t ws_bytes, void* stream);

/* ---- input.hip : device-side counterpart of CARLA_Data.__getitem__, data2_seq.py:42-173 --------
 * pack_image_u8: decoded RGB frame batch [B][H][W][3] uint8 (data2_seq.py:110-141, before its HWC->CHW transpose) ->
 *   frame slot t of the NHWC x4 stem input [(b*frames_per_sample + t)][H][W][4], cast + normalize_imagenet
 *   (model2_seq.py:36-45) fused; flip mirrors W (data2_seq.py:144-146).
 * lidar_bev_count / lidar_bev_finish: lidar_to_histogram_features (data2_seq.py:177-211).  points: float64
 *   [npoints][point_stride] (x, y first) of nclouds clouds back to back, cloud c = [cloud_offsets[c],
 *   cloud_offsets[c+1]); xedges / yedges: nbins+1 float64 bin edges - one set, or one per cloud when edges_per_cloud
 *   (the per-scenario custom field of view, data2_seq.py:190-202) - (np.linspace in the reference, np.histogramdd
 *   semantics: half-open bins, last bin closed, outliers dropped); counts: [nclouds][nbins][nbins] uint32, must be zero
 *   on entry.  finish writes min(count, cap)/cap into channel 0 of frame slot t of an NHWC xCd tensor (flip mirrors
 *   the y axis, data2_seq.py:157-158) and re-zeroes counts.
 * soft_beam_target: target[b][k] = 1.25 * N(k; beamidx[b], 0.5) for |k - beamidx[b]| <= 5 else 0 (data2_seq.py:160-170);
 *   flip mirrors the beam axis and writes beamidx_out[b] = nbeams-1-beamidx[b] (nullable). */
int ds6g_pack_image_u8(const uint8_t* src_hwc, float* dst, int B, int H, int W, int frames_per_sample, int t, int flip,
                       void* stream);
int ds6g_lidar_bev_count(const double* points, int point_stride, const long* cloud_offsets, int nclouds,
                         long npoints, const double* xedges, const double* yedges, int edges_per_cloud, int nbins,
                         unsigned* counts, void* stream);
int ds6g_lidar_bev_finish(unsigned* counts, float* dst, int B, int nbins, int Cd, int frames_per_sample, int t, int flip,
                          int cap, void* stream);
int ds6g_soft_beam_target(const int* beamidx, float* target, int* beamidx_out, int B, int nbeams, int flip,
                          void* stream);

/* ---- radar.hip : raw radar cube -> range-angle / range-velocity maps, the offline numpy step of the reference
 * (Data_Preprocessing/Radar_data_preprocessing.py:7-23,41-42), for N frames per launch.  cube: [N][A][256][128] complex64
 * as interleaved floats (antenna, sample, chirp); S must be 256, K 128, 1 <= A <= 8; cube, R and a dst with Cd == 4 must
 * be 16-byte aligned.  Every buffer comes with its length in floats and a short one is refused before any launch; the
 * caller owns the scratch: R N*A*256*128*2 floats, raw N*2*256*256, part N*256*4.
 * radar_range_fft: R[n][a][r][k] = sum_s cube[n][a][s][k] e^(-2 pi i r s / 256).
 * radar_maps_raw: raw[n][0][r][th] = sum_k |sum_a (R[n][a][r][k] - mean_k R[n][a][r][:]) e^(-2 pi i th a / 256)| and, when
 *   nch == 2, raw[n][1][r][v] = sum_a |sum_k R[n][a][r][k] e^(-2 pi i v k / 256)| (th, v < 256); part[n][r][c][0 / 1] =
 *   min / max of row r of map c.  nch == 1 leaves plane 1 and its partials untouched.
 * radar_finish: (map - min) / (max - min) per map and frame (a constant map is NaN, as in numpy) into frame slot t of an
 *   NHWC xCd tensor dst[(n*frames_per_sample + t)][r][w][Cd], channel 0 angle, 1 velocity, channels nch..Cd-1 zero; with
 *   planar != 0 (Cd == nch, frames_per_sample == 1) dst is [N][nch][256][256] instead.  flip mirrors the w axis
 *   (data2_seq.py:144-152).  No float atomics anywhere: results are bit-reproducible. */
int ds6g_radar_range_fft(const float* cube, long cube_elems, float* R, long r_elems, int N, int A, int S, int K,
                         void* stream);
int ds6g_radar_maps_raw(const float* R, long r_elems, float* raw, long raw_elems, float* part, long part_elems, int N,
                        int A, int S, int K, int nch, void* stream);
int ds6g_radar_finish(const float* raw, long raw_elems, const float* part, long part_elems, float* dst, long dst_elems,
                      int N, int nch, int Cd, int frames_per_sample, int t, int flip, int planar, void* stream);

/* ---- gru.hip : autoregressive GRU beam-sequence head of the 30->5 variant, model2_seq_30to5.py:842-862:
 * x = 0, h = h0 (the join output); T times: h = GRUCell(x, h); x = x + Linear(h); pred[:, t] = x.  H must be 64.
 * w_ih / w_hh: [3H][H] (gate rows r, z, n as in nn.GRUCell), b_ih / b_hh: [3H], w_out: [H][H], b_out: [H].
 * saved: B*T*6*H floats (gru_head_saved_floats) written by fwd for bwd, or NULL for inference.
 * bwd writes dh0 [B][H] and one parameter-gradient slab per sample (gru_head_slab_floats each, laid out dW_ih, dW_hh,
 * db_ih, db_hh, dW_out, db_out); sum the slabs over the batch with ds6g_batch_sum. */
size_t ds6g_gru_head_saved_floats(int B, int T);
size_t ds6g_gru_head_slab_floats(void);
int ds6g_gru_head_fwd(const float* h0, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                      const float* w_out, const float* b_out, float* pred, float* saved, int B, int T, int H,
                      void* stream);
int ds6g_gru_head_bwd(const float* dpred, const float* h0, const float* saved, const float* w_ih, const float* w_hh,
                      const float* w_out, float* dh0, float* slabs, int B, int T, int H, void* stream);

/* ---- mamba.hip : the two non-GEMM operators of mamba_ssm.Mamba(d_model, d_state=16, d_conv=4, expand=2), the layer under
 * every model the reference's training script builds (mambafuser_seq.py:83-101 MambaBlock's forward / backward_mamba pair,
 * :240 MambaFusion, :261-263 TimeMamba); the four projections are ds6g_linear_*.  Token-major fp32: row = b * L + t, D =
 * d_inner channels contiguous; every operand is pointer + row stride in floats (stride >= width, % 4 == 0, pointers 16-byte
 * aligned), so x / z are read as the column halves of in_proj's output and dt / Bm / Cm as column slices of x_proj's.
 * D % 128 == 0.  reverse != 0 walks each sequence back to front (the result of flip -> op -> flip, without the copies).
 *   causal_conv1d_silu   y_t = silu(bias + sum_k w[d][k] x_{t-3+k}), zeros before t = 0; w: conv1d.weight (D, 1, 4).  bwd
 *                        recomputes the pre-activation from x; dw / dbias are written (not accumulated) from per-workgroup
 *                        partials reduced in a fixed order.  ws >= ds6g_causal_conv1d_workspace_bytes.
 *   selective_scan_fwd   delta = softplus(delta_raw + dt_bias) (v > 20: v); h_t = exp(delta_t A) h_{t-1} + delta_t u_t Bm_t,
 *                        A = -exp(A_log) (D, 16); y_t = (<h_t, Cm_t> + Dp u_t) silu(z_t).  The sequence is cut into chunks
 *                        of ds6g_selective_scan_chunk() positions that run in parallel (state pass, carry over the chunks,
 *                        emitting pass).  saved (nullable): ds6g_selective_scan_saved_floats floats, the states at the chunk
 *                        starts (B, chunks, D, 16; chunk 0's slot, the zero state, is neither written nor read) - the only tape
 *                        the backward needs beside the operands.
 *   selective_scan_bwd   du, d delta_raw, dz (D wide each), dBm / dCm (16 wide; summed over the channels), dA_log (D, 16)
 *                        and dD (D) (summed over the tokens), all written, not accumulated.  Recomputes the states of a chunk
 *                        from its checkpoint; never divides by exp(delta A).  Deterministic (partial slabs, fixed order).
 *   ws of both scans >= ds6g_selective_scan_workspace_bytes.  The three size queries are host-only.
 *   copy_cols            dst[r][0..cols) = src[r][0..cols) between two row strides (packs the dt slice of x_proj's output
 *                        for the dt_proj GEMM and unpacks its gradient); cols % 4 == 0. */
int ds6g_selective_scan_chunk(void);
size_t ds6g_selective_scan_saved_floats(int B, int L, int D);
size_t ds6g_selective_scan_workspace_bytes(int B, int L, int D);
size_t ds6g_causal_conv1d_workspace_bytes(int B, int L, int D);
int ds6g_causal_conv1d_silu_fwd(const float* x, int ld_x, const float* w, const float* bias, float* y, int ld_y, int B,
                                int L, int D, int reverse, void* stream);
int ds6g_causal_conv1d_silu_bwd(const float* x, int ld_x, const float* w, const float* bias, const float* dy, int ld_dy,
                                float* dx, int ld_dx, float* dw, float* dbias, int B, int L, int D, int reverse, void* ws,
                                size_t ws_bytes, void* stream);
int ds6g_selective_scan_fwd(const float* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                            const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                            const float* z, int ld_z, float* y, int ld_y, float* saved, int B, int L, int D, int reverse,
                            void* ws, size_t ws_bytes, void* stream);
int ds6g_selective_scan_bwd(const float* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                            const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                            const float* z, int ld_z, const float* dy, int ld_dy, const float* saved, float* du, int ld_du,
                            float* ddelta, int ld_ddelta, float* dBm, int ld_dbm, float* dCm, int ld_dcm, float* dz,
                            int ld_dz, float* dA_log, float* dD, int B, int L, int D, int reverse, void* ws,
                            size_t ws_bytes, void* stream);
int ds6g_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, long rows, int cols, void* stream);
/* The same four operators on 16-bit storage (st16: DS6G_ST_BF16 / DS6G_ST_F16) - the same kernels instantiated on the
 * storage type, the same chunking, workspace and saved-floats queries, fp32 arithmetic, no atomics.  What is 16-bit and what
 * stays fp32 follows the layer's storage map (deepsense6g_tii_amd/mamba.py):
 *   conv   16-bit: x, y, dy, dx                      fp32: w, bias, dw, dbias
 *   scan   16-bit: u, z, y, dy, dz                   fp32: delta_raw, ddelta, Bm, Cm, dBm, dCm, du (x_proj's data gradient is
 *          added to du in fp32 afterwards), dt_bias, A_log, Dp, saved, the workspace, dA_log, dD
 * Row strides are in ELEMENTS of the operand's own type and cover whole 16-byte pieces: % 8 for a 16-bit operand, % 4 for an
 * fp32 one; every pointer 16-byte aligned.  Refusals (DS6G_ERR_ARG / DS6G_ERR_WORKSPACE) come before any launch.
 *   cast_h16_f32   dst (fp32) = src (16-bit), exact; n % 8 == 0 (the inverse of ds6g_cast_f32_h16). */
int ds6g_h16_causal_conv1d_silu_fwd(int st16, const void* x, int ld_x, const float* w, const float* bias, void* y, int ld_y,
                                    int B, int L, int D, int reverse, void* stream);
int ds6g_h16_causal_conv1d_silu_bwd(int st16, const void* x, int ld_x, const float* w, const float* bias, const void* dy,
                                    int ld_dy, void* dx, int ld_dx, float* dw, float* dbias, int B, int L, int D, int reverse,
                                    void* ws, size_t ws_bytes, void* stream);
int ds6g_h16_selective_scan_fwd(int st16, const void* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                                const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                                const void* z, int ld_z, void* y, int ld_y, float* saved, int B, int L, int D, int reverse,
                                void* ws, size_t ws_bytes, void* stream);
int ds6g_h16_selective_scan_bwd(int st16, const void* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                                const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                                const void* z, int ld_z, const void* dy, int ld_dy, const float* saved, float* du, int ld_du,
                                float* ddelta, int ld_ddelta, float* dBm, int ld_dbm, float* dCm, int ld_dcm, void* dz,
                                int ld_dz, float* dA_log, float* dD, int B, int L, int D, int reverse, void* ws,
                                size_t ws_bytes, void* stream);
int ds6g_cast_h16_f32(int st16, const void* src, float* dst, long n, void* stream);

/* ---- mamba_infer.hip : the layer's conv and scan for a frozen model - forward only, no tape, grouped ------------------
 * One launch covers ndir = 1 or 2 directions; dirs: host array of ndir descriptors (ds6g_mamba_conv_dir / ds6g_mamba_scan_dir,
 * ds6g_types.h), read during the call and handed to the kernel by value.  Every direction has operands, row strides (in
 * elements of the operand's type, whole 16-byte pieces) and a `reverse` flag of its own; B, L, D (and r) are shared.  The
 * fp32 entry points take fp32 x / y (conv) and u / z / y (scan), the ds6g_h16_ ones bf16 / f16 (st16); x_dbl, every parameter,
 * the chunk states and all arithmetic are fp32 for every storage.
 *   mamba_conv_fwd_grouped  y = silu(causal depthwise conv1d(x) + bias) per direction: per element the arithmetic of
 *                           ds6g_(h16_)causal_conv1d_silu_fwd, so the result equals ndir such calls bit for bit.  One launch.
 *   mamba_scan_fwd_grouped  the selective scan of ds6g_(h16_)selective_scan_fwd with dt_proj inside: from x_dbl (x_proj's
 *                           fp32 output, row stride ld_x >= r + 32) the kernel reads dt = columns [0, r), Bm = [r, r + 16),
 *                           Cm = [r + 16, r + 32) in place and evaluates
 *                               delta[t][d] = softplus(dt_b[d] + sum_j dt[t][j] dt_w[d][j])
 *                           as one fmaf chain over j = 0 .. r - 1 starting from 0, the bias added last, once per (token,
 *                           channel) in the staging prologue of both passes: no delta_raw tensor, no column copy.  Same lane
 *                           mapping, chunking (ds6g_selective_scan_chunk) and recurrences as the layer's scan.  Three launches
 *                           for all directions (state pass, carry, emit pass), one when L fits a single chunk.  The
 *                           chunk-start states and delta sums live in ws: ds6g_mamba_scan_fwd_grouped_workspace_size
 *                           (bytes; host only, 0 for a non-positive argument; a call on exactly that size inside poisoned
 *                           moats and the refusal of one byte less: tests/test_mamba_infer_gpu.py / _cpu.py).
 * Supported: D % 128 == 0, r % 4 == 0, 4 <= r <= 32, B, L >= 1, ndir * B <= 65535, pointers 16-byte aligned.  Anything else,
 * a null operand or a bad stride returns DS6G_ERR_ARG, an undersized workspace DS6G_ERR_WORKSPACE, before any HIP call.
 * No float atomics: two runs are bit-identical, and an ndir = 2 launch equals the two ndir = 1 launches bit for bit. */
size_t ds6g_mamba_scan_fwd_grouped_workspace_size(int B, int L, int D, int ndir);
int ds6g_mamba_conv_fwd_grouped(const ds6g_mamba_conv_dir* dirs, int ndir, int B, int L, int D, void* stream);
int ds6g_h16_mamba_conv_fwd_grouped(int st16, const ds6g_mamba_conv_dir* dirs, int ndir, int B, int L, int D, void* stream);
int ds6g_mamba_scan_fwd_grouped(const ds6g_mamba_scan_dir* dirs, int ndir, int B, int L, int D, int r, void* ws,
                                size_t ws_bytes, void* stream);
int ds6g_h16_mamba_scan_fwd_grouped(int st16, const ds6g_mamba_scan_dir* dirs, int ndir, int B, int L, int D, int r, void* ws,
                                    size_t ws_bytes, void* stream);

/* ---- mamba_fusion.hip : the bi-branch Mamba fusion stage around the Mamba layer, fp32 (mambafuser_seq.py:74-231) -------
 * Pointers 16-byte aligned, row strides (ld_*) in floats and multiples of 4; bad arguments return DS6G_ERR_ARG before
 * anything is launched.  No float atomics: every sum has a fixed order, two runs are bit-identical.
 *   sample_layernorm_fwd  ln1 = nn.LayerNorm((T, C)) (:79,94): x [B][n], n = T * C (n % 4 == 0), ONE mean / variance per
 *                         sample over its n values, gamma / beta [n]; -> y, mean [B], rstd [B].  Several workgroups per
 *                         sample: each reduces a chunk to (mean, squared deviations from that mean), the chunks are combined
 *                         in double in chunk order (Chan et al.); the variance is never formed as E[x^2] - E[x]^2.
 *   sample_layernorm_bwd  dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, means over the sample's n; dgamma [n] =
 *                         sum_b dy xhat and dbeta [n] = sum_b dy in index order, added to the destination when
 *                         accumulate_param_grads.  ws of both >= ds6g_sample_layernorm_workspace_bytes (host-only query).
 *   bimamba_gate_fwd      (:100-107) out[b, t] = bmN[b, L-1-t] * (leaky_relu_0.2(f2N[b, L-1-t]) + fm[b, t]) on [B*L][C]
 *                         operands: bmN = backward_mamba walked in reverse and f2N = fc2, both of the UNflipped fc1 output,
 *                         i.e. in natural token order; the reference never flips them back, the kernel reads them back to
 *                         front instead of copying.
 *   bimamba_gate_bwd      dfm, dbmN, df2N from dout and the three forward operands (the LeakyReLU slope from f2N: 1 for
 *                         f2N > 0, else 0.2), each written in its producer's natural order.
 *   swap_pack_fwd         (:196-214) image / lidar / radar [B*S][C][8][8] (NCHW), gps [B][2][C], pos_emb [T][C], T = 192 S + 2
 *                         -> tokens [B][T][C] = dropout(pos_emb + t): token row ((m S + s) 64 + h 8 + w) of modality m = 0, 1,
 *                         2 takes channel c from the map of modality (m + seg(c)) % 3, seg = 0 for c < C/3, 1 for
 *                         c < 2 (C/3), else 2 (integer division); the gps rows come last.  Dropout counter = seed_off + flat
 *                         element index of tokens, the rule of ds6g_dropout.  C % 64 == 0.
 *   swap_pack_bwd         the three map gradients and dgps (the masked token gradient, routed back), dpos_emb [T][C] = its
 *                         sum over b in index order; all written, not accumulated.
 *   token_unpack_fwd/bwd  (:219-231) tokens [B][T][C] <-> three NCHW maps + [B][2][C] without the channel swap.
 * The NCHW <-> token transposes are staged through LDS: 256-byte rows on both sides. */
size_t ds6g_sample_layernorm_workspace_bytes(int B, long n);
int ds6g_sample_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                              int B, long n, float eps, void* ws, size_t ws_bytes, void* stream);
int ds6g_sample_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                              float* dx, float* dgamma, float* dbeta, int B, long n, int accumulate_param_grads, void* ws,
                              size_t ws_bytes, void* stream);
int ds6g_bimamba_gate_fwd(const float* fm, int ld_fm, const float* bm, int ld_bm, const float* f2, int ld_f2, float* out,
                          int ld_out, int B, int L, int C, void* stream);
int ds6g_bimamba_gate_bwd(const float* dout, int ld_dout, const float* fm, int ld_fm, const float* bm, int ld_bm,
                          const float* f2, int ld_f2, float* dfm, int ld_dfm, float* dbm, int ld_dbm, float* df2, int ld_df2,
                          int B, int L, int C, void* stream);
int ds6g_swap_pack_fwd(const float* image, const float* lidar, const float* radar, const float* gps, const float* pos_emb,
                       float* tokens, int B, int S, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_swap_pack_bwd(const float* dtokens, float* dimage, float* dlidar, float* dradar, float* dgps, float* dpos_emb, int B,
                       int S, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_token_unpack_fwd(const float* tokens, float* image, float* lidar, float* radar, float* gps, int B, int S, int C,
                          void* stream);
int ds6g_token_unpack_bwd(const float* dimage, const float* dlidar, const float* dradar, const float* dgps, float* dtokens,
                          int B, int S, int C, void* stream);
/* The pack on the model walk's layout: the three modality maps arrive NHWC at full resolution, [B*S][H][H][C] each, as the
 * ds6g_map_desc array of the grouped glue kernels (ds6g_types.h; frames_per_sample == S and mod_off == m * S * 64 for map m,
 * anything else is DS6G_ERR_ARG).  H % 8 == 0, 8 <= H <= 64; C % 4 == 0, C <= 512; fp32; T = 192 S + 2.
 *   pool_swap_tokens_fwd  maps[m].in = map m, gemb [B][2][C], pos_emb [T][C] -> tokens [B][T][C]:
 *                             tokens[b][(m S + f) 64 + h 8 + w][c] = dropout(pos_emb + mean over the (H/8)^2 window (h, w) of
 *                             map_q[b S + f][.][.][c]),  q = (m + seg(c)) % 3 with swap_pack_fwd's seg;
 *                             tokens[b][T - 2 + j][c] = dropout(pos_emb + gemb[b][j][c]).
 *                         = avgpool_tokens_fwd3 + gps_tokens_fwd + the channel swap in ONE launch, per element the same
 *                         arithmetic; dropout counter = seed_off + flat element index of tokens (ds6g_dropout's rule, with
 *                         the device salt of ds6g_set_dropout_salt).
 *   pool_swap_tokens_bwd  from dtokens [B][T][C], the mask regenerated: maps[q].out = maps[q].in (dfeat_in, nullable, may
 *                         equal out) + the masked token gradient spread over its window / (H/8)^2, the channels of segment j
 *                         of map q taken from token modality (q - j) mod 3; dgemb [B][2][C] written; dpos_emb [T][C] = (its
 *                         old value when accumulate_dpos, +) the sum over b in index order.  Two launches.
 * No float atomics: two runs are bit-identical. */
int ds6g_pool_swap_tokens_fwd(const ds6g_map_desc* maps, const float* gemb, const float* pos_emb, float* tokens, int B, int S,
                              int H, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_pool_swap_tokens_bwd(const ds6g_map_desc* maps, const float* dtokens, float* dgemb, float* dpos_emb,
                              int accumulate_dpos, int B, int S, int H, int C, float drop_p, uint64_t seed,
                              uint64_t seed_off, void* stream);
/* The sample LayerNorm, the gate and the pool-swap pack on 16-bit storage (st16: DS6G_ST_BF16 / DS6G_ST_F16) - the same
 * kernels instantiated on the storage type, the same chunking, fixed-order partials and workspace query, fp32 arithmetic with
 * ONE rounding per stored element, no atomics.  What is 16-bit follows the stage's storage map
 * (deepsense6g_tii_amd/mamba_fusion.py):
 *   sample_layernorm   16-bit: x, y, dy, dx                 fp32: gamma, beta, dgamma, dbeta, mean, rstd (statistics of the
 *                      widened values), the double partials of the workspace
 *   bimamba_gate       16-bit: all seven streams (fm, bm, f2, out; dout, dfm, dbm, df2); the LeakyReLU slope from the stored f2
 *   pool_swap_tokens   16-bit: the maps (in and out), tokens, dtokens       fp32: gemb, pos_emb, dgemb, dpos_emb
 * A thread moves 16 bytes = 8 elements of a 16-bit operand: n % 8 == 0, C % 8 == 0, row strides (in ELEMENTS of the operand's
 * own type) % 8 for a 16-bit operand; every pointer 16-byte aligned.  Refusals (DS6G_ERR_ARG / DS6G_ERR_WORKSPACE) come before
 * any launch. */
int ds6g_h16_sample_layernorm_fwd(int st16, const void* x, const float* gamma, const float* beta, void* y, float* mean,
                                  float* rstd, int B, long n, float eps, void* ws, size_t ws_bytes, void* stream);
int ds6g_h16_sample_layernorm_bwd(int st16, const void* dy, const void* x, const float* mean, const float* rstd,
                                  const float* gamma, void* dx, float* dgamma, float* dbeta, int B, long n,
                                  int accumulate_param_grads, void* ws, size_t ws_bytes, void* stream);
int ds6g_h16_bimamba_gate_fwd(int st16, const void* fm, int ld_fm, const void* bm, int ld_bm, const void* f2, int ld_f2,
                              void* out, int ld_out, int B, int L, int C, void* stream);
int ds6g_h16_bimamba_gate_bwd(int st16, const void* dout, int ld_dout, const void* fm, int ld_fm, const void* bm, int ld_bm,
                              const void* f2, int ld_f2, void* dfm, int ld_dfm, void* dbm, int ld_dbm, void* df2, int ld_df2,
                              int B, int L, int C, void* stream);
int ds6g_h16_pool_swap_tokens_fwd(int st16, const ds6g_map_desc* maps, const float* gemb, const float* pos_emb, void* tokens,
                                  int B, int S, int H, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_h16_pool_swap_tokens_bwd(int st16, const ds6g_map_desc* maps, const void* dtokens, float* dgemb, float* dpos_emb,
                                  int accumulate_dpos, int B, int S, int H, int C, float drop_p, uint64_t seed,
                                  uint64_t seed_off, void* stream);

/* ---- time_mamba.hip : the temporal Mamba fusion head behind its shared Mamba layer, fp32 (mambafuser_seq.py:233-284) --
 * A sample has 17 rows of C = 512 floats: 3 modalities x S = 5 frames of the layer's output y, then its 2 gps rows.  y is
 * the layer's output on the modality-major batch [3 * B * 5][512], row (m * B + b) * 5 + t (m = image, lidar, radar); the gps
 * rows are addressed as gps + b * ld_gps_sample + j * 512, so they may be the last two token rows of a [B][T][512] stage
 * output (ld_gps_sample = T * 512) as well as a [B][2][512] tensor (1024).  All pointers 16-byte aligned, B >= 1, S == 5,
 * C == 512, the sample strides >= 1024 floats and multiples of 4; anything else returns DS6G_ERR_ARG before anything is
 * launched.  One launch each, one workgroup per sample.  No float atomics: every sum has a fixed order, two runs are
 * bit-identical.
 *   time_attn_fwd  (:265-282) score[b][r] = max_c row[c] + (1 / 512) sum_c row[c]  (MaxPool1d(512) + AvgPool1d(512));
 *                  attn[b][5 m .. 5 m + 5) = softmax(w5 score[b][5 m ..] + b5) per modality (mlp: one Linear(5, 5) for the
 *                  three), attn[b][15 .. 17) = softmax(w2 score[b][15 ..] + b2) (mlp_gps);  out[b][c] = sum_r attn[b][r]
 *                  row_r[c].  Also written for the backward: attn, score [B][17] and argmax [B][17] (int32: the channel of
 *                  each row's maximum, the LOWEST one of a tie - torch's CPU max-pool rule).
 *   time_attn_bwd  from dout [B][512] and the saved tensors: dy [3 * B * 5][512] (y's layout) and dgps (at dgps + b *
 *                  ld_dgps_sample + j * 512), both written, not accumulated:
 *                      d row_r[c] = attn[r] dout[c] + ds[r] / 512 + (c == argmax[r] ? ds[r] : 0),
 *                      ds = W^T (attn (.) (da - sum attn da)) per softmax group,  da[r] = sum_c dout[c] row_r[c];
 *                  dparam_part [B][36]: sample b's share of dw5 (25, row-major), db5 (5), dw2 (4), db2 (2) - sum it over
 *                  b with ds6g_batch_sum(dparam_part, dst, 36, B, 36, accumulate). */
int ds6g_time_attn_fwd(const float* y, const float* gps, long ld_gps_sample, const float* w5, const float* b5,
                       const float* w2, const float* b2, float* out, float* attn, float* score, int* argmax, int B, int S,
                       int C, void* stream);
int ds6g_time_attn_bwd(const float* dout, const float* y, const float* gps, long ld_gps_sample, const float* attn,
                       const float* score, const int* argmax, const float* w5, const float* w2, float* dy, float* dgps,
                       long ld_dgps_sample, float* dparam_part, int B, int S, int C, void* stream);
/* temporal_param_grads (behind time_attn_bwd): dparam_part [B][36] summed over b in index order with ds6g_batch_sum's arithmetic and delivered to the
 * four parameters' own gradients dw5 [25], db5 [5], dw2 [4], db2 [2] (4-byte aligned, e.g. slices of a gradient arena), each
 * written, or added to where its acc_* flag is set.  One launch; a null pointer or B < 1 is DS6G_ERR_ARG. */
int ds6g_temporal_param_grads(const float* dparam_part, int B, float* dw5, int acc_w5, float* db5, int acc_b5, float* dw2,
                          int acc_w2, float* db2, int acc_b2, void* stream);
/* The grouped head pool between the three fp32 NHWC maps [N][8][8][C] of the last stage (three independent base pointers) and
 * the head's modality-major rows [3 N][C]; one launch each way in place of three ds6g_global_pool / ds6g_head_bwd launches.
 * N >= 1, C % 4 == 0, N * 64 * C <= 2^31, all pointers 16-byte aligned; anything else is DS6G_ERR_ARG before anything is
 * launched.  Memory-bound: 16-byte loads and stores, no atomics, fixed summation order (two runs are bit-identical).
 *   pool_rows3_fwd  rows[m N + n][c] = (1 / 64) sum over the 64 positions p (in index order) of feat_m[n][p][c].
 *   pool_rows3_bwd  dfeat_m[n][p][c] = (dfeat_in_m[n][p][c], or 0 where dfeat_in_m is null) + drows[m N + n][c] / 64; every
 *                   element is written exactly once; dfeat_in_m may be dfeat_m itself. */
int ds6g_pool_rows3_fwd(const float* feat0, const float* feat1, const float* feat2, float* rows, int N, int C, void* stream);
int ds6g_pool_rows3_bwd(const float* drows, const float* dfeat_in0, const float* dfeat_in1, const float* dfeat_in2,
                        float* dfeat0, float* dfeat1, float* dfeat2, int N, int C, void* stream);
/* The head pool on 16-bit storage (st16: DS6G_ST_BF16 / DS6G_ST_F16): the same two kernels instantiated on the storage type of
 * the MAPS of a model walk, the same single launch each way.  Storage map:
 *   16-bit: feat_m; dfeat_in_m and dfeat_m          fp32: rows, drows (the temporal head's input and its gradient, which stay
 *                                                   fp32 whatever the walk's storage), every sum and product
 * A thread moves 16 bytes = 8 map elements: C % 8 == 0, C >= 8; N >= 1, N * 64 * C <= 2^31, all pointers 16-byte aligned;
 * anything else (st16 == 0 included) is DS6G_ERR_ARG before anything is launched.
 *   fwd  the 64 positions are widened and summed in fp32 in position order, as on fp32 storage; rows is not rounded.
 *   bwd  float(dfeat_in_m or 0) + drows / 64 in fp32, rounded ONCE (to nearest even) at the store; dfeat_in_m may be null or
 *        dfeat_m itself.  No atomics, fixed order: two runs are bit-identical. */
int ds6g_h16_pool_rows3_fwd(int st16, const void* feat0, const void* feat1, const void* feat2, float* rows, int N, int C,
                            void* stream);
int ds6g_h16_pool_rows3_bwd(int st16, const float* drows, const void* dfeat_in0, const void* dfeat_in1, const void* dfeat_in2,
                            void* dfeat0, void* dfeat1, void* dfeat2, int N, int C, void* stream);

/* ---- spatial.hip-------------------------------------------------------------------------------*/
/* normalize_imagenet + stack + NCHW->NHWC: model2_seq.py:36-45,481-482,491-493 */
int ds6g_pack_input(const float* src, float* dst, int B, int Cs, int H, int W, int Cd, int frames_per_sample, int t,
                    int normalize_imagenet, void* stream);
int ds6g_pack_input_h16(int st16, const float* src, void* dst, int B, int Cs, int H, int W, int frames_per_sample, int t,
                        int normalize_imagenet, void* stream);
int ds6g_pad_channels(const float* src, float* dst, long rows, int cin, int cout, int unpad, int accumulate,
                      void* stream);
/* MaxPool2d(3,2,1) of the stems: model2_seq.py:498,503,508 */
int ds6g_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int ds6g_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int N, int H, int W, int C, void* stream);
/* the ResNet stem's BN -> ReLU -> MaxPool(3, 2, 1) (torchvision resnet.py forward, used at model2_seq.py:495-500) without
 * materialising the activation: forward = ds6g_bn_apply(relu) + ds6g_maxpool3x3s2_fwd in one pass (bit-identical);
 * backward = ds6g_maxpool3x3s2_bwd + ds6g_bn_bwd(relu_beta) with the pool gradient gathered from (dpool, idx) inside the
 * BN kernels.  x: the conv output [N][H][W][C]; mean / invstd from ds6g_bn_stats or ds6g_bn_eval_prepare. */
int ds6g_bn_relu_maxpool3x3s2_fwd(const float* x, const float* mean, const float* invstd, const float* gamma,
                                  const float* beta, float* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int ds6g_bn_bwd_maxpool(const float* dpool, const uint8_t* idx, const float* x, const float* mean, const float* invstd,
                        const float* gamma, const float* relu_beta, float* dx, float* dgamma, float* dbeta, int N, int H,
                        int W, int C, int accumulate_param_grads, void* ws, size_t ws_bytes, void* stream);
/* bf16-storage path: the 4-channel stem keeps the fp32-storage conv kernels (x, dx fp32); its pooled output is written as
 * bf16 (first tensor of the bf16 trunk) and the gradient of the pooled tensor arrives as bf16 */
int ds6g_bn_relu_maxpool3x3s2_fwd_h16out(int st16, const float* x, const float* mean, const float* invstd, const float* gamma,
                                         const float* beta, void* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int ds6g_bn_bwd_maxpool_h16in(int st16, const void* dpool, const uint8_t* idx, const float* x, const float* mean,
                              const float* invstd, const float* gamma, const float* relu_beta, float* dx, float* dgamma,
                              float* dbeta, int N, int H, int W, int C, int accumulate_param_grads, void* ws, size_t ws_bytes,
                              void* stream);
/* bf16-storage path of the pooling / resampling / head kernels below: feature maps (feat, out, dfeat, dout) bf16, tokens /
 * pos_emb / pooled vectors fp32 */
int ds6g_h16_avgpool_tokens_fwd(int st16, const void* feat, const float* pos_emb, float* tokens, int N, int H, int C,
                                int frames_per_sample, int mod_off, int T, float drop_p, uint64_t seed, uint64_t seed_off,
                                void* stream);
int ds6g_h16_avgpool_tokens_bwd(int st16, const float* dtok, const void* dfeat_in, void* dfeat, int N, int H, int C,
                                int frames_per_sample, int mod_off, int T, void* stream);
int ds6g_h16_upsample_add_fwd(int st16, const void* feat, const float* tokens, void* out, int N, int H, int C,
                              int frames_per_sample, int mod_off, int T, void* stream);
int ds6g_h16_upsample_add_bwd(int st16, const void* dout, float* dtok, int N, int H, int C, int frames_per_sample, int mod_off,
                              int T, void* stream);
int ds6g_h16_global_pool(int st16, const void* feat, float* pooled, int N, int C, void* stream);
int ds6g_h16_head_bwd(int st16, const float* dfused, void* dfeat, int N, int C, int frames_per_sample, void* stream);
/* AdaptiveAvgPool2d((8,8)) + token pack + pos_emb + embd dropout: model2_seq.py:414,515-517,261-272 */
int ds6g_avgpool_tokens_fwd(const float* feat, const float* pos_emb, float* tokens, int N, int H, int C,
                            int frames_per_sample, int mod_off, int T, float drop_p, uint64_t seed,
                            uint64_t seed_off, void* stream);
int ds6g_gps_tokens_fwd(const float* emb, const float* pos_emb, float* tokens, int B, int C, int T, float drop_p,
                        uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_dropout(const float* src, float* dst, long n, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_avgpool_tokens_bwd(const float* dtok, const float* dfeat_in, float* dfeat, int N, int H, int C,
                            int frames_per_sample, int mod_off, int T, void* stream);
/* token unpack + F.interpolate(bilinear, align_corners=False) + residual: model2_seq.py:275-287,521-526,
 * 539-544,558-563,577-579 */
int ds6g_upsample_add_fwd(const float* feat, const float* tokens, float* out, int N, int H, int C,
                          int frames_per_sample, int mod_off, int T, void* stream);
int ds6g_upsample_add_bwd(const float* dout, float* dtok, int N, int H, int C, int frames_per_sample, int mod_off,
                          int T, void* stream);
/* The four kernels above for the THREE modality maps of a fusion stage in one launch each (per element the same
 * arithmetic and dropout counters as three single-map calls).  st: 0 = fp32 maps, DS6G_ST_BF16 / DS6G_ST_F16 = 16-bit maps;
 * maps: host array of 3 descriptors, read during the call; map m has B * frames_per_sample frames of H x H x C and its
 * tokens start at row mod_off of each sample's T.  in / out: feat / - (avgpool_fwd3), dfeat_in (nullable) / dfeat
 * (avgpool_bwd3), feat / out (upsample_add_fwd3), dout / - (upsample_add_bwd3). */
/* ds6g_map_desc {in, out, frames_per_sample, mod_off}: ds6g_types.h */
int ds6g_avgpool_tokens_fwd3(int st, const ds6g_map_desc* maps, const float* pos_emb, float* tokens, int B, int H, int C,
                             int T, float drop_p, uint64_t seed, uint64_t seed_off, void* stream);
int ds6g_avgpool_tokens_bwd3(int st, const ds6g_map_desc* maps, const float* dtok, int B, int H, int C, int T, void* stream);
int ds6g_upsample_add_fwd3(int st, const ds6g_map_desc* maps, const float* tokens, int B, int H, int C, int T, void* stream);
int ds6g_upsample_add_bwd3(int st, const ds6g_map_desc* maps, float* dtok, int B, int H, int C, int T, void* stream);
/* features.avgpool + flatten + cat + sum(dim=1): model2_seq.py:581-595 */
int ds6g_global_pool(const float* feat, float* pooled, int N, int C, void* stream);
int ds6g_head_sum(const float* pooled_img, const float* pooled_lidar, const float* pooled_radar, const float* tokens,
                  float* fused, int B, int C, int fps_img, int fps_other, int T, void* stream);
int ds6g_head_bwd(const float* dfused, float* dfeat, int N, int C, int frames_per_sample, void* stream);
int ds6g_feat_to_tokens(const float* dfeat, float* dtok, int N, int C, int frames_per_sample, int mod_off, int T,
                        void* stream);
int ds6g_gps_rows(const float* src, float* dst, int B, int C, int T, int to_tokens, int accumulate, int src_bcast,
                  void* stream);
int ds6g_axpby(const float* a, const float* b, float* out, long n, float alpha, float beta, void* stream);
int ds6g_batch_sum(const float* src, float* out, long n, int count, long stride, int accumulate, void* stream);

/* ---- step.hip ----------------------------------------------------------------------------------*/
/* FocalLoss -> torchvision.ops.sigmoid_focal_loss(alpha .25, gamma 2, mean): train2_seq.py:291-301 */
int ds6g_focal_loss(const float* logits, const float* target, float* loss, float* dlogits, int n, float alpha,
                    float gamma, float upstream, void* stream);
/* optim.AdamW step (train2_seq.py:131,539) fused with EMA.update (train2_seq.py:315-320) */
/* grad_scale_dev (nullable): one device float multiplied into grad_scale at run time - the clip coefficient below. */
int ds6g_adamw_step(float* p, const float* g, float* m, float* v, float* shadow, long n, int step, float lr,
                    float beta1, float beta2, float eps, float wd, float ema_decay, float grad_scale,
                    const float* grad_scale_dev, void* stream);
/* the same step with its per-step scalars in DEVICE memory, so that a hipGraph capture of the whole training step can be
 * replayed: state = 16 bytes {float lr, float bc1, float bc2_sqrt, int step}, zero-initialised; the host writes lr when the
 * schedule changes it; ds6g_adamw_state_advance (one thread) increments step and recomputes the bias corrections. */
int ds6g_adamw_state_advance(void* state, float beta1, float beta2, void* stream);
int ds6g_adamw_step_dev(float* p, const float* g, float* m, float* v, float* shadow, long n, const void* state, float beta1,
                        float beta2, float eps, float wd, float ema_decay, float grad_scale, const float* grad_scale_dev,
                        void* stream);
/* torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) of the 30->5 training step (train2_seq_30to5.py:120) on
 * the flat gradient arena: out[0] = pre_scale * ||g||_2, out[1] = min(1, max_norm / (out[0] + 1e-6)); the gradients are
 * not rewritten - pass out + 1 to ds6g_adamw_step as grad_scale_dev.  One launch (last-block-done reduction in index
 * order: deterministic).  ws: >= 8 KiB + 8 bytes, its first 4 bytes zero on first use. */
int ds6g_grad_norm_clip(const float* g, long n, float max_norm, float pre_scale, float* out, void* ws, size_t ws_bytes,
                        void* stream);
/* Dynamic loss scaling (train.DynamicLossScaler; torch.amp.GradScaler semantics, all of it on the device: no host sync, graph-
 * replayable).  scaler_state: ds6g_loss_scaler_state_bytes() of device memory {float scale, int clean_steps, int found_inf,
 * float adamw_coef, float unscaled_norm, 3 x pad} - the host writes the initial scale and zeros.  Per step:
 *   ds6g_focal_loss_scaled    the focal loss with dlogits multiplied by the scale (the reported loss stays unscaled);
 *   ds6g_loss_scale_check     one deterministic reduction over the (scaled, rank-summed) gradient arena: found_inf when any
 *                             element is non-finite, the unscaled norm (* pre_scale) and the AdamW coefficient
 *                             1/scale * min(1, max_norm / (norm + 1e-6)) (no clip when max_norm <= 0);
 *   ds6g_loss_scale_update    one thread: found_inf -> scale *= backoff, clean_steps = 0, the AdamW state is NOT advanced;
 *                             else the AdamW state advances (ds6g_adamw_state_advance) and every growth_interval clean steps
 *                             scale *= growth;
 *   ds6g_adamw_step_scaled    ds6g_adamw_step_dev with the coefficient / skip flag of scaler_state: a skipped step leaves
 *                             p, m, v untouched and still updates the EMA shadow from the unchanged p.
 * ws of the check: >= ds6g_loss_scale_check_workspace_bytes(n), first 4 bytes zero on first use (left zero). */
size_t ds6g_loss_scaler_state_bytes(void);
size_t ds6g_loss_scale_check_workspace_bytes(long n);
int ds6g_focal_loss_scaled(const float* logits, const float* target, float* loss, float* dlogits, int n, float alpha,
                           float gamma, const void* scaler_state, void* stream);
int ds6g_loss_scale_check(const float* g, long n, float max_norm, float pre_scale, void* scaler_state, void* ws,
                          size_t ws_bytes, void* stream);
int ds6g_loss_scale_update(void* scaler_state, void* adam_state, float beta1, float beta2, float backoff, float growth,
                           int growth_interval, void* stream);
int ds6g_adamw_step_scaled(float* p, const float* g, float* m, float* v, float* shadow, long n, const void* state,
                           const void* scaler_state, float beta1, float beta2, float eps, float wd, float ema_decay,
                           float grad_scale, void* stream);
/* dst (bf16, RNE) = src (fp32): refreshes the bf16 shadow of the parameter arena for the bf16-storage path */
int ds6g_cast_f32_h16(int st16, const float* src, void* dst, long n, void* stream);
/* vel_emb1..4 and the join MLP: model2_seq.py:422-425,518,536,555,574,863-869 */
int ds6g_small_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, int K,
                          int rows_per_group, long group_stride, int relu, void* stream);
int ds6g_small_linear_bwd(const float* dy, const float* y_mask, const float* x, const float* w, float* dx, float* dw,
                          float* db, int M, int N, int K, int rows_per_group, long group_stride,
                          int dx_rows_per_group, long dx_group_stride, int accumulate_dx, int accumulate_params,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DS6G_H */
