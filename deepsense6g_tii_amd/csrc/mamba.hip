// The Mamba layer's two non-GEMM operators (mamba_ssm.Mamba, slow-path semantics; reference call sites
// mambafuser_seq.py:83-101, 240, 261-263), fp32, d_state = 16, d_conv = 4:
//   causal depthwise conv1d (4 taps) + bias + SiLU, forward and backward, in either sequence direction;
//   the selective scan   delta = softplus(raw + dt_bias);  h_t = exp(delta_t A) h_{t-1} + delta_t u_t B_t;
//                        y_t = (<h_t, C_t> + D u_t) silu(z_t)
//   forward and backward, in either direction.
// Data is token-major: row = b * L + t, channels contiguous; every operand is pointer + row stride (floats), so the column
// halves of in_proj's output and the column slices of x_proj's output are read in place.
// Every kernel is a template on the storage type T of the WIDE activations (x, y, dy, dx of the conv; u, z, y, dy, dz of the
// scan): float behind the fp32 entry points, __bf16 / _Float16 behind the ds6g_h16_* ones (row strides then in elements of T).
// Parameters, delta_raw, Bm / Cm, their gradients, du, the scan state, checkpoints, slabs and all arithmetic are fp32 for every
// T.  A 16-bit workgroup keeps the fp32 mapping - 16 channels, now 32-byte row pieces moved as two 16-byte loads and widened on
// the way into LDS - because the scan is instruction-issue-bound, not byte-bound (DESIGN.md 3.9a has the decision).
//
// Scan mapping: lane = (channel, state).  The 16 states of a channel are one DPP row, so <h, C>, d delta and du are row
// reductions without LDS; a workgroup is 16 channels x 16 states and walks ONE chunk of SCAN_CHUNK positions whose operands
// it stages in LDS first (coalesced 64-byte row pieces; softplus / sigmoid are evaluated once per (token, channel) there,
// not once per lane).  The sequence is chunked so that B * chunks * D / 16 workgroups exist where B * D / 16 would leave
// the GPU idle (d_model = 64, B = 12: 96):
//   forward   state pass   each chunk from h = 0 -> its end state and its sum of delta
//             carry        h_in[c + 1] = exp(A * sum_delta_c) h_in[c] + h_end[c]          (in place; the checkpoints)
//             emit pass    each chunk from its true h_in -> y
//   backward  local pass   each chunk's reverse recurrence from a zero incoming gradient
//             carry        G[c] = exp(A * sum_delta_c) G[c + 1] + local[c]
//             main pass    recomputes h_t of the chunk from the checkpoint into REGISTERS (one per position), then walks the
//                          chunk backwards.  The recurrence is never inverted: no division by exp(delta A), which is 0 for a
//                          large step.
// Sums over channels (dB, dC) and over tokens (dA_log, dD, the conv's dweight / dbias) go through partial slabs and a
// fixed-order reduction: no float atomics, two runs are bit-identical.
#include "mamba_dev.h"   // the mapping constants, staging helpers, forward recurrences, conv lane body and argument rules

namespace {

// T: the storage type of the wide activations u, z, y, dy, dz - float, or __bf16 / _Float16 on the 16-bit-storage path
// (ds6g_h16_selective_scan_*).  Everything else, and everything held in LDS or registers, is fp32 for every T.
template <typename T>
struct ScanP {
    const T *u, *z, *dy;
    const float *raw, *dt_bias, *A_log, *Bm, *Cm, *Dp;
    int ld_u, ld_raw, ld_b, ld_c, ld_z, ld_dy;
    T *y; int ld_y;
    float *hin;      // [B][nc][D][16] states at chunk starts (slot 0 is never touched: it is zero)
    float *sumd;     // [B][nc][D]
    float *gl;       // [B][nc][D][16] gradient w.r.t. the state at chunk starts
    float *du, *draw; T *dz; int ld_du, ld_draw, ld_dz;
    float *slab_bc;  // [D / 16][B * L][32]
    float *slab_a;   // [B * nc][D][16]
    float *slab_d;   // [B * nc][D]
    int B, L, D, nc, rev;
};

#define SCAN_IDS()                                                                         \
    const int g = blockIdx.x, c = blockIdx.y, b = blockIdx.z;                              \
    const int tid = threadIdx.x, dl = tid >> 4, n = tid & 15;                              \
    const int d0 = g * CPB, d = d0 + dl;                                                   \
    const int s0 = c * SCAN_CHUNK;                                                         \
    const int len = min(SCAN_CHUNK, p.L - s0);                                             \
    const size_t rowbase = (size_t)b * p.L;                                                \
    const float A2 = -expf(p.A_log[d * NS + n]) * LOG2E;   /* exp(delta A) = exp2(delta A2) */ \
    const size_t chunk_id = (size_t)b * p.nc + c

// forward state pass: chunk c (< nc - 1) from h = 0 -> hin slot c + 1 (its end state), sumd[c]
template <typename T>
__global__ __launch_bounds__(256) void scan_state_kernel(const ScanP<T> p) {
    __shared__ float s_dl[TILE], s_u[TILE], s_B[TILE];
    SCAN_IDS();
    stage16(s_dl, p.raw, p.ld_raw, rowbase, p.L, s0, len, p.rev, d0, 0);
    stage16(s_u, p.u, p.ld_u, rowbase, p.L, s0, len, p.rev, d0, 1);
    __syncthreads();
    stage16(s_B, p.Bm, p.ld_b, rowbase, p.L, s0, len, p.rev, 0, 0);
    for (int i = tid; i < TILE; i += 256) {
        const float dt = softplus_(s_dl[i] + p.dt_bias[d0 + (i & 15)]);
        s_dl[i] = dt;
        s_u[i] *= dt;
    }
    __syncthreads();
    float h, sd;
    scan_state_walk(s_dl, s_u, s_B, len, dl, n, A2, h, sd);
    p.hin[((chunk_id + 1) * p.D + d) * NS + n] = h;
    if (n == 0) p.sumd[chunk_id * p.D + d] = sd;
}

// hin[c + 1] = exp(A sum_delta_c) hin[c] + hin[c + 1] for c = 0 .. nc - 2 (hin[0] = 0, never stored); one thread per
// (b, channel, state)
template <typename T>
__global__ __launch_bounds__(256) void scan_carry_kernel(const ScanP<T> p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)p.D * NS;
    if (i >= (size_t)p.B * per) return;
    const int b = (int)(i / per);
    const int dn = (int)(i % per);
    scan_carry_walk(p.hin, p.sumd, p.A_log, (size_t)b * p.nc, p.nc, p.D, per, dn);
}

// forward emit pass
template <typename T>
__global__ __launch_bounds__(256) void scan_emit_kernel(const ScanP<T> p) {
    __shared__ float s_dl[TILE], s_u[TILE], s_z[TILE], s_B[TILE], s_C[TILE];
    SCAN_IDS();
    stage16(s_dl, p.raw, p.ld_raw, rowbase, p.L, s0, len, p.rev, d0, 0);
    stage16(s_u, p.u, p.ld_u, rowbase, p.L, s0, len, p.rev, d0, 1);
    __syncthreads();
    stage16(s_z, p.z, p.ld_z, rowbase, p.L, s0, len, p.rev, d0, 0);
    stage16(s_B, p.Bm, p.ld_b, rowbase, p.L, s0, len, p.rev, 0, 1);
    for (int i = tid; i < TILE; i += 256) s_dl[i] = softplus_(s_dl[i] + p.dt_bias[d0 + (i & 15)]);
    __syncthreads();
    stage16(s_C, p.Cm, p.ld_c, rowbase, p.L, s0, len, p.rev, 0, 0);
    for (int i = tid; i < TILE; i += 256) { const float zz = s_z[i]; s_z[i] = zz * sigmoid_(zz); }
    __syncthreads();
    const float h = c > 0 ? p.hin[(chunk_id * p.D + d) * NS + n] : 0.f;
    scan_emit_walk(s_dl, s_u, s_z, s_B, s_C, len, dl, n, A2, p.Dp[d], h);
    __syncthreads();
    unstage16(s_z, p.y, p.ld_y, rowbase, p.L, s0, len, p.rev, d0, 0);
}

// backward local pass: chunk c (>= 1) from a zero incoming gradient -> gl slot c (gradient w.r.t. the state the chunk
// starts from), sumd[c]
template <typename T>
__global__ __launch_bounds__(256) void scan_bwd_local_kernel(const ScanP<T> p) {
    __shared__ float s_dl[TILE], s_z[TILE], s_dy[TILE], s_C[TILE];
    SCAN_IDS();
    stage16(s_dl, p.raw, p.ld_raw, rowbase, p.L, s0, len, p.rev, d0, 0);
    stage16(s_z, p.z, p.ld_z, rowbase, p.L, s0, len, p.rev, d0, 1);
    __syncthreads();
    stage16(s_dy, p.dy, p.ld_dy, rowbase, p.L, s0, len, p.rev, d0, 0);
    stage16(s_C, p.Cm, p.ld_c, rowbase, p.L, s0, len, p.rev, 0, 1);
    for (int i = tid; i < TILE; i += 256) s_dl[i] = softplus_(s_dl[i] + p.dt_bias[d0 + (i & 15)]);
    __syncthreads();
    for (int i = tid; i < TILE; i += 256) { const float zz = s_z[i]; s_dy[i] *= zz * sigmoid_(zz); }
    __syncthreads();
    float gb = 0.f, sd = 0.f;
    for (int s = len - 1; s >= 0; --s) {
        const float dt = s_dl[s * 16 + dl];
        const float gg = fmaf(s_dy[s * 16 + dl], s_C[s * 16 + n], gb);
        gb = exp2f(dt * A2) * gg;
        sd += dt;
    }
    p.gl[(chunk_id * p.D + d) * NS + n] = gb;
    if (n == 0) p.sumd[chunk_id * p.D + d] = sd;
}

// G[c] = exp(A sum_delta_c) G[c + 1] + local[c] for c = nc - 1 .. 1 (G[nc] = 0), in place
template <typename T>
__global__ __launch_bounds__(256) void scan_bwd_carry_kernel(const ScanP<T> p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)p.D * NS;
    if (i >= (size_t)p.B * per) return;
    const int b = (int)(i / per);
    const int dn = (int)(i % per);
    const float A2 = -expf(p.A_log[dn]) * LOG2E;
    float gcar = 0.f;
    for (int c = p.nc - 1; c >= 1; --c) {
        const size_t cid = (size_t)b * p.nc + c;
        float* slot = p.gl + cid * per + dn;
        gcar = fmaf(exp2f(p.sumd[cid * p.D + (dn >> 4)] * A2), gcar, *slot);
        *slot = gcar;
    }
}

// backward main pass
template <typename T>
__global__ __launch_bounds__(256) void scan_bwd_main_kernel(const ScanP<T> p) {
    __shared__ float s_dl[TILE], s_u[TILE], s_sg[TILE], s_dyv[TILE], s_dzf[TILE], s_B[TILE], s_C[TILE];
    __shared__ float s_red[4][SCAN_CHUNK][32];
    SCAN_IDS();
    stage16(s_dl, p.raw, p.ld_raw, rowbase, p.L, s0, len, p.rev, d0, 0);
    stage16(s_u, p.u, p.ld_u, rowbase, p.L, s0, len, p.rev, d0, 1);
    __syncthreads();
    stage16(s_dzf, p.z, p.ld_z, rowbase, p.L, s0, len, p.rev, d0, 0);
    stage16(s_dyv, p.dy, p.ld_dy, rowbase, p.L, s0, len, p.rev, d0, 1);
    __syncthreads();
    stage16(s_B, p.Bm, p.ld_b, rowbase, p.L, s0, len, p.rev, 0, 0);
    stage16(s_C, p.Cm, p.ld_c, rowbase, p.L, s0, len, p.rev, 0, 1);
    for (int i = tid; i < TILE; i += 256) {
        const float v = s_dl[i] + p.dt_bias[d0 + (i & 15)];
        s_dl[i] = softplus_(v);
        s_sg[i] = v > 20.f ? 1.f : sigmoid_(v);          // d softplus / d v
        const float zz = s_dzf[i], sz = sigmoid_(zz), dout = s_dyv[i];
        s_dyv[i] = dout * zz * sz;                        // gradient of (<h, C> + D u)
        s_dzf[i] = dout * sz * fmaf(zz, 1.f - sz, 1.f);   // dz = this * (<h, C> + D u)
    }
    __syncthreads();
    const float hin = c > 0 ? p.hin[(chunk_id * p.D + d) * NS + n] : 0.f;
    const float Dd = p.Dp[d];
    float hist[SCAN_CHUNK];
    {
        float h = hin;
#pragma unroll
        for (int s = 0; s < SCAN_CHUNK; ++s) {
            if (s < len) {
                const float dt = s_dl[s * 16 + dl], uu = s_u[s * 16 + dl];
                h = fmaf(exp2f(dt * A2), h, dt * uu * s_B[s * 16 + n]);
                const float yv = row16_sum(h * s_C[s * 16 + n]);
                if (n == 0) s_dzf[s * 16 + dl] *= fmaf(Dd, uu, yv);
            }
            hist[s] = h;
        }
    }
    float gb = c + 1 < p.nc ? p.gl[((chunk_id + 1) * p.D + d) * NS + n] : 0.f;
    float accA = 0.f, accD = 0.f;
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int s = SCAN_CHUNK - 1; s >= 0; --s) {
        if (s < len) {
            const float dt = s_dl[s * 16 + dl], uu = s_u[s * 16 + dl], dyv = s_dyv[s * 16 + dl];
            const float hs = hist[s];
            const float hprev = s > 0 ? hist[s > 0 ? s - 1 : 0] : hin;
            const float Bv = s_B[s * 16 + n];
            const float gg = fmaf(dyv, s_C[s * 16 + n], gb);
            const float a = exp2f(dt * A2);
            const float da = gg * hprev * a;              // d a_t * a_t
            gb = a * gg;
            accA = fmaf(da, dt, accA);
            const float dxu = row16_sum(gg * Bv);        // gradient of delta_t u_t
            const float dda = row16_sum(da * A2);        // * ln 2 below: d delta through exp(delta A)
            float pb = gg * dt * uu, pc = dyv * hs;      // dB, dC contributions of this channel
            pb += __shfl_xor(pb, 16, 64); pc += __shfl_xor(pc, 16, 64);
            pb += __shfl_xor(pb, 32, 64); pc += __shfl_xor(pc, 32, 64);
            if (lane < 16) { s_red[wave][s][lane] = pb; s_red[wave][s][16 + lane] = pc; }
            if (n == 0) {
                accD = fmaf(dyv, uu, accD);
                const float ddt = fmaf(uu, dxu, dda * (1.f / LOG2E));
                s_u[s * 16 + dl] = fmaf(dyv, Dd, dt * dxu);
                s_sg[s * 16 + dl] *= ddt;
            }
        }
    }
    // dA_log = A * sum_t (d a_t a_t delta_t);  A = A2 / log2(e)
    p.slab_a[(chunk_id * p.D + d) * NS + n] = accA * A2 * (1.f / LOG2E);
    if (n == 0) p.slab_d[chunk_id * p.D + d] = accD;
    __syncthreads();
    unstage16(s_u, p.du, p.ld_du, rowbase, p.L, s0, len, p.rev, d0, 0);
    unstage16(s_sg, p.draw, p.ld_draw, rowbase, p.L, s0, len, p.rev, d0, 1);
    __syncthreads();
    unstage16(s_dzf, p.dz, p.ld_dz, rowbase, p.L, s0, len, p.rev, d0, 0);
    {
        const int s = tid >> 3, q = tid & 7;
        if (s < len) {
            f32x4 acc = ld4(&s_red[0][s][q * 4]);
            for (int w = 1; w < 4; ++w) acc += ld4(&s_red[w][s][q * 4]);
            const int t = p.rev ? p.L - 1 - (s0 + s) : s0 + s;
            st4(p.slab_bc + (((size_t)g * p.B * p.L) + rowbase + t) * 32 + q * 4, acc);
        }
    }
}

// dBm / dCm [row][16] = sum over the D / 16 channel groups of slab_bc, in group order
__global__ __launch_bounds__(256) void scan_bc_reduce_kernel(const float* __restrict__ slab, int groups, size_t rows,
                                                             float* __restrict__ dBm, int ld_dbm, float* __restrict__ dCm,
                                                             int ld_dcm) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * 8) return;
    const size_t row = i >> 3;
    const int q = (int)(i & 7);
    f32x4 acc = ld4(slab + row * 32 + q * 4);
    for (int gi = 1; gi < groups; ++gi) acc += ld4(slab + ((size_t)gi * rows + row) * 32 + q * 4);
    if (q < 4) st4(dBm + row * ld_dbm + q * 4, acc);
    else st4(dCm + row * ld_dcm + (q - 4) * 4, acc);
}

// out[i] = sum_e slab[e][i], e = 0 .. entries - 1 in order
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slab, int entries, int n,
                                                          float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    for (int e = 0; e < entries; ++e) acc += slab[(size_t)e * n + i];
    out[i] = acc;
}

// ---- causal depthwise conv1d (4 taps) + bias + SiLU ----------------------------------------------------------------
// position s of the walk is token t = s (forward) or L - 1 - s (reverse); y_s = silu(bias + sum_k w[k] x_{s - 3 + k})
// T: the storage type of x / y (and dy / dx below): float, or __bf16 / _Float16.  A lane keeps its four channels for every T
// (the weight registers and the reduction layout do not change), so a 16-bit lane moves 8 bytes and 32 lanes one 256-byte row.
template <typename T>
__global__ __launch_bounds__(256) void conv1d_silu_fwd_kernel(const T* __restrict__ x, int ld_x,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              T* __restrict__ y, int ld_y, int B, int L, int D, int rev) {
    conv1d_silu_fwd_lane<T>(x, ld_x, w, bias, y, ld_y, B, L, D, rev, (size_t)blockIdx.x * 256 + threadIdx.x);
}

// backward: recomputes the pre-activation.  Workgroup = 128 channels (32 quads) x 8 position lanes over CONV_TT positions
// of one sample; its dweight / dbias partial goes to slab[(b * nblk + blk)][D][5].
template <typename T>
__global__ __launch_bounds__(256) void conv1d_silu_bwd_kernel(const T* __restrict__ x, int ld_x,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const T* __restrict__ dy, int ld_dy,
                                                              T* __restrict__ dx, int ld_dx, float* __restrict__ slab,
                                                              int L, int D, int rev) {
    __shared__ float red[8][32][20];
    const int tid = threadIdx.x, cq = tid & 31, tr = tid >> 5;
    const int d = blockIdx.x * CONV_CB + cq * 4;
    const int blk = blockIdx.y, b = blockIdx.z;
    const size_t rowbase = (size_t)b * L;
    f32x4 wv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wv[j] = ld4(w + (d + j) * 4);
    const f32x4 bv = ld4(bias + d);
    float acc[4][5];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[j][k] = 0.f;
    const int send = min(L, (blk + 1) * CONV_TT);
    for (int s = blk * CONV_TT + tr; s < send; s += 8) {
        f32x4 xl[7], dpre[4];
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            const int sm = s - 3 + m;
            xl[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (sm >= 0 && sm < L) xl[m] = ld4(x + (rowbase + (rev ? L - 1 - sm : sm)) * ld_x + d);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            dpre[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (s + m < L) {
                const f32x4 g = ld4(dy + (rowbase + (rev ? L - 1 - (s + m) : s + m)) * ld_dy + d);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float pre = bv[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) pre = fmaf(wv[j][k], xl[m + k][j], pre);
                    const float sg = sigmoid_(pre);
                    dpre[m][j] = g[j] * sg * fmaf(pre, 1.f - sg, 1.f);
                }
            }
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) v = fmaf(wv[j][3 - m], dpre[m][j], v);
            o[j] = v;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[j][k] = fmaf(dpre[0][j], xl[k][j], acc[j][k]);
            acc[j][4] += dpre[0][j];
        }
        st4(dx + (rowbase + (rev ? L - 1 - s : s)) * ld_dx + d, o);
    }
    // red[tr][cq][j * 5 + k]: channel-major within the quad, so the 640 values of a position lane are [128 channels][5]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 5; ++k) red[tr][cq][j * 5 + k] = acc[j][k];
    __syncthreads();
    float* out = slab + (((size_t)b * gridDim.y + blk) * D + (size_t)blockIdx.x * CONV_CB) * 5;
    for (int i = tid; i < 32 * 20; i += 256) {
        float v = (&red[0][0][0])[i];
        for (int r = 1; r < 8; ++r) v += (&red[r][0][0])[i];
        out[i] = v;
    }
}

// dweight[d][k] = sum_e slab[e][d][k], dbias[d] = sum_e slab[e][d][4]
__global__ __launch_bounds__(256) void conv1d_param_reduce_kernel(const float* __restrict__ slab, int entries, int D,
                                                                  float* __restrict__ dw, float* __restrict__ dbias) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D * 5) return;
    float acc = 0.f;
    for (int e = 0; e < entries; ++e) acc += slab[(size_t)e * D * 5 + i];
    const int d = i / 5, k = i % 5;
    if (k < 4) dw[d * 4 + k] = acc;
    else dbias[d] = acc;
}

__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst,
                                                        int ld_dst, size_t rows, int cols4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols4) return;
    const size_t row = i / cols4;
    const int q = (int)(i % cols4) * 4;
    st4(dst + row * ld_dst + q, ld4(src + row * ld_src + q));
}

template <typename T>
__global__ __launch_bounds__(256) void cast_h16_f32_kernel(const T* __restrict__ src, float* __restrict__ dst, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    float v[8];
    ld_piece(src + i * 8, v);
    st4(dst + i * 8, f32x4{v[0], v[1], v[2], v[3]});
    st4(dst + i * 8 + 4, f32x4{v[4], v[5], v[6], v[7]});
}

struct ScanWs { size_t sumd, st, slab_bc, slab_a, slab_d, total; };   // offsets in floats
ScanWs scan_ws(int B, int L, int D) {
    const size_t nc = (size_t)nchunks(L), bc = (size_t)B * nc;
    ScanWs w;
    w.sumd = 0;
    w.st = w.sumd + bc * D;                       // hin (forward without a tape) / gl (backward)
    w.slab_bc = w.st + bc * D * NS;
    w.slab_a = w.slab_bc + (size_t)(D / CPB) * B * L * 32;
    w.slab_d = w.slab_a + bc * D * NS;
    w.total = w.slab_d + bc * D;
    return w;
}

}  // namespace

extern "C" {

int ds6g_selective_scan_chunk(void) { return SCAN_CHUNK; }

size_t ds6g_selective_scan_saved_floats(int B, int L, int D) {
    if (B <= 0 || L <= 0 || D <= 0) return 0;
    return (size_t)B * nchunks(L) * D * NS;
}

size_t ds6g_selective_scan_workspace_bytes(int B, int L, int D) {
    if (B <= 0 || L <= 0 || D <= 0) return 0;
    return scan_ws(B, L, D).total * sizeof(float);
}

size_t ds6g_causal_conv1d_workspace_bytes(int B, int L, int D) {
    if (B <= 0 || L <= 0 || D <= 0) return 0;
    return (size_t)B * ((L + CONV_TT - 1) / CONV_TT) * D * 5 * sizeof(float);
}

// The four operators over the storage type T of their wide operands (x, y, dy, dx; u, z, y, dy, dz): float behind the fp32
// entry points, __bf16 / _Float16 behind the ds6g_h16_* ones.  Same checks, same launches, same workspace for every T.
extern "C++" template <typename T>
static int conv1d_silu_fwd(const void* x, int ld_x, const float* w, const float* bias, void* y, int ld_y, int B, int L, int D,
                           int reverse, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(x && w && bias && y && dims_ok(B, L, D));
    DS6G_CHECK_ARG(ld_okT<T>(ld_x, D) && ld_okT<T>(ld_y, D) && al16(x) && al16(w) && al16(bias) && al16(y));
    const size_t n = (size_t)B * L * (D / 4);
    hipLaunchKernelGGL(conv1d_silu_fwd_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)x, ld_x, w, bias, (T*)y, ld_y, B, L, D, reverse ? 1 : 0);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_causal_conv1d_silu_fwd(const float* x, int ld_x, const float* w, const float* bias, float* y, int ld_y, int B,
                                int L, int D, int reverse, void* stream) {
    return conv1d_silu_fwd<float>(x, ld_x, w, bias, y, ld_y, B, L, D, reverse, stream);
}
int ds6g_h16_causal_conv1d_silu_fwd(int st16, const void* x, int ld_x, const float* w, const float* bias, void* y, int ld_y,
                                    int B, int L, int D, int reverse, void* stream) {
    DS6G_RETURN_H16(st16, conv1d_silu_fwd, x, ld_x, w, bias, y, ld_y, B, L, D, reverse, stream);
}

extern "C++" template <typename T>
static int conv1d_silu_bwd(const void* x, int ld_x, const float* w, const float* bias, const void* dy, int ld_dy, void* dx,
                           int ld_dx, float* dw, float* dbias, int B, int L, int D, int reverse, void* ws, size_t ws_bytes,
                           void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(x && w && bias && dy && dx && dw && dbias && ws && dims_ok(B, L, D));
    DS6G_CHECK_ARG(ld_okT<T>(ld_x, D) && ld_okT<T>(ld_dy, D) && ld_okT<T>(ld_dx, D));
    DS6G_CHECK_ARG(al16(x) && al16(w) && al16(bias) && al16(dy) && al16(dx) && al16(ws));
    DS6G_CHECK_WS(ws_bytes >= ds6g_causal_conv1d_workspace_bytes(B, L, D));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (L + CONV_TT - 1) / CONV_TT;
    hipLaunchKernelGGL(conv1d_silu_bwd_kernel<T>, dim3(D / CONV_CB, nblk, B), dim3(256), 0, st, (const T*)x, ld_x, w, bias,
                       (const T*)dy, ld_dy, (T*)dx, ld_dx, (float*)ws, L, D, reverse ? 1 : 0);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv1d_param_reduce_kernel, dim3(cdiv((long)D * 5, 256)), dim3(256), 0, st, (const float*)ws, B * nblk,
                       D, dw, dbias);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_causal_conv1d_silu_bwd(const float* x, int ld_x, const float* w, const float* bias, const float* dy, int ld_dy,
                                float* dx, int ld_dx, float* dw, float* dbias, int B, int L, int D, int reverse, void* ws,
                                size_t ws_bytes, void* stream) {
    return conv1d_silu_bwd<float>(x, ld_x, w, bias, dy, ld_dy, dx, ld_dx, dw, dbias, B, L, D, reverse, ws, ws_bytes, stream);
}
int ds6g_h16_causal_conv1d_silu_bwd(int st16, const void* x, int ld_x, const float* w, const float* bias, const void* dy,
                                    int ld_dy, void* dx, int ld_dx, float* dw, float* dbias, int B, int L, int D, int reverse,
                                    void* ws, size_t ws_bytes, void* stream) {
    DS6G_RETURN_H16(st16, conv1d_silu_bwd, x, ld_x, w, bias, dy, ld_dy, dx, ld_dx, dw, dbias, B, L, D, reverse, ws, ws_bytes,
                    stream);
}

// 16-bit T: u, z, y are T; delta_raw, Bm, Cm (and everything else) stay fp32 - they come from the fp32 side of the layer's
// storage map (x_proj's output and dt_proj's)
extern "C++" template <typename T>
static int selective_scan_fwd(const void* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                              const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                              const void* z, int ld_z, void* y, int ld_y, float* saved, int B, int L, int D, int reverse,
                              void* ws, size_t ws_bytes, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(u && delta_raw && dt_bias && A_log && Bm && Cm && Dp && z && y && ws && dims_ok(B, L, D));
    DS6G_CHECK_ARG(ld_okT<T>(ld_u, D) && ld_ok(ld_delta, D) && ld_okT<T>(ld_z, D) && ld_okT<T>(ld_y, D) && ld_ok(ld_b, NS) &&
                   ld_ok(ld_c, NS));
    DS6G_CHECK_ARG(al16(u) && al16(delta_raw) && al16(Bm) && al16(Cm) && al16(z) && al16(y) && al16(ws) && al16(saved));
    DS6G_CHECK_WS(ws_bytes >= ds6g_selective_scan_workspace_bytes(B, L, D));
    hipStream_t st = (hipStream_t)stream;
    const ScanWs o = scan_ws(B, L, D);
    float* wsf = (float*)ws;
    ScanP<T> p{};
    p.u = (const T*)u; p.raw = delta_raw; p.dt_bias = dt_bias; p.A_log = A_log; p.Bm = Bm; p.Cm = Cm; p.Dp = Dp;
    p.z = (const T*)z;
    p.ld_u = ld_u; p.ld_raw = ld_delta; p.ld_b = ld_b; p.ld_c = ld_c; p.ld_z = ld_z;
    p.y = (T*)y; p.ld_y = ld_y;
    p.hin = saved ? saved : wsf + o.st;
    p.sumd = wsf + o.sumd;
    p.B = B; p.L = L; p.D = D; p.nc = nchunks(L); p.rev = reverse ? 1 : 0;
    if (p.nc > 1) {
        hipLaunchKernelGGL(scan_state_kernel<T>, dim3(D / CPB, p.nc - 1, B), dim3(256), 0, st, p);
        DS6G_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_carry_kernel<T>, dim3(cdiv((long)B * D * NS, 256)), dim3(256), 0, st, p);
        DS6G_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scan_emit_kernel<T>, dim3(D / CPB, p.nc, B), dim3(256), 0, st, p);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_selective_scan_fwd(const float* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                            const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                            const float* z, int ld_z, float* y, int ld_y, float* saved, int B, int L, int D, int reverse,
                            void* ws, size_t ws_bytes, void* stream) {
    return selective_scan_fwd<float>(u, ld_u, delta_raw, ld_delta, dt_bias, A_log, Bm, ld_b, Cm, ld_c, Dp, z, ld_z, y, ld_y,
                                     saved, B, L, D, reverse, ws, ws_bytes, stream);
}
int ds6g_h16_selective_scan_fwd(int st16, const void* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                                const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                                const void* z, int ld_z, void* y, int ld_y, float* saved, int B, int L, int D, int reverse,
                                void* ws, size_t ws_bytes, void* stream) {
    DS6G_RETURN_H16(st16, selective_scan_fwd, u, ld_u, delta_raw, ld_delta, dt_bias, A_log, Bm, ld_b, Cm, ld_c, Dp, z, ld_z, y,
                    ld_y, saved, B, L, D, reverse, ws, ws_bytes, stream);
}

// 16-bit T: u, z, dy, dz are T; du, ddelta, dBm, dCm stay fp32 (du is the buffer x_proj's data gradient is added to in fp32)
extern "C++" template <typename T>
static int selective_scan_bwd(const void* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                              const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                              const void* z, int ld_z, const void* dy, int ld_dy, const float* saved, float* du, int ld_du,
                              float* ddelta, int ld_ddelta, float* dBm, int ld_dbm, float* dCm, int ld_dcm, void* dz,
                              int ld_dz, float* dA_log, float* dD, int B, int L, int D, int reverse, void* ws,
                              size_t ws_bytes, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(u && delta_raw && dt_bias && A_log && Bm && Cm && Dp && z && dy && saved && du && ddelta && dBm && dCm &&
                   dz && dA_log && dD && ws && dims_ok(B, L, D));
    DS6G_CHECK_ARG(ld_okT<T>(ld_u, D) && ld_ok(ld_delta, D) && ld_okT<T>(ld_z, D) && ld_okT<T>(ld_dy, D) && ld_ok(ld_b, NS) &&
                   ld_ok(ld_c, NS) && ld_ok(ld_du, D) && ld_ok(ld_ddelta, D) && ld_okT<T>(ld_dz, D) && ld_ok(ld_dbm, NS) &&
                   ld_ok(ld_dcm, NS));
    DS6G_CHECK_ARG(al16(u) && al16(delta_raw) && al16(Bm) && al16(Cm) && al16(z) && al16(dy) && al16(saved) && al16(du) &&
                   al16(ddelta) && al16(dBm) && al16(dCm) && al16(dz) && al16(ws));
    DS6G_CHECK_WS(ws_bytes >= ds6g_selective_scan_workspace_bytes(B, L, D));
    hipStream_t st = (hipStream_t)stream;
    const ScanWs o = scan_ws(B, L, D);
    float* wsf = (float*)ws;
    ScanP<T> p{};
    p.u = (const T*)u; p.raw = delta_raw; p.dt_bias = dt_bias; p.A_log = A_log; p.Bm = Bm; p.Cm = Cm; p.Dp = Dp;
    p.z = (const T*)z; p.dy = (const T*)dy;
    p.ld_u = ld_u; p.ld_raw = ld_delta; p.ld_b = ld_b; p.ld_c = ld_c; p.ld_z = ld_z; p.ld_dy = ld_dy;
    p.hin = const_cast<float*>(saved);
    p.sumd = wsf + o.sumd; p.gl = wsf + o.st;
    p.du = du; p.draw = ddelta; p.dz = (T*)dz; p.ld_du = ld_du; p.ld_draw = ld_ddelta; p.ld_dz = ld_dz;
    p.slab_bc = wsf + o.slab_bc; p.slab_a = wsf + o.slab_a; p.slab_d = wsf + o.slab_d;
    p.B = B; p.L = L; p.D = D; p.nc = nchunks(L); p.rev = reverse ? 1 : 0;
    if (p.nc > 1) {
        // chunk 0 is computed too (nobody reads its slot): one chunk in nc, and no special case in the kernel
        hipLaunchKernelGGL(scan_bwd_local_kernel<T>, dim3(D / CPB, p.nc, B), dim3(256), 0, st, p);
        DS6G_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_bwd_carry_kernel<T>, dim3(cdiv((long)B * D * NS, 256)), dim3(256), 0, st, p);
        DS6G_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scan_bwd_main_kernel<T>, dim3(D / CPB, p.nc, B), dim3(256), 0, st, p);
    DS6G_LAUNCH_CHECK();
    const size_t rows = (size_t)B * L;
    hipLaunchKernelGGL(scan_bc_reduce_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st,
                       (const float*)p.slab_bc, D / CPB, rows, dBm, ld_dbm, dCm, ld_dcm);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(cdiv((long)D * NS, 256)), dim3(256), 0, st, (const float*)p.slab_a,
                       B * p.nc, D * NS, dA_log);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(cdiv(D, 256)), dim3(256), 0, st, (const float*)p.slab_d, B * p.nc, D, dD);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_selective_scan_bwd(const float* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                            const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                            const float* z, int ld_z, const float* dy, int ld_dy, const float* saved, float* du, int ld_du,
                            float* ddelta, int ld_ddelta, float* dBm, int ld_dbm, float* dCm, int ld_dcm, float* dz,
                            int ld_dz, float* dA_log, float* dD, int B, int L, int D, int reverse, void* ws,
                            size_t ws_bytes, void* stream) {
    return selective_scan_bwd<float>(u, ld_u, delta_raw, ld_delta, dt_bias, A_log, Bm, ld_b, Cm, ld_c, Dp, z, ld_z, dy, ld_dy,
                                     saved, du, ld_du, ddelta, ld_ddelta, dBm, ld_dbm, dCm, ld_dcm, dz, ld_dz, dA_log, dD, B, L,
                                     D, reverse, ws, ws_bytes, stream);
}
int ds6g_h16_selective_scan_bwd(int st16, const void* u, int ld_u, const float* delta_raw, int ld_delta, const float* dt_bias,
                                const float* A_log, const float* Bm, int ld_b, const float* Cm, int ld_c, const float* Dp,
                                const void* z, int ld_z, const void* dy, int ld_dy, const float* saved, float* du, int ld_du,
                                float* ddelta, int ld_ddelta, float* dBm, int ld_dbm, float* dCm, int ld_dcm, void* dz,
                                int ld_dz, float* dA_log, float* dD, int B, int L, int D, int reverse, void* ws,
                                size_t ws_bytes, void* stream) {
    DS6G_RETURN_H16(st16, selective_scan_bwd, u, ld_u, delta_raw, ld_delta, dt_bias, A_log, Bm, ld_b, Cm, ld_c, Dp, z, ld_z, dy,
                    ld_dy, saved, du, ld_du, ddelta, ld_ddelta, dBm, ld_dbm, dCm, ld_dcm, dz, ld_dz, dA_log, dD, B, L, D,
                    reverse, ws, ws_bytes, stream);
}

// dst (fp32) = src (bf16 / f16), exact; n % 8 == 0, both 16-byte aligned.  The layer's 16-bit path widens xc with it for the
// fp32 weight-gradient GEMM of x_proj, whose r + 32 output rows the 16-bit GEMM's shape rules do not admit.
extern "C++" template <typename T>
static int cast_h16_f32(const void* src, float* dst, long n, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(src && dst && n > 0 && n % 8 == 0 && al16(src) && al16(dst));
    const long n8 = n / 8;
    hipLaunchKernelGGL(cast_h16_f32_kernel<T>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)src, dst, n8);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_cast_h16_f32(int st16, const void* src, float* dst, long n, void* stream) {
    DS6G_RETURN_H16(st16, cast_h16_f32, src, dst, n, stream);
}

int ds6g_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, long rows, int cols, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(src && dst && rows > 0 && cols > 0 && cols % 4 == 0 && ld_ok(ld_src, cols) && ld_ok(ld_dst, cols) &&
                   al16(src) && al16(dst));
    const size_t n = (size_t)rows * (cols / 4);
    hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, ld_src,
                       dst, ld_dst, (size_t)rows, cols / 4);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

}  // extern "C"
