// The bi-branch Mamba fusion stage's operators that are neither a GEMM nor part of the Mamba layer (reference call sites
// mambafuser_seq.py:79,94 ln1 = LayerNorm((T, C)); :100-107 the gate; :200-214 the channel-swapping token pack; :219-231 the
// unpack), fp32:
//   sample LayerNorm   one mean / variance per SAMPLE over its n = T * C values, affine weight and bias of n elements;
//   bi-branch gate     out[b, t] = bmN[b, L-1-t] * (leaky_0.2(f2N[b, L-1-t]) + fm[b, t]): the reverse-walk Mamba's and fc2's
//                      outputs stay in natural token order in memory and are read back to front, no flip copy;
//   swap pack          three NCHW [B*S][C][8][8] maps + gps [B][2][C] -> tokens [B][T][C] = dropout(pos_emb + swapped tokens);
//   token unpack       tokens -> three NCHW maps + [B][2][C], no swap;
//   pool swap tokens   the pack for the model walk: three NHWC [B*S][H][H][C] maps, pooled to 8 x 8 as they are swapped.
// All five are bandwidth-class.  Sums that cross workgroups (the sample statistics, the two sample sums of the LayerNorm
// backward) go through partial slabs reduced in a fixed order; sums over the batch (dgamma, dbeta, dpos) are loops over b in
// index order inside one thread: no float atomics, two runs are bit-identical.
#include "common.h"

namespace {

constexpr int LN_CHUNK = 2048;     // floats per workgroup of the statistics / apply passes (256 threads x 2 float4)
constexpr int LN_COLS = 1024;      // floats per workgroup of the backward's batch-loop pass (256 threads x 1 float4)
constexpr int HW = 64;             // positions per feature map (8 x 8)
constexpr int TC = 64;             // channels per transpose tile
constexpr int TLD = TC + 1;        // LDS row stride of the tile: a column walk touches every bank

// sum over the 256 threads of the workgroup, delivered to all of them; fixed order (butterfly inside the wave, the four
// waves in index order).  `red` is 4 doubles of LDS; two barriers.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_reduce_sum_d(v);
    __syncthreads();               // the previous call's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- sample LayerNorm ------------------------------------------------------------------------------------------------
// statistics pass: workgroup (chunk, b) -> part[b][chunk] = (mean of the chunk, sum of squared deviations from THAT mean).
// The chunk stays in registers between the two sums, so the variance is never a difference of two large numbers.
__global__ __launch_bounds__(256) void sln_stats_kernel(const float* __restrict__ x, size_t n, double* __restrict__ part) {
    __shared__ double red[4];
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t c0 = (size_t)chunk * LN_CHUNK;
    const int len = (int)min((size_t)LN_CHUNK, n - c0);
    const float* xs = x + (size_t)b * n + c0;
    f32x4 v[2];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = (k * 256 + tid) * 4;
        v[k] = i < len ? ld4(xs + i) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
    }
    const double mu = block_sum_d((double)s, red) / (double)len;
    const float muf = (float)mu;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = (k * 256 + tid) * 4;
        if (i < len) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = v[k][j] - muf; q = fmaf(d, d, q); }
        }
    }
    const double m2 = block_sum_d((double)q, red);
    if (tid == 0) {
        double* o = part + ((size_t)b * gridDim.x + chunk) * 2;
        o[0] = (double)muf;        // the deviations were taken from the rounded mean: combine with that one
        o[1] = m2;
    }
}

// one workgroup per sample: mean = sum n_c mean_c / n;  M2 = sum (M2_c + n_c (mean_c - mean)^2)   (Chan et al., all chunks
// at once; in double, fixed order)
__global__ __launch_bounds__(256) void sln_stats_finalize_kernel(const double* __restrict__ part, int nchunk, size_t n,
                                                                 float eps, float* __restrict__ mean,
                                                                 float* __restrict__ rstd) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const double* p = part + (size_t)b * nchunk * 2;
    double s = 0.0;
    for (int c = threadIdx.x; c < nchunk; c += 256) {
        const double cnt = (double)min((size_t)LN_CHUNK, n - (size_t)c * LN_CHUNK);
        s += cnt * p[c * 2];
    }
    const double mu = block_sum_d(s, red) / (double)n;
    double q = 0.0;
    for (int c = threadIdx.x; c < nchunk; c += 256) {
        const double cnt = (double)min((size_t)LN_CHUNK, n - (size_t)c * LN_CHUNK);
        const double d = p[c * 2] - mu;
        q += p[c * 2 + 1] + cnt * d * d;
    }
    const double var = block_sum_d(q, red) / (double)n;
    if (threadIdx.x == 0) {
        mean[b] = (float)mu;
        rstd[b] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

__global__ __launch_bounds__(256) void sln_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, float* __restrict__ y, size_t n) {
    const int b = blockIdx.y;
    const float mu = mean[b], rs = rstd[b];
    const size_t c0 = (size_t)blockIdx.x * LN_CHUNK;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const size_t i = c0 + (size_t)(k * 256 + threadIdx.x) * 4;
        if (i < n) {
            const f32x4 xv = ld4(x + (size_t)b * n + i), g = ld4(gamma + i), bb = ld4(beta + i);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaf((xv[j] - mu) * rs, g[j], bb[j]);
            st4(y + (size_t)b * n + i, o);
        }
    }
}

// backward, batch-loop pass: a thread owns four consecutive columns of the sample and walks b = 0 .. B - 1 in order:
// dgamma / dbeta are complete in its registers, the two sample sums (g = dy gamma; sum g, sum g xhat) leave as one partial per
// (b, wave): part[b][blk * 4 + wave] = (sum g, sum g xhat)
__global__ __launch_bounds__(256) void sln_bwd_cols_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, double* __restrict__ part, int B,
                                                           size_t n, int accumulate) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const bool on = i < n;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), nslot = gridDim.x * 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 g = on ? ld4(gamma + i) : zero;
    f32x4 dg = zero, db = zero;
    for (int b = 0; b < B; ++b) {
        const float mu = mean[b], rs = rstd[b];
        const f32x4 d = on ? ld4(dy + (size_t)b * n + i) : zero;
        const f32x4 xv = on ? ld4(x + (size_t)b * n + i) : zero;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = on ? (xv[j] - mu) * rs : 0.f;
            const float gj = d[j] * g[j];
            dg[j] = fmaf(d[j], xh, dg[j]);
            db[j] += d[j];
            s1 += gj;
            s2 = fmaf(gj, xh, s2);
        }
        const double r1 = wave_reduce_sum_d((double)s1), r2 = wave_reduce_sum_d((double)s2);
        if ((threadIdx.x & 63) == 0) {
            double* o = part + ((size_t)b * nslot + slot) * 2;
            o[0] = r1;
            o[1] = r2;
        }
    }
    if (on) {
        if (accumulate) { dg += ld4(dgamma + i); db += ld4(dbeta + i); }
        st4(dgamma + i, dg);
        st4(dbeta + i, db);
    }
}

// one workgroup per sample: coef[b] = (mean(g), mean(g xhat))
__global__ __launch_bounds__(256) void sln_bwd_finalize_kernel(const double* __restrict__ part, int nslot, size_t n,
                                                               float* __restrict__ coef) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const double* p = part + (size_t)b * nslot * 2;
    double s1 = 0.0, s2 = 0.0;
    for (int c = threadIdx.x; c < nslot; c += 256) { s1 += p[c * 2]; s2 += p[c * 2 + 1]; }
    s1 = block_sum_d(s1, red);
    s2 = block_sum_d(s2, red);
    if (threadIdx.x == 0) {
        coef[b * 2] = (float)(s1 / (double)n);
        coef[b * 2 + 1] = (float)(s2 / (double)n);
    }
}

// dx = rstd (g - mean(g) - xhat mean(g xhat))
__global__ __launch_bounds__(256) void sln_bwd_dx_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ gamma, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ coef,
                                                         float* __restrict__ dx, size_t n) {
    const int b = blockIdx.y;
    const float mu = mean[b], rs = rstd[b], c1 = coef[b * 2], c2 = coef[b * 2 + 1];
    const size_t c0 = (size_t)blockIdx.x * LN_CHUNK;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const size_t i = c0 + (size_t)(k * 256 + threadIdx.x) * 4;
        if (i < n) {
            const f32x4 d = ld4(dy + (size_t)b * n + i), xv = ld4(x + (size_t)b * n + i), g = ld4(gamma + i);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (xv[j] - mu) * rs;
                o[j] = rs * ((d[j] * g[j] - c1) - xh * c2);
            }
            st4(dx + (size_t)b * n + i, o);
        }
    }
}

// ---- bi-branch gate --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.2f * v; }

__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* __restrict__ fm, int ld_fm, const float* __restrict__ bm,
                                                       int ld_bm, const float* __restrict__ f2, int ld_f2,
                                                       float* __restrict__ out, int ld_out, int B, int L, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int q4 = C >> 2;
    if (i >= (size_t)B * L * q4) return;
    const size_t row = i / q4;
    const int c = (int)(i % q4) * 4;
    const size_t b = row / L;
    const size_t rrow = b * L + (L - 1 - (row - b * L));
    const f32x4 a = ld4(fm + row * ld_fm + c), m = ld4(bm + rrow * ld_bm + c), f = ld4(f2 + rrow * ld_f2 + c);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = m[j] * (leaky(f[j]) + a[j]);
    st4(out + row * ld_out + c, o);
}

// indexed by the row r of bmN / f2N (their natural order); the matching output row is t = L - 1 - r
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ dout, int ld_do, const float* __restrict__ fm,
                                                       int ld_fm, const float* __restrict__ bm, int ld_bm,
                                                       const float* __restrict__ f2, int ld_f2, float* __restrict__ dfm,
                                                       int ld_dfm, float* __restrict__ dbm, int ld_dbm,
                                                       float* __restrict__ df2, int ld_df2, int B, int L, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int q4 = C >> 2;
    if (i >= (size_t)B * L * q4) return;
    const size_t rrow = i / q4;
    const int c = (int)(i % q4) * 4;
    const size_t b = rrow / L;
    const size_t row = b * L + (L - 1 - (rrow - b * L));
    const f32x4 g = ld4(dout + row * ld_do + c), a = ld4(fm + row * ld_fm + c), m = ld4(bm + rrow * ld_bm + c),
                f = ld4(f2 + rrow * ld_f2 + c);
    f32x4 oa, om, of;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gm = g[j] * m[j];
        oa[j] = gm;
        om[j] = g[j] * (leaky(f[j]) + a[j]);
        of[j] = f[j] > 0.f ? gm : 0.2f * gm;
    }
    st4(dfm + row * ld_dfm + c, oa);
    st4(dbm + rrow * ld_dbm + c, om);
    st4(df2 + rrow * ld_df2 + c, of);
}

// ---- token pack / unpack ---------------------------------------------------------------------------------------------
// Token row of (modality m, frame s, position hw) of a sample: (m * S + s) * 64 + hw; the two gps rows come last.
// swap: channel c of modality m's tokens lives in the map of modality (m + seg(c)) % 3, seg = 0 / 1 / 2 for c < C/3,
// c < 2 (C/3), the rest.  Workgroup = (modality, frame, 64-channel block) of one sample, or the sample's two gps rows
// (blockIdx.x == gridDim.x - 1).  The 64 x 64 tile goes through LDS, so the map side moves 256-byte position rows and the
// token side 256-byte channel rows.
struct Maps { float* m[3]; };

__device__ __forceinline__ int src_mod(int m, int c, int s1, int s2, int swap) {
    if (!swap) return m;
    const int k = m + (c < s1 ? 0 : (c < s2 ? 1 : 2));
    return k >= 3 ? k - 3 : k;
}

__device__ __forceinline__ f32x4 drop4(f32x4 v, uint64_t seed, uint64_t ctr, uint32_t thr, float scale) {
    if (thr) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ds6g_keep(seed, ctr + j, thr) ? v[j] * scale : 0.f;
    }
    return v;
}

// tokens = dropout(pos + gather(maps, gps)); pos nullable (the unpack's backward: no pos, no dropout, no swap)
__global__ __launch_bounds__(256) void maps_to_tokens_kernel(const Maps maps, const float* __restrict__ gps,
                                                             const float* __restrict__ pos, float* __restrict__ tok, int S,
                                                             int C, int swap, uint32_t thr, float scale, uint64_t seed,
                                                             uint64_t seed_off_in, const uint64_t* __restrict__ salt) {
    __shared__ float tile[HW * TLD];
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const int b = blockIdx.y, tid = threadIdx.x;
    const int T = 3 * S * HW + 2;
    const int ncb = C / TC;
    if ((int)blockIdx.x == 3 * S * ncb) {   // the gps rows
        for (int i = tid * 4; i < 2 * C; i += 1024) {
            const size_t o = ((size_t)b * T + (T - 2)) * C + i;
            f32x4 v = ld4(gps + (size_t)b * 2 * C + i);
            if (pos) v += ld4(pos + (size_t)(T - 2) * C + i);
            st4(tok + o, drop4(v, seed, seed_off + o, thr, scale));
        }
        return;
    }
    const int cb = blockIdx.x % ncb, ms = blockIdx.x / ncb;
    const int m = ms / S, s = ms - m * S;
    const int s1 = C / 3, s2 = s1 * 2;
    {
        const int q = tid & 15;              // position quad
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cl = k * 16 + (tid >> 4), c = cb * TC + cl;
            const float* src = maps.m[src_mod(m, c, s1, s2, swap)] + (((size_t)b * S + s) * C + c) * HW;
            const f32x4 v = ld4(src + q * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[(q * 4 + j) * TLD + cl] = v[j];
        }
    }
    __syncthreads();
    {
        const int q = tid & 15;              // channel quad
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int hw = k * 16 + (tid >> 4);
            const size_t row = (size_t)ms * HW + hw;
            const size_t o = ((size_t)b * T + row) * C + cb * TC + q * 4;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = tile[hw * TLD + q * 4 + j];
            if (pos) v += ld4(pos + row * C + cb * TC + q * 4);
            st4(tok + o, drop4(v, seed, seed_off + o, thr, scale));
        }
    }
}

// maps / gps <- scatter(dropout-mask(tokens)): the pack's backward (swap, mask) and the unpack's forward (neither)
__global__ __launch_bounds__(256) void tokens_to_maps_kernel(const float* __restrict__ tok, const Maps maps,
                                                             float* __restrict__ gps, int S, int C, int swap, uint32_t thr,
                                                             float scale, uint64_t seed, uint64_t seed_off_in,
                                                             const uint64_t* __restrict__ salt) {
    __shared__ float tile[HW * TLD];
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const int b = blockIdx.y, tid = threadIdx.x;
    const int T = 3 * S * HW + 2;
    const int ncb = C / TC;
    if ((int)blockIdx.x == 3 * S * ncb) {
        for (int i = tid * 4; i < 2 * C; i += 1024) {
            const size_t o = ((size_t)b * T + (T - 2)) * C + i;
            st4(gps + (size_t)b * 2 * C + i, drop4(ld4(tok + o), seed, seed_off + o, thr, scale));
        }
        return;
    }
    const int cb = blockIdx.x % ncb, ms = blockIdx.x / ncb;
    const int m = ms / S, s = ms - m * S;
    const int s1 = C / 3, s2 = s1 * 2;
    {
        const int q = tid & 15;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int hw = k * 16 + (tid >> 4);
            const size_t o = ((size_t)b * T + (size_t)ms * HW + hw) * C + cb * TC + q * 4;
            const f32x4 v = drop4(ld4(tok + o), seed, seed_off + o, thr, scale);
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[hw * TLD + q * 4 + j] = v[j];
        }
    }
    __syncthreads();
    {
        const int q = tid & 15;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int cl = k * 16 + (tid >> 4), c = cb * TC + cl;
            float* dst = maps.m[src_mod(m, c, s1, s2, swap)] + (((size_t)b * S + s) * C + c) * HW;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = tile[(q * 4 + j) * TLD + cl];
            st4(dst + q * 4, v);
        }
    }
}

// dpos[i] = sum over b, in index order, of the masked token gradient
__global__ __launch_bounds__(256) void pos_grad_kernel(const float* __restrict__ dtok, float* __restrict__ dpos, int B,
                                                       size_t tc, uint32_t thr, float scale, uint64_t seed,
                                                       uint64_t seed_off_in, const uint64_t* __restrict__ salt,
                                                       int accumulate) {
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= tc) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
        const size_t o = (size_t)b * tc + i;
        acc += drop4(ld4(dtok + o), seed, seed_off + o, thr, scale);
    }
    if (accumulate) acc += ld4(dpos + i);
    st4(dpos + i, acc);
}

// ---- NHWC token pack of the model walk --------------------------------------------------------------------------------
// The walk keeps the three modality maps NHWC [B*S][H][H][C] at full resolution, so the pack pools as it swaps:
//   tokens[b][(m S + f) 64 + ph 8 + pw][c] = dropout(pos + mean over window (ph, pw) of map_q[b S + f][.][.][c]),
//   q = (m + seg(c)) % 3; seen from the SOURCE map q, channel c goes to the token rows of modality (q - seg(c)) mod 3.
// Workgroup = (sample b, source map q, frame f, row ph of 8 windows), or the sample's two gps rows (blockIdx.x ==
// gridDim.x - 1).  A pooled float4 is computed once and stored to the destination row of its segment; the two float4 groups
// per row that straddle a segment cut (C/3 and 2 (C/3) are never multiples of 4 here) go element by element.
constexpr int PST_CMAX = 512;      // widest map: the backward keeps 8 x C masked token gradients in LDS

struct PoolMaps { const float* in[3]; float* out[3]; };

__device__ __forceinline__ int swap_seg(int c, int s1, int s2) { return c < s1 ? 0 : (c < s2 ? 1 : 2); }
// token row (inside the sample) that channel segment `sg` of source map q pairs with, at frame f and window hw
__device__ __forceinline__ int swap_row(int q, int sg, int S, int f, int hw) {
    const int m = q - sg;
    return ((m < 0 ? m + 3 : m) * S + f) * HW + hw;
}

__global__ __launch_bounds__(256) void pool_swap_tokens_fwd_kernel(const PoolMaps maps, const float* __restrict__ gemb,
                                                                   const float* __restrict__ pos, float* __restrict__ tok,
                                                                   int S, int H, int C, uint32_t thr, float scale,
                                                                   uint64_t seed, uint64_t seed_off_in,
                                                                   const uint64_t* __restrict__ salt) {
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const int b = blockIdx.y, tid = threadIdx.x;
    const int T = 3 * S * HW + 2;
    if ((int)blockIdx.x == 3 * S * 8) {     // the gps rows
        for (int i = tid * 4; i < 2 * C; i += 1024) {
            const size_t o = ((size_t)b * T + (T - 2)) * C + i;
            const f32x4 v = ld4(gemb + (size_t)b * 2 * C + i) + ld4(pos + (size_t)(T - 2) * C + i);
            st4(tok + o, drop4(v, seed, seed_off + o, thr, scale));
        }
        return;
    }
    const int ph = blockIdx.x & 7, qf = blockIdx.x >> 3;
    const int q = qf / S, f = qf - q * S;
    const int k = H >> 3, cg = C >> 2;
    const int s1 = C / 3, s2 = s1 * 2;
    const float inv = 1.0f / (float)(k * k);
    const float* feat = maps.in[q] + ((size_t)b * S + f) * H * H * C;
    for (int it = tid; it < 8 * cg; it += 256) {
        const int pw = it / cg, c4 = (it - pw * cg) * 4;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < k; ++r)
            for (int u = 0; u < k; ++u) s += ld4(feat + ((size_t)(ph * k + r) * H + pw * k + u) * C + c4);
        s *= inv;
        const int hw = ph * 8 + pw;
        const int g0 = swap_seg(c4, s1, s2), g3 = swap_seg(c4 + 3, s1, s2);
        if (g0 == g3) {
            const int row = swap_row(q, g0, S, f, hw);
            const size_t o = ((size_t)b * T + row) * C + c4;
            st4(tok + o, drop4(s + ld4(pos + (size_t)row * C + c4), seed, seed_off + o, thr, scale));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = swap_row(q, swap_seg(c4 + j, s1, s2), S, f, hw);
                const size_t o = ((size_t)b * T + row) * C + c4 + j;
                float v = s[j] + pos[(size_t)row * C + c4 + j];
                if (thr) v = ds6g_keep(seed, seed_off + o, thr) ? v * scale : 0.f;
                tok[o] = v;
            }
        }
    }
}

// dfeat_q = dfeat_in_q + (masked token gradient of the window) / k^2, dgemb = the masked gps-row gradient.  Same workgroups
// as the forward: the 8 x C masked, scaled gradients of the row of windows are gathered into LDS through the inverse swap,
// then spread over the k pixel rows x H pixels the windows cover (in == out is allowed: an element is read, then written,
// by one thread).
__global__ __launch_bounds__(256) void pool_swap_tokens_bwd_kernel(const float* __restrict__ dtok, const PoolMaps maps,
                                                                   float* __restrict__ dgemb, int S, int H, int C,
                                                                   uint32_t thr, float scale, uint64_t seed,
                                                                   uint64_t seed_off_in, const uint64_t* __restrict__ salt) {
    __shared__ f32x4 gs[8 * PST_CMAX / 4];
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const int b = blockIdx.y, tid = threadIdx.x;
    const int T = 3 * S * HW + 2;
    if ((int)blockIdx.x == 3 * S * 8) {
        for (int i = tid * 4; i < 2 * C; i += 1024) {
            const size_t o = ((size_t)b * T + (T - 2)) * C + i;
            st4(dgemb + (size_t)b * 2 * C + i, drop4(ld4(dtok + o), seed, seed_off + o, thr, scale));
        }
        return;
    }
    const int ph = blockIdx.x & 7, qf = blockIdx.x >> 3;
    const int q = qf / S, f = qf - q * S;
    const int k = H >> 3, cg = C >> 2;
    const int s1 = C / 3, s2 = s1 * 2;
    const float inv = 1.0f / (float)(k * k);
    for (int it = tid; it < 8 * cg; it += 256) {
        const int pw = it / cg, c4 = (it - pw * cg) * 4;
        const int hw = ph * 8 + pw;
        const int g0 = swap_seg(c4, s1, s2), g3 = swap_seg(c4 + 3, s1, s2);
        f32x4 v;
        if (g0 == g3) {
            const size_t o = ((size_t)b * T + swap_row(q, g0, S, f, hw)) * C + c4;
            v = drop4(ld4(dtok + o), seed, seed_off + o, thr, scale);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t o = ((size_t)b * T + swap_row(q, swap_seg(c4 + j, s1, s2), S, f, hw)) * C + c4 + j;
                const float d = dtok[o];
                v[j] = thr ? (ds6g_keep(seed, seed_off + o, thr) ? d * scale : 0.f) : d;
            }
        }
        gs[it] = v * inv;
    }
    __syncthreads();
    const size_t base = (((size_t)b * S + f) * H + (size_t)ph * k) * H * C;   // k full pixel rows: k * H * C contiguous floats
    const float* din = maps.in[q];
    float* dout = maps.out[q];
    const int n4 = k * H * cg;
    for (int it = tid; it < n4; it += 256) {
        const int c4i = it % cg, w = (it / cg) % H;
        f32x4 v = gs[(w / k) * cg + c4i];
        const size_t o = base + (size_t)it * 4;
        if (din) v += ld4(din + o);
        st4(dout + o, v);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool ld_ok(int ld, int width) { return ld >= width && ld % 4 == 0; }
inline bool sln_dims_ok(int B, long n) { return B > 0 && B <= 65535 && n > 0 && n % 4 == 0 && n <= (1L << 30); }
inline int sln_chunks(long n) { return (int)((n + LN_CHUNK - 1) / LN_CHUNK); }
inline int sln_colblocks(long n) { return (int)((n + LN_COLS - 1) / LN_COLS); }
inline bool gate_dims_ok(int B, int L, int C) {
    // the grid: one thread per float4
    return B > 0 && L > 0 && C > 0 && C % 4 == 0 && C <= (1 << 16) && (long)B * L < (1L << 31) / 64 &&
           (long)B * L * (C / 4) < (1L << 31) * 128;
}
inline bool tok_dims_ok(int B, int S, int C) {
    return B > 0 && B <= 65535 && S > 0 && S <= 4096 && C > 0 && C % TC == 0 && C <= 4096;
}
inline bool pool_dims_ok(int B, int S, int H, int C) {
    return B > 0 && B <= 65535 && S > 0 && S <= 4096 && H >= 8 && H <= 64 && H % 8 == 0 && C >= 4 && C % 4 == 0 &&
           C <= PST_CMAX;
}

}  // namespace

extern "C" {

size_t ds6g_sample_layernorm_workspace_bytes(int B, long n) {
    if (B <= 0 || n <= 0) return 0;
    // forward: (mean, M2) per chunk; backward: two sums per (column block, wave) + two coefficients per sample
    const size_t fwd = (size_t)B * sln_chunks(n) * 2 * sizeof(double);
    const size_t bwd = (size_t)B * sln_colblocks(n) * 4 * 2 * sizeof(double) + (size_t)B * 2 * sizeof(float);
    return fwd > bwd ? fwd : bwd;
}

int ds6g_sample_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                              int B, long n, float eps, void* ws, size_t ws_bytes, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(x && gamma && beta && y && mean && rstd && ws && sln_dims_ok(B, n) && eps > 0.f);
    DS6G_CHECK_ARG(al16(x) && al16(gamma) && al16(beta) && al16(y) && al16(ws));
    DS6G_CHECK_WS(ws_bytes >= ds6g_sample_layernorm_workspace_bytes(B, n));
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = sln_chunks(n);
    double* part = (double*)ws;
    hipLaunchKernelGGL(sln_stats_kernel, dim3(nchunk, B), dim3(256), 0, st, x, (size_t)n, part);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_stats_finalize_kernel, dim3(B), dim3(256), 0, st, (const double*)part, nchunk, (size_t)n, eps, mean,
                       rstd);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_apply_kernel, dim3(nchunk, B), dim3(256), 0, st, x, gamma, beta, (const float*)mean,
                       (const float*)rstd, y, (size_t)n);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_sample_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                              float* dx, float* dgamma, float* dbeta, int B, long n, int accumulate_param_grads, void* ws,
                              size_t ws_bytes, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dy && x && mean && rstd && gamma && dx && dgamma && dbeta && ws && sln_dims_ok(B, n));
    DS6G_CHECK_ARG(al16(dy) && al16(x) && al16(gamma) && al16(dx) && al16(dgamma) && al16(dbeta) && al16(ws));
    DS6G_CHECK_WS(ws_bytes >= ds6g_sample_layernorm_workspace_bytes(B, n));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = sln_colblocks(n);
    double* part = (double*)ws;
    float* coef = (float*)(part + (size_t)B * nblk * 4 * 2);
    hipLaunchKernelGGL(sln_bwd_cols_kernel, dim3(nblk), dim3(256), 0, st, dy, x, gamma, mean, rstd, dgamma, dbeta, part, B,
                       (size_t)n, accumulate_param_grads ? 1 : 0);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_bwd_finalize_kernel, dim3(B), dim3(256), 0, st, (const double*)part, nblk * 4, (size_t)n, coef);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_bwd_dx_kernel, dim3(sln_chunks(n), B), dim3(256), 0, st, dy, x, gamma, mean, rstd,
                       (const float*)coef, dx, (size_t)n);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_bimamba_gate_fwd(const float* fm, int ld_fm, const float* bm, int ld_bm, const float* f2, int ld_f2, float* out,
                          int ld_out, int B, int L, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(fm && bm && f2 && out && gate_dims_ok(B, L, C));
    DS6G_CHECK_ARG(ld_ok(ld_fm, C) && ld_ok(ld_bm, C) && ld_ok(ld_f2, C) && ld_ok(ld_out, C));
    DS6G_CHECK_ARG(al16(fm) && al16(bm) && al16(f2) && al16(out));
    const size_t nq = (size_t)B * L * (C / 4);
    hipLaunchKernelGGL(gate_fwd_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fm, ld_fm, bm,
                       ld_bm, f2, ld_f2, out, ld_out, B, L, C);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_bimamba_gate_bwd(const float* dout, int ld_dout, const float* fm, int ld_fm, const float* bm, int ld_bm,
                          const float* f2, int ld_f2, float* dfm, int ld_dfm, float* dbm, int ld_dbm, float* df2, int ld_df2,
                          int B, int L, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dout && fm && bm && f2 && dfm && dbm && df2 && gate_dims_ok(B, L, C));
    DS6G_CHECK_ARG(ld_ok(ld_dout, C) && ld_ok(ld_fm, C) && ld_ok(ld_bm, C) && ld_ok(ld_f2, C) && ld_ok(ld_dfm, C) &&
                   ld_ok(ld_dbm, C) && ld_ok(ld_df2, C));
    DS6G_CHECK_ARG(al16(dout) && al16(fm) && al16(bm) && al16(f2) && al16(dfm) && al16(dbm) && al16(df2));
    const size_t nq = (size_t)B * L * (C / 4);
    hipLaunchKernelGGL(gate_bwd_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dout, ld_dout,
                       fm, ld_fm, bm, ld_bm, f2, ld_f2, dfm, ld_dfm, dbm, ld_dbm, df2, ld_df2, B, L, C);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_swap_pack_fwd(const float* image, const float* lidar, const float* radar, const float* gps, const float* pos_emb,
                       float* tokens, int B, int S, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(image && lidar && radar && gps && pos_emb && tokens && tok_dims_ok(B, S, C));
    DS6G_CHECK_ARG(al16(image) && al16(lidar) && al16(radar) && al16(gps) && al16(pos_emb) && al16(tokens));
    DS6G_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f);
    Maps maps{{const_cast<float*>(image), const_cast<float*>(lidar), const_cast<float*>(radar)}};
    hipLaunchKernelGGL(maps_to_tokens_kernel, dim3(3 * S * (C / TC) + 1, B), dim3(256), 0, (hipStream_t)stream, maps, gps,
                       pos_emb, tokens, S, C, 1, ds6g_drop_threshold(drop_p), 1.f / (1.f - drop_p), seed, seed_off,
                       g_ds6g_salt);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_swap_pack_bwd(const float* dtokens, float* dimage, float* dlidar, float* dradar, float* dgps, float* dpos_emb, int B,
                       int S, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dtokens && dimage && dlidar && dradar && dgps && dpos_emb && tok_dims_ok(B, S, C));
    DS6G_CHECK_ARG(al16(dtokens) && al16(dimage) && al16(dlidar) && al16(dradar) && al16(dgps) && al16(dpos_emb));
    DS6G_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t thr = ds6g_drop_threshold(drop_p);
    const float scale = 1.f / (1.f - drop_p);
    Maps maps{{dimage, dlidar, dradar}};
    hipLaunchKernelGGL(tokens_to_maps_kernel, dim3(3 * S * (C / TC) + 1, B), dim3(256), 0, st, dtokens, maps, dgps, S, C, 1,
                       thr, scale, seed, seed_off, g_ds6g_salt);
    DS6G_LAUNCH_CHECK();
    const size_t tc = (size_t)(3 * S * HW + 2) * C;
    hipLaunchKernelGGL(pos_grad_kernel, dim3((unsigned)((tc / 4 + 255) / 256)), dim3(256), 0, st, dtokens, dpos_emb, B, tc,
                       thr, scale, seed, seed_off, g_ds6g_salt, 0);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_pool_swap_tokens_fwd(const ds6g_map_desc* maps, const float* gemb, const float* pos_emb, float* tokens, int B, int S,
                              int H, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(maps && gemb && pos_emb && tokens && pool_dims_ok(B, S, H, C));
    DS6G_CHECK_ARG(al16(gemb) && al16(pos_emb) && al16(tokens) && drop_p >= 0.f && drop_p < 1.f);
    PoolMaps pm{};
    for (int m = 0; m < 3; ++m) {
        DS6G_CHECK_ARG(maps[m].in && al16(maps[m].in) && maps[m].frames_per_sample == S && maps[m].mod_off == m * S * HW);
        pm.in[m] = (const float*)maps[m].in;
    }
    hipLaunchKernelGGL(pool_swap_tokens_fwd_kernel, dim3(3 * S * 8 + 1, B), dim3(256), 0, (hipStream_t)stream, pm, gemb,
                       pos_emb, tokens, S, H, C, ds6g_drop_threshold(drop_p), 1.f / (1.f - drop_p), seed, seed_off,
                       g_ds6g_salt);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_pool_swap_tokens_bwd(const ds6g_map_desc* maps, const float* dtokens, float* dgemb, float* dpos_emb,
                              int accumulate_dpos, int B, int S, int H, int C, float drop_p, uint64_t seed,
                              uint64_t seed_off, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(maps && dtokens && dgemb && dpos_emb && pool_dims_ok(B, S, H, C));
    DS6G_CHECK_ARG(al16(dtokens) && al16(dgemb) && al16(dpos_emb) && drop_p >= 0.f && drop_p < 1.f);
    PoolMaps pm{};
    for (int m = 0; m < 3; ++m) {
        DS6G_CHECK_ARG(maps[m].out && al16(maps[m].out) && al16(maps[m].in) && maps[m].frames_per_sample == S &&
                       maps[m].mod_off == m * S * HW);
        pm.in[m] = (const float*)maps[m].in;
        pm.out[m] = (float*)maps[m].out;
    }
    hipStream_t st = (hipStream_t)stream;
    const uint32_t thr = ds6g_drop_threshold(drop_p);
    const float scale = 1.f / (1.f - drop_p);
    hipLaunchKernelGGL(pool_swap_tokens_bwd_kernel, dim3(3 * S * 8 + 1, B), dim3(256), 0, st, dtokens, pm, dgemb, S, H, C,
                       thr, scale, seed, seed_off, g_ds6g_salt);
    DS6G_LAUNCH_CHECK();
    const size_t tc = (size_t)(3 * S * HW + 2) * C;
    hipLaunchKernelGGL(pos_grad_kernel, dim3((unsigned)((tc / 4 + 255) / 256)), dim3(256), 0, st, dtokens, dpos_emb, B, tc,
                       thr, scale, seed, seed_off, g_ds6g_salt, accumulate_dpos ? 1 : 0);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_token_unpack_fwd(const float* tokens, float* image, float* lidar, float* radar, float* gps, int B, int S, int C,
                          void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(tokens && image && lidar && radar && gps && tok_dims_ok(B, S, C));
    DS6G_CHECK_ARG(al16(tokens) && al16(image) && al16(lidar) && al16(radar) && al16(gps));
    Maps maps{{image, lidar, radar}};
    hipLaunchKernelGGL(tokens_to_maps_kernel, dim3(3 * S * (C / TC) + 1, B), dim3(256), 0, (hipStream_t)stream, tokens, maps,
                       gps, S, C, 0, 0u, 1.f, (uint64_t)0, (uint64_t)0, (const uint64_t*)nullptr);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_token_unpack_bwd(const float* dimage, const float* dlidar, const float* dradar, const float* dgps, float* dtokens,
                          int B, int S, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dimage && dlidar && dradar && dgps && dtokens && tok_dims_ok(B, S, C));
    DS6G_CHECK_ARG(al16(dimage) && al16(dlidar) && al16(dradar) && al16(dgps) && al16(dtokens));
    Maps maps{{const_cast<float*>(dimage), const_cast<float*>(dlidar), const_cast<float*>(dradar)}};
    hipLaunchKernelGGL(maps_to_tokens_kernel, dim3(3 * S * (C / TC) + 1, B), dim3(256), 0, (hipStream_t)stream, maps, dgps,
                       (const float*)nullptr, dtokens, S, C, 0, 0u, 1.f, (uint64_t)0, (uint64_t)0, (const uint64_t*)nullptr);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

}  // extern "C"
