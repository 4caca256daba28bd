// The bi-branch Mamba fusion stage's operators that are neither a GEMM nor part of the Mamba layer (reference call sites
// mambafuser_seq.py:79,94 ln1 = LayerNorm((T, C)); :100-107 the gate; :200-214 the channel-swapping token pack; :219-231 the
// unpack).  The sample LayerNorm, the gate and the pool-swap pack are templates on the storage type of their wide operands
// (fp32, or bf16 / f16 behind the ds6g_h16_* entry points: 16-byte pieces, fp32 arithmetic, one rounding per stored element);
// the NCHW pack / unpack of the module form are fp32 only:
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

constexpr int LN_CHUNK = 2048;     // elements per workgroup of the statistics / apply passes (256 threads x 2 float4, or x 8 16-bit)
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

// ---- one 16-byte piece of a wide operand ----------------------------------------------------------------------------------
// T is the storage type of a kernel's wide operands: float behind the fp32 entry points, __bf16 / _Float16 behind the
// ds6g_h16_* ones.  A thread moves 16 bytes of such an operand at a time: one float4, or 8 elements of a 16-bit type, held as
// Pc<T>::Q float4 quads.  All arithmetic is on the quads, in fp32; a 16-bit store rounds once (RNE).  With T = float every
// loop over the quads has one trip and the kernels are the fp32 kernels they were.
template <typename T> struct Pc {
    static constexpr int N = 16 / (int)sizeof(T);   // elements per piece
    static constexpr int Q = N / 4;                 // float4 quads per piece
    f32x4 q[Q];
    __device__ __forceinline__ void set(int j, float v) { q[j >> 2][j & 3] = v; }
    __device__ __forceinline__ float operator[](int j) const { return q[j >> 2][j & 3]; }
};
__device__ __forceinline__ Pc<float> ldp(const float* p) { return Pc<float>{{ld4(p)}}; }
__device__ __forceinline__ void stp(float* p, const Pc<float>& v) { st4(p, v.q[0]); }
template <typename H>
__device__ __forceinline__ Pc<H> ldp(const H* p) {
    const typename H16<H>::x8 t = *reinterpret_cast<const typename H16<H>::x8*>(p);
    return Pc<H>{{f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]},
                  f32x4{(float)t[4], (float)t[5], (float)t[6], (float)t[7]}}};
}
template <typename H>
__device__ __forceinline__ void stp(H* p, const Pc<H>& v) {
    typename H16<H>::x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (H)v[e];
    *reinterpret_cast<typename H16<H>::x8*>(p) = t;
}
// the piece's worth of an fp32 operand (a parameter, a parameter gradient) beside a T operand
template <typename T>
__device__ __forceinline__ Pc<T> ldf(const float* p) {
    Pc<T> v;
#pragma unroll
    for (int k = 0; k < Pc<T>::Q; ++k) v.q[k] = ld4(p + k * 4);
    return v;
}
template <typename T>
__device__ __forceinline__ void stf(float* p, const Pc<T>& v) {
#pragma unroll
    for (int k = 0; k < Pc<T>::Q; ++k) st4(p + k * 4, v.q[k]);
}
template <typename T>
__device__ __forceinline__ Pc<T> zerop() {
    Pc<T> v;
#pragma unroll
    for (int k = 0; k < Pc<T>::Q; ++k) v.q[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    return v;
}

// ---- sample LayerNorm ------------------------------------------------------------------------------------------------
// statistics pass: workgroup (chunk, b) -> part[b][chunk] = (mean of the chunk, sum of squared deviations from THAT mean).
// The chunk stays in registers between the two sums, so the variance is never a difference of two large numbers.  A 16-bit
// chunk is widened as it is loaded: the statistics are those of the stored values.
template <typename T>
__global__ __launch_bounds__(256) void sln_stats_kernel(const T* __restrict__ x, size_t n, double* __restrict__ part) {
    constexpr int N = Pc<T>::N, Q = Pc<T>::Q, K = LN_CHUNK / (256 * N);   // pieces per thread: 2 (fp32), 1 (16-bit)
    __shared__ double red[4];
    const int chunk = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t c0 = (size_t)chunk * LN_CHUNK;
    const int len = (int)min((size_t)LN_CHUNK, n - c0);
    const T* xs = x + (size_t)b * n + c0;
    Pc<T> v[K];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = (k * 256 + tid) * N;
        v[k] = i < len ? ldp(xs + i) : zerop<T>();
#pragma unroll
        for (int u = 0; u < Q; ++u) s += (v[k].q[u][0] + v[k].q[u][1]) + (v[k].q[u][2] + v[k].q[u][3]);
    }
    const double mu = block_sum_d((double)s, red) / (double)len;
    const float muf = (float)mu;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = (k * 256 + tid) * N;
        if (i < len) {
#pragma unroll
            for (int j = 0; j < N; ++j) { const float d = v[k][j] - muf; q = fmaf(d, d, q); }
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

template <typename T>
__global__ __launch_bounds__(256) void sln_apply_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, T* __restrict__ y, size_t n) {
    constexpr int N = Pc<T>::N, K = LN_CHUNK / (256 * N);
    const int b = blockIdx.y;
    const float mu = mean[b], rs = rstd[b];
    const size_t c0 = (size_t)blockIdx.x * LN_CHUNK;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const size_t i = c0 + (size_t)(k * 256 + threadIdx.x) * N;
        if (i < n) {
            const Pc<T> xv = ldp(x + (size_t)b * n + i), g = ldf<T>(gamma + i), bb = ldf<T>(beta + i);
            Pc<T> o;
#pragma unroll
            for (int j = 0; j < N; ++j) o.set(j, fmaf((xv[j] - mu) * rs, g[j], bb[j]));
            stp(y + (size_t)b * n + i, o);
        }
    }
}

// backward, batch-loop pass: a thread owns one piece of consecutive columns of the sample (4 on fp32, 8 on 16-bit storage:
// a workgroup covers 256 pieces) and walks b = 0 .. B - 1 in order: dgamma / dbeta are complete in its registers, the two
// sample sums (g = dy gamma; sum g, sum g xhat) leave as one partial per (b, wave): part[b][blk * 4 + wave] = (sum g,
// sum g xhat)
template <typename T>
__global__ __launch_bounds__(256) void sln_bwd_cols_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, double* __restrict__ part, int B,
                                                           size_t n, int accumulate) {
    constexpr int N = Pc<T>::N, Q = Pc<T>::Q;
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * N;
    const bool on = i < n;
    const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), nslot = gridDim.x * 4;
    const Pc<T> zero = zerop<T>();
    const Pc<T> g = on ? ldf<T>(gamma + i) : zero;
    Pc<T> dg = zero, db = zero;
    for (int b = 0; b < B; ++b) {
        const float mu = mean[b], rs = rstd[b];
        const Pc<T> d = on ? ldp(dy + (size_t)b * n + i) : zero;
        const Pc<T> xv = on ? ldp(x + (size_t)b * n + i) : zero;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float xh = on ? (xv[j] - mu) * rs : 0.f;
            const float gj = d[j] * g[j];
            dg.set(j, fmaf(d[j], xh, dg[j]));
            db.set(j, db[j] + d[j]);
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
        if (accumulate) {
            const Pc<T> og = ldf<T>(dgamma + i), ob = ldf<T>(dbeta + i);
#pragma unroll
            for (int k = 0; k < Q; ++k) { dg.q[k] += og.q[k]; db.q[k] += ob.q[k]; }
        }
        stf<T>(dgamma + i, dg);
        stf<T>(dbeta + i, db);
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
template <typename T>
__global__ __launch_bounds__(256) void sln_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                         const float* __restrict__ gamma, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ coef,
                                                         T* __restrict__ dx, size_t n) {
    constexpr int N = Pc<T>::N, K = LN_CHUNK / (256 * N);
    const int b = blockIdx.y;
    const float mu = mean[b], rs = rstd[b], c1 = coef[b * 2], c2 = coef[b * 2 + 1];
    const size_t c0 = (size_t)blockIdx.x * LN_CHUNK;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const size_t i = c0 + (size_t)(k * 256 + threadIdx.x) * N;
        if (i < n) {
            const Pc<T> d = ldp(dy + (size_t)b * n + i), xv = ldp(x + (size_t)b * n + i), g = ldf<T>(gamma + i);
            Pc<T> o;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float xh = (xv[j] - mu) * rs;
                o.set(j, rs * ((d[j] * g[j] - c1) - xh * c2));
            }
            stp(dx + (size_t)b * n + i, o);
        }
    }
}

// ---- bi-branch gate --------------------------------------------------------------------------------------------------
// 16-bit storage: all seven streams are T, the arithmetic fp32 with one rounding per output; the LeakyReLU slope is decided
// on the stored f2 (its widened value), so forward and backward agree on the side of the kink.
__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.2f * v; }

template <typename T>
__global__ __launch_bounds__(256) void gate_fwd_kernel(const T* __restrict__ fm, int ld_fm, const T* __restrict__ bm,
                                                       int ld_bm, const T* __restrict__ f2, int ld_f2,
                                                       T* __restrict__ out, int ld_out, int B, int L, int C) {
    constexpr int N = Pc<T>::N;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int q4 = C / N;
    if (i >= (size_t)B * L * q4) return;
    const size_t row = i / q4;
    const int c = (int)(i % q4) * N;
    const size_t b = row / L;
    const size_t rrow = b * L + (L - 1 - (row - b * L));
    const Pc<T> a = ldp(fm + row * ld_fm + c), m = ldp(bm + rrow * ld_bm + c), f = ldp(f2 + rrow * ld_f2 + c);
    Pc<T> o;
#pragma unroll
    for (int j = 0; j < N; ++j) o.set(j, m[j] * (leaky(f[j]) + a[j]));
    stp(out + row * ld_out + c, o);
}

// indexed by the row r of bmN / f2N (their natural order); the matching output row is t = L - 1 - r
template <typename T>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const T* __restrict__ dout, int ld_do, const T* __restrict__ fm,
                                                       int ld_fm, const T* __restrict__ bm, int ld_bm,
                                                       const T* __restrict__ f2, int ld_f2, T* __restrict__ dfm,
                                                       int ld_dfm, T* __restrict__ dbm, int ld_dbm,
                                                       T* __restrict__ df2, int ld_df2, int B, int L, int C) {
    constexpr int N = Pc<T>::N;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int q4 = C / N;
    if (i >= (size_t)B * L * q4) return;
    const size_t rrow = i / q4;
    const int c = (int)(i % q4) * N;
    const size_t b = rrow / L;
    const size_t row = b * L + (L - 1 - (rrow - b * L));
    const Pc<T> g = ldp(dout + row * ld_do + c), a = ldp(fm + row * ld_fm + c), m = ldp(bm + rrow * ld_bm + c),
                f = ldp(f2 + rrow * ld_f2 + c);
    Pc<T> oa, om, of;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float gm = g[j] * m[j];
        oa.set(j, gm);
        om.set(j, g[j] * (leaky(f[j]) + a[j]));
        of.set(j, f[j] > 0.f ? gm : 0.2f * gm);
    }
    stp(dfm + row * ld_dfm + c, oa);
    stp(dbm + rrow * ld_dbm + c, om);
    stp(df2 + rrow * ld_df2 + c, of);
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

// drop4 on every quad of a piece whose first element has counter ctr
template <typename T>
__device__ __forceinline__ Pc<T> dropp(Pc<T> v, uint64_t seed, uint64_t ctr, uint32_t thr, float scale) {
#pragma unroll
    for (int k = 0; k < Pc<T>::Q; ++k) v.q[k] = drop4(v.q[k], seed, ctr + k * 4, thr, scale);
    return v;
}

// dpos[i] = sum over b, in index order, of the masked token gradient (dtok in the storage type T, the sum and dpos fp32)
template <typename T>
__global__ __launch_bounds__(256) void pos_grad_kernel(const T* __restrict__ dtok, float* __restrict__ dpos, int B,
                                                       size_t tc, uint32_t thr, float scale, uint64_t seed,
                                                       uint64_t seed_off_in, const uint64_t* __restrict__ salt,
                                                       int accumulate) {
    constexpr int N = Pc<T>::N, Q = Pc<T>::Q;
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * N;
    if (i >= tc) return;
    Pc<T> acc = zerop<T>();
    for (int b = 0; b < B; ++b) {
        const size_t o = (size_t)b * tc + i;
        const Pc<T> d = dropp(ldp(dtok + o), seed, seed_off + o, thr, scale);
#pragma unroll
        for (int k = 0; k < Q; ++k) acc.q[k] += d.q[k];
    }
    if (accumulate) {
        const Pc<T> old = ldf<T>(dpos + i);
#pragma unroll
        for (int k = 0; k < Q; ++k) acc.q[k] += old.q[k];
    }
    stf<T>(dpos + i, acc);
}

// ---- NHWC token pack of the model walk --------------------------------------------------------------------------------
// The walk keeps the three modality maps NHWC [B*S][H][H][C] at full resolution, so the pack pools as it swaps:
//   tokens[b][(m S + f) 64 + ph 8 + pw][c] = dropout(pos + mean over window (ph, pw) of map_q[b S + f][.][.][c]),
//   q = (m + seg(c)) % 3; seen from the SOURCE map q, channel c goes to the token rows of modality (q - seg(c)) mod 3.
// Workgroup = (sample b, source map q, frame f, row ph of 8 windows), or the sample's two gps rows (blockIdx.x ==
// gridDim.x - 1).  A pooled float4 is computed once and stored to the destination row of its segment; the two float4 groups
// per row that straddle a segment cut (C/3 and 2 (C/3) are never multiples of 4 here) go element by element.
// 16-bit storage (T = __bf16 / _Float16): the maps, the tokens and their gradients are T; gemb, pos_emb and their gradients
// fp32.  A thread moves one 16-byte piece (8 channels); the pixel sum, the 1 / k^2 scale, the pos_emb add and the dropout
// scale are fp32, rounded once at the store.  C/3 and 2 (C/3) are no multiples of 8 either, so again exactly two pieces per
// window straddle a cut and go element by element.  The backward's LDS tile stays fp32: g / k^2 meets dfeat_in unrounded.
constexpr int PST_CMAX = 512;      // widest map: the backward keeps 8 x C masked token gradients in LDS

template <typename T> struct PoolMaps { const T* in[3]; T* out[3]; };

__device__ __forceinline__ int swap_seg(int c, int s1, int s2) { return c < s1 ? 0 : (c < s2 ? 1 : 2); }
// token row (inside the sample) that channel segment `sg` of source map q pairs with, at frame f and window hw
__device__ __forceinline__ int swap_row(int q, int sg, int S, int f, int hw) {
    const int m = q - sg;
    return ((m < 0 ? m + 3 : m) * S + f) * HW + hw;
}

template <typename T>
__global__ __launch_bounds__(256) void pool_swap_tokens_fwd_kernel(const PoolMaps<T> maps, const float* __restrict__ gemb,
                                                                   const float* __restrict__ pos, T* __restrict__ tok,
                                                                   int S, int H, int C, uint32_t thr, float scale,
                                                                   uint64_t seed, uint64_t seed_off_in,
                                                                   const uint64_t* __restrict__ salt) {
    constexpr int N = Pc<T>::N, Q = Pc<T>::Q;
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const int b = blockIdx.y, tid = threadIdx.x;
    const int T_ = 3 * S * HW + 2;
    if ((int)blockIdx.x == 3 * S * 8) {     // the gps rows
        for (int i = tid * N; i < 2 * C; i += 256 * N) {
            const size_t o = ((size_t)b * T_ + (T_ - 2)) * C + i;
            Pc<T> v = ldf<T>(gemb + (size_t)b * 2 * C + i);
            const Pc<T> pe = ldf<T>(pos + (size_t)(T_ - 2) * C + i);
#pragma unroll
            for (int u = 0; u < Q; ++u) v.q[u] = v.q[u] + pe.q[u];
            stp(tok + o, dropp(v, seed, seed_off + o, thr, scale));
        }
        return;
    }
    const int ph = blockIdx.x & 7, qf = blockIdx.x >> 3;
    const int q = qf / S, f = qf - q * S;
    const int k = H >> 3, cg = C / N;
    const int s1 = C / 3, s2 = s1 * 2;
    const float inv = 1.0f / (float)(k * k);
    const T* feat = maps.in[q] + ((size_t)b * S + f) * H * H * C;
    for (int it = tid; it < 8 * cg; it += 256) {
        const int pw = it / cg, c4 = (it - pw * cg) * N;
        Pc<T> s = zerop<T>();
        for (int r = 0; r < k; ++r)
            for (int u = 0; u < k; ++u) {
                const Pc<T> px = ldp(feat + ((size_t)(ph * k + r) * H + pw * k + u) * C + c4);
#pragma unroll
                for (int e = 0; e < Q; ++e) s.q[e] += px.q[e];
            }
#pragma unroll
        for (int e = 0; e < Q; ++e) s.q[e] *= inv;
        const int hw = ph * 8 + pw;
        const int g0 = swap_seg(c4, s1, s2), g3 = swap_seg(c4 + N - 1, s1, s2);
        if (g0 == g3) {
            const int row = swap_row(q, g0, S, f, hw);
            const size_t o = ((size_t)b * T_ + row) * C + c4;
            const Pc<T> pe = ldf<T>(pos + (size_t)row * C + c4);
#pragma unroll
            for (int e = 0; e < Q; ++e) s.q[e] = s.q[e] + pe.q[e];
            stp(tok + o, dropp(s, seed, seed_off + o, thr, scale));
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int row = swap_row(q, swap_seg(c4 + j, s1, s2), S, f, hw);
                const size_t o = ((size_t)b * T_ + row) * C + c4 + j;
                float v = s[j] + pos[(size_t)row * C + c4 + j];
                if (thr) v = ds6g_keep(seed, seed_off + o, thr) ? v * scale : 0.f;
                tok[o] = (T)v;
            }
        }
    }
}

// dfeat_q = dfeat_in_q + (masked token gradient of the window) / k^2, dgemb = the masked gps-row gradient.  Same workgroups
// as the forward: the 8 x C masked, scaled gradients of the row of windows are gathered into LDS through the inverse swap,
// then spread over the k pixel rows x H pixels the windows cover (in == out is allowed: an element is read, then written,
// by one thread).
template <typename T>
__global__ __launch_bounds__(256) void pool_swap_tokens_bwd_kernel(const T* __restrict__ dtok, const PoolMaps<T> maps,
                                                                   float* __restrict__ dgemb, int S, int H, int C,
                                                                   uint32_t thr, float scale, uint64_t seed,
                                                                   uint64_t seed_off_in, const uint64_t* __restrict__ salt) {
    constexpr int N = Pc<T>::N, Q = Pc<T>::Q;
    __shared__ f32x4 gs[8 * PST_CMAX / 4];
    const uint64_t seed_off = seed_off_in + ((salt && thr) ? *salt : (uint64_t)0);
    const int b = blockIdx.y, tid = threadIdx.x;
    const int T_ = 3 * S * HW + 2;
    if ((int)blockIdx.x == 3 * S * 8) {
        for (int i = tid * N; i < 2 * C; i += 256 * N) {
            const size_t o = ((size_t)b * T_ + (T_ - 2)) * C + i;
            stf<T>(dgemb + (size_t)b * 2 * C + i, dropp(ldp(dtok + o), seed, seed_off + o, thr, scale));
        }
        return;
    }
    const int ph = blockIdx.x & 7, qf = blockIdx.x >> 3;
    const int q = qf / S, f = qf - q * S;
    const int k = H >> 3, cg = C / N;
    const int s1 = C / 3, s2 = s1 * 2;
    const float inv = 1.0f / (float)(k * k);
    for (int it = tid; it < 8 * cg; it += 256) {
        const int pw = it / cg, c4 = (it - pw * cg) * N;
        const int hw = ph * 8 + pw;
        const int g0 = swap_seg(c4, s1, s2), g3 = swap_seg(c4 + N - 1, s1, s2);
        Pc<T> v;
        if (g0 == g3) {
            const size_t o = ((size_t)b * T_ + swap_row(q, g0, S, f, hw)) * C + c4;
            v = dropp(ldp(dtok + o), seed, seed_off + o, thr, scale);
        } else {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const size_t o = ((size_t)b * T_ + swap_row(q, swap_seg(c4 + j, s1, s2), S, f, hw)) * C + c4 + j;
                const float d = (float)dtok[o];
                v.set(j, thr ? (ds6g_keep(seed, seed_off + o, thr) ? d * scale : 0.f) : d);
            }
        }
#pragma unroll
        for (int e = 0; e < Q; ++e) gs[it * Q + e] = v.q[e] * inv;
    }
    __syncthreads();
    const size_t base = (((size_t)b * S + f) * H + (size_t)ph * k) * H * C;   // k full pixel rows: k * H * C contiguous elements
    const T* din = maps.in[q];
    T* dout = maps.out[q];
    const int n4 = k * H * cg;
    for (int it = tid; it < n4; it += 256) {
        const int c4i = it % cg, w = (it / cg) % H;
        Pc<T> v;
#pragma unroll
        for (int e = 0; e < Q; ++e) v.q[e] = gs[((w / k) * cg + c4i) * Q + e];
        const size_t o = base + (size_t)it * N;
        if (din) {
            const Pc<T> old = ldp(din + o);
#pragma unroll
            for (int e = 0; e < Q; ++e) v.q[e] += old.q[e];
        }
        stp(dout + o, v);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// row stride of an operand stored as T, in elements: whole 16-byte pieces (4 floats, 8 elements of a 16-bit type)
template <typename T> inline bool ld_ok(int ld, int width) { return ld >= width && ld % Pc<T>::N == 0; }
template <typename T> inline bool sln_dims_ok(int B, long n) {
    return B > 0 && B <= 65535 && n > 0 && n % Pc<T>::N == 0 && n <= (1L << 30);
}
inline int sln_chunks(long n) { return (int)((n + LN_CHUNK - 1) / LN_CHUNK); }
// workgroups of the backward's batch-loop pass: 256 pieces each, LN_COLS floats or twice as many 16-bit elements
template <typename T> inline int sln_colblocks(long n) {
    const long cols = (long)LN_COLS / 4 * Pc<T>::N;
    return (int)((n + cols - 1) / cols);
}
template <typename T> inline bool gate_dims_ok(int B, int L, int C) {
    // the grid: one thread per piece
    return B > 0 && L > 0 && C > 0 && C % Pc<T>::N == 0 && C <= (1 << 16) && (long)B * L < (1L << 31) / 64 &&
           (long)B * L * (C / Pc<T>::N) < (1L << 31) * 128;
}
inline bool tok_dims_ok(int B, int S, int C) {
    return B > 0 && B <= 65535 && S > 0 && S <= 4096 && C > 0 && C % TC == 0 && C <= 4096;
}
template <typename T> inline bool pool_dims_ok(int B, int S, int H, int C) {
    return B > 0 && B <= 65535 && S > 0 && S <= 4096 && H >= 8 && H <= 64 && H % 8 == 0 && C >= Pc<T>::N &&
           C % Pc<T>::N == 0 && C <= PST_CMAX;
}

}  // namespace

extern "C" {

size_t ds6g_sample_layernorm_workspace_bytes(int B, long n) {
    if (B <= 0 || n <= 0) return 0;
    // forward: (mean, M2) per chunk; backward: two sums per (column block, wave) + two coefficients per sample.  Sized for
    // fp32 storage; the 16-bit instances run the same chunks and half as many column blocks
    const size_t fwd = (size_t)B * sln_chunks(n) * 2 * sizeof(double);
    const size_t bwd = (size_t)B * sln_colblocks<float>(n) * 4 * 2 * sizeof(double) + (size_t)B * 2 * sizeof(float);
    return fwd > bwd ? fwd : bwd;
}

// The sample LayerNorm, the gate and the pool-swap pack over the storage type T of their wide operands: float behind the
// fp32 entry points, __bf16 / _Float16 behind the ds6g_h16_* ones.  Same checks, same launches, same workspace for every T.
extern "C++" template <typename T>
static int sample_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                int B, long n, float eps, void* ws, size_t ws_bytes, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(x && gamma && beta && y && mean && rstd && ws && sln_dims_ok<T>(B, n) && eps > 0.f);
    DS6G_CHECK_ARG(al16(x) && al16(gamma) && al16(beta) && al16(y) && al16(ws));
    DS6G_CHECK_WS(ws_bytes >= ds6g_sample_layernorm_workspace_bytes(B, n));
    hipStream_t st = (hipStream_t)stream;
    const int nchunk = sln_chunks(n);
    double* part = (double*)ws;
    hipLaunchKernelGGL(sln_stats_kernel<T>, dim3(nchunk, B), dim3(256), 0, st, (const T*)x, (size_t)n, part);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_stats_finalize_kernel, dim3(B), dim3(256), 0, st, (const double*)part, nchunk, (size_t)n, eps, mean,
                       rstd);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_apply_kernel<T>, dim3(nchunk, B), dim3(256), 0, st, (const T*)x, gamma, beta, (const float*)mean,
                       (const float*)rstd, (T*)y, (size_t)n);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_sample_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                              int B, long n, float eps, void* ws, size_t ws_bytes, void* stream) {
    return sample_layernorm_fwd<float>(x, gamma, beta, y, mean, rstd, B, n, eps, ws, ws_bytes, stream);
}
int ds6g_h16_sample_layernorm_fwd(int st16, const void* x, const float* gamma, const float* beta, void* y, float* mean,
                                  float* rstd, int B, long n, float eps, void* ws, size_t ws_bytes, void* stream) {
    DS6G_RETURN_H16(st16, sample_layernorm_fwd, x, gamma, beta, y, mean, rstd, B, n, eps, ws, ws_bytes, stream);
}

extern "C++" template <typename T>
static int sample_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                                void* dx, float* dgamma, float* dbeta, int B, long n, int accumulate_param_grads, void* ws,
                                size_t ws_bytes, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dy && x && mean && rstd && gamma && dx && dgamma && dbeta && ws && sln_dims_ok<T>(B, n));
    DS6G_CHECK_ARG(al16(dy) && al16(x) && al16(gamma) && al16(dx) && al16(dgamma) && al16(dbeta) && al16(ws));
    DS6G_CHECK_WS(ws_bytes >= ds6g_sample_layernorm_workspace_bytes(B, n));
    hipStream_t st = (hipStream_t)stream;
    const int nblk = sln_colblocks<T>(n);
    double* part = (double*)ws;
    float* coef = (float*)(part + (size_t)B * nblk * 4 * 2);
    hipLaunchKernelGGL(sln_bwd_cols_kernel<T>, dim3(nblk), dim3(256), 0, st, (const T*)dy, (const T*)x, gamma, mean, rstd,
                       dgamma, dbeta, part, B, (size_t)n, accumulate_param_grads ? 1 : 0);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_bwd_finalize_kernel, dim3(B), dim3(256), 0, st, (const double*)part, nblk * 4, (size_t)n, coef);
    DS6G_LAUNCH_CHECK();
    hipLaunchKernelGGL(sln_bwd_dx_kernel<T>, dim3(sln_chunks(n), B), dim3(256), 0, st, (const T*)dy, (const T*)x, gamma, mean,
                       rstd, (const float*)coef, (T*)dx, (size_t)n);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_sample_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                              float* dx, float* dgamma, float* dbeta, int B, long n, int accumulate_param_grads, void* ws,
                              size_t ws_bytes, void* stream) {
    return sample_layernorm_bwd<float>(dy, x, mean, rstd, gamma, dx, dgamma, dbeta, B, n, accumulate_param_grads, ws, ws_bytes,
                                       stream);
}
int ds6g_h16_sample_layernorm_bwd(int st16, const void* dy, const void* x, const float* mean, const float* rstd,
                                  const float* gamma, void* dx, float* dgamma, float* dbeta, int B, long n,
                                  int accumulate_param_grads, void* ws, size_t ws_bytes, void* stream) {
    DS6G_RETURN_H16(st16, sample_layernorm_bwd, dy, x, mean, rstd, gamma, dx, dgamma, dbeta, B, n, accumulate_param_grads, ws,
                    ws_bytes, stream);
}

extern "C++" template <typename T>
static int bimamba_gate_fwd(const void* fm, int ld_fm, const void* bm, int ld_bm, const void* f2, int ld_f2, void* out,
                            int ld_out, int B, int L, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(fm && bm && f2 && out && gate_dims_ok<T>(B, L, C));
    DS6G_CHECK_ARG(ld_ok<T>(ld_fm, C) && ld_ok<T>(ld_bm, C) && ld_ok<T>(ld_f2, C) && ld_ok<T>(ld_out, C));
    DS6G_CHECK_ARG(al16(fm) && al16(bm) && al16(f2) && al16(out));
    const size_t nq = (size_t)B * L * (C / Pc<T>::N);
    hipLaunchKernelGGL(gate_fwd_kernel<T>, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)fm, ld_fm, (const T*)bm, ld_bm, (const T*)f2, ld_f2, (T*)out, ld_out, B, L, C);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_bimamba_gate_fwd(const float* fm, int ld_fm, const float* bm, int ld_bm, const float* f2, int ld_f2, float* out,
                          int ld_out, int B, int L, int C, void* stream) {
    return bimamba_gate_fwd<float>(fm, ld_fm, bm, ld_bm, f2, ld_f2, out, ld_out, B, L, C, stream);
}
int ds6g_h16_bimamba_gate_fwd(int st16, const void* fm, int ld_fm, const void* bm, int ld_bm, const void* f2, int ld_f2,
                              void* out, int ld_out, int B, int L, int C, void* stream) {
    DS6G_RETURN_H16(st16, bimamba_gate_fwd, fm, ld_fm, bm, ld_bm, f2, ld_f2, out, ld_out, B, L, C, stream);
}

extern "C++" template <typename T>
static int bimamba_gate_bwd(const void* dout, int ld_dout, const void* fm, int ld_fm, const void* bm, int ld_bm,
                            const void* f2, int ld_f2, void* dfm, int ld_dfm, void* dbm, int ld_dbm, void* df2, int ld_df2,
                            int B, int L, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dout && fm && bm && f2 && dfm && dbm && df2 && gate_dims_ok<T>(B, L, C));
    DS6G_CHECK_ARG(ld_ok<T>(ld_dout, C) && ld_ok<T>(ld_fm, C) && ld_ok<T>(ld_bm, C) && ld_ok<T>(ld_f2, C) &&
                   ld_ok<T>(ld_dfm, C) && ld_ok<T>(ld_dbm, C) && ld_ok<T>(ld_df2, C));
    DS6G_CHECK_ARG(al16(dout) && al16(fm) && al16(bm) && al16(f2) && al16(dfm) && al16(dbm) && al16(df2));
    const size_t nq = (size_t)B * L * (C / Pc<T>::N);
    hipLaunchKernelGGL(gate_bwd_kernel<T>, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const T*)dout, ld_dout, (const T*)fm, ld_fm, (const T*)bm, ld_bm, (const T*)f2, ld_f2, (T*)dfm, ld_dfm,
                       (T*)dbm, ld_dbm, (T*)df2, ld_df2, B, L, C);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_bimamba_gate_bwd(const float* dout, int ld_dout, const float* fm, int ld_fm, const float* bm, int ld_bm,
                          const float* f2, int ld_f2, float* dfm, int ld_dfm, float* dbm, int ld_dbm, float* df2, int ld_df2,
                          int B, int L, int C, void* stream) {
    return bimamba_gate_bwd<float>(dout, ld_dout, fm, ld_fm, bm, ld_bm, f2, ld_f2, dfm, ld_dfm, dbm, ld_dbm, df2, ld_df2, B, L,
                                   C, stream);
}
int ds6g_h16_bimamba_gate_bwd(int st16, const void* dout, int ld_dout, const void* fm, int ld_fm, const void* bm, int ld_bm,
                              const void* f2, int ld_f2, void* dfm, int ld_dfm, void* dbm, int ld_dbm, void* df2, int ld_df2,
                              int B, int L, int C, void* stream) {
    DS6G_RETURN_H16(st16, bimamba_gate_bwd, dout, ld_dout, fm, ld_fm, bm, ld_bm, f2, ld_f2, dfm, ld_dfm, dbm, ld_dbm, df2,
                    ld_df2, B, L, C, stream);
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
    hipLaunchKernelGGL(pos_grad_kernel<float>, dim3((unsigned)((tc / 4 + 255) / 256)), dim3(256), 0, st, dtokens, dpos_emb, B,
                       tc, thr, scale, seed, seed_off, g_ds6g_salt, 0);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

extern "C++" template <typename T>
static int pool_swap_tokens_fwd(const ds6g_map_desc* maps, const float* gemb, const float* pos_emb, void* tokens, int B, int S,
                                int H, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(maps && gemb && pos_emb && tokens && pool_dims_ok<T>(B, S, H, C));
    DS6G_CHECK_ARG(al16(gemb) && al16(pos_emb) && al16(tokens) && drop_p >= 0.f && drop_p < 1.f);
    PoolMaps<T> pm{};
    for (int m = 0; m < 3; ++m) {
        DS6G_CHECK_ARG(maps[m].in && al16(maps[m].in) && maps[m].frames_per_sample == S && maps[m].mod_off == m * S * HW);
        pm.in[m] = (const T*)maps[m].in;
    }
    hipLaunchKernelGGL(pool_swap_tokens_fwd_kernel<T>, dim3(3 * S * 8 + 1, B), dim3(256), 0, (hipStream_t)stream, pm, gemb,
                       pos_emb, (T*)tokens, S, H, C, ds6g_drop_threshold(drop_p), 1.f / (1.f - drop_p), seed, seed_off,
                       g_ds6g_salt);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_pool_swap_tokens_fwd(const ds6g_map_desc* maps, const float* gemb, const float* pos_emb, float* tokens, int B, int S,
                              int H, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream) {
    return pool_swap_tokens_fwd<float>(maps, gemb, pos_emb, tokens, B, S, H, C, drop_p, seed, seed_off, stream);
}
int ds6g_h16_pool_swap_tokens_fwd(int st16, const ds6g_map_desc* maps, const float* gemb, const float* pos_emb, void* tokens,
                                  int B, int S, int H, int C, float drop_p, uint64_t seed, uint64_t seed_off, void* stream) {
    DS6G_RETURN_H16(st16, pool_swap_tokens_fwd, maps, gemb, pos_emb, tokens, B, S, H, C, drop_p, seed, seed_off, stream);
}

extern "C++" template <typename T>
static int pool_swap_tokens_bwd(const ds6g_map_desc* maps, const void* dtokens, float* dgemb, float* dpos_emb,
                                int accumulate_dpos, int B, int S, int H, int C, float drop_p, uint64_t seed,
                                uint64_t seed_off, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(maps && dtokens && dgemb && dpos_emb && pool_dims_ok<T>(B, S, H, C));
    DS6G_CHECK_ARG(al16(dtokens) && al16(dgemb) && al16(dpos_emb) && drop_p >= 0.f && drop_p < 1.f);
    PoolMaps<T> pm{};
    for (int m = 0; m < 3; ++m) {
        DS6G_CHECK_ARG(maps[m].out && al16(maps[m].out) && al16(maps[m].in) && maps[m].frames_per_sample == S &&
                       maps[m].mod_off == m * S * HW);
        pm.in[m] = (const T*)maps[m].in;
        pm.out[m] = (T*)maps[m].out;
    }
    hipStream_t st = (hipStream_t)stream;
    const uint32_t thr = ds6g_drop_threshold(drop_p);
    const float scale = 1.f / (1.f - drop_p);
    hipLaunchKernelGGL(pool_swap_tokens_bwd_kernel<T>, dim3(3 * S * 8 + 1, B), dim3(256), 0, st, (const T*)dtokens, pm, dgemb,
                       S, H, C, thr, scale, seed, seed_off, g_ds6g_salt);
    DS6G_LAUNCH_CHECK();
    const size_t tc = (size_t)(3 * S * HW + 2) * C;
    hipLaunchKernelGGL(pos_grad_kernel<T>, dim3((unsigned)((tc / Pc<T>::N + 255) / 256)), dim3(256), 0, st, (const T*)dtokens,
                       dpos_emb, B, tc, thr, scale, seed, seed_off, g_ds6g_salt, accumulate_dpos ? 1 : 0);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_pool_swap_tokens_bwd(const ds6g_map_desc* maps, const float* dtokens, float* dgemb, float* dpos_emb,
                              int accumulate_dpos, int B, int S, int H, int C, float drop_p, uint64_t seed,
                              uint64_t seed_off, void* stream) {
    return pool_swap_tokens_bwd<float>(maps, dtokens, dgemb, dpos_emb, accumulate_dpos, B, S, H, C, drop_p, seed, seed_off,
                                       stream);
}
int ds6g_h16_pool_swap_tokens_bwd(int st16, const ds6g_map_desc* maps, const void* dtokens, float* dgemb, float* dpos_emb,
                                  int accumulate_dpos, int B, int S, int H, int C, float drop_p, uint64_t seed,
                                  uint64_t seed_off, void* stream) {
    DS6G_RETURN_H16(st16, pool_swap_tokens_bwd, maps, dtokens, dgemb, dpos_emb, accumulate_dpos, B, S, H, C, drop_p, seed,
                    seed_off, stream);
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
