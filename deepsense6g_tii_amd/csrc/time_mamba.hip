// The temporal Mamba fusion head's arithmetic behind its shared Mamba layer (reference call site mambafuser_seq.py:265-282),
// fp32: for the 17 rows of a sample - 3 modalities x 5 frames of the layer's output y, then the 2 gps rows -
//   score   s[r] = max_c row[r][c] + (1 / 512) sum_c row[r][c]                (MaxPool1d(512) + AvgPool1d(512))
//   attn    a = softmax(W5 s + b5) over the 5 frames of a modality (one Linear(5, 5) shared by the three),
//           a_g = softmax(W2 s_g + b2) over the 2 gps rows
//   out[c]  = sum_m sum_t a_m[t] y_m[t][c] + sum_j a_g[j] gps[j][c]
// ONE launch forward, ONE backward.  One workgroup per sample, 512 threads: thread c owns channel c of all 17 rows in
// registers, so every global access is a coalesced 2 KB row and the weighted sum over rows is thread-local.  The 17 row
// reductions go butterfly-wise through the wave, then through an LDS table across the 8 waves in wave order; the two tiny
// linears and softmaxes are done by 4 lanes (one per softmax group) out of LDS.  No float atomics: every sum has a fixed
// order, two runs are bit-identical.  The backward leaves the 36 parameter-gradient values of a sample in a [B][36] slab
// (W5 25, b5 5, W2 4, b2 2) for ds6g_batch_sum, or for ds6g_temporal_param_grads, which delivers the sums to the four
// parameters' own gradients.  Below them: the grouped head pool that feeds the head from a model walk (ds6g_pool_rows3_*), a
// template on the storage type of the walk's maps (ds6g_h16_pool_rows3_* for bf16 / f16 maps); the head itself stays fp32.
#include "common.h"

namespace {

constexpr int TM_C = 512;          // channels == threads per workgroup
constexpr int TM_S = 5;            // frames per modality
constexpr int TM_R = 17;           // rows per sample: 3 * 5 + 2
constexpr int TM_GPS = 15;         // first gps row
constexpr int TM_W = TM_C / 64;    // waves per workgroup
constexpr int TM_NP = 36;          // parameter-gradient values per sample

// row r of sample b, channel c: y is the layer's output on the modality-major batch, row (m * B + b) * 5 + t
__device__ __forceinline__ size_t y_off(int B, int b, int r, int c) {
    const int m = r / TM_S, t = r - m * TM_S;
    return (((size_t)m * B + b) * TM_S + t) * TM_C + c;
}

__device__ __forceinline__ void load_rows(const float* __restrict__ y, const float* __restrict__ gps, size_t ld_gps, int B,
                                          int b, int c, float v[TM_R]) {
#pragma unroll
    for (int r = 0; r < TM_GPS; ++r) v[r] = y[y_off(B, b, r, c)];
#pragma unroll
    for (int j = 0; j < 2; ++j) v[TM_GPS + j] = gps[(size_t)b * ld_gps + j * TM_C + c];
}

// softmax group g = 0, 1, 2 (a modality: 5 rows from 5 g, Linear(5, 5)) or 3 (gps: 2 rows from 15, Linear(2, 2))
__device__ __forceinline__ int group_n(int g) { return g < 3 ? TM_S : 2; }

__global__ __launch_bounds__(TM_C) void time_attn_fwd_kernel(const float* __restrict__ y, const float* __restrict__ gps,
                                                             size_t ld_gps, const float* __restrict__ w5,
                                                             const float* __restrict__ b5, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, float* __restrict__ out,
                                                             float* __restrict__ attn, float* __restrict__ score,
                                                             int* __restrict__ argmax, int B) {
    __shared__ float s_max[TM_R][TM_W], s_sum[TM_R][TM_W];
    __shared__ int s_idx[TM_R][TM_W];
    __shared__ float s_score[TM_R], s_attn[TM_R];
    const int b = blockIdx.x, c = threadIdx.x, wave = c >> 6, lane = c & 63;
    float v[TM_R];
    load_rows(y, gps, ld_gps, B, b, c, v);
    // per row: (max, lowest channel holding it) and the sum, over the wave's 64 channels
#pragma unroll
    for (int r = 0; r < TM_R; ++r) {
        float mx = v[r], sm = v[r];
        int ix = c;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(mx, o, 64);
            const int oi = __shfl_xor(ix, o, 64);
            sm += __shfl_xor(sm, o, 64);
            if (ov > mx || (ov == mx && oi < ix)) { mx = ov; ix = oi; }
        }
        if (lane == 0) { s_max[r][wave] = mx; s_idx[r][wave] = ix; s_sum[r][wave] = sm; }
    }
    __syncthreads();
    if (c < TM_R) {
        // the waves hold ascending channel ranges: a strict > keeps the lowest channel of a tie.  The running maximum starts
        // at -inf, not 0: a row can be all negative.
        float mx = -INFINITY, sm = 0.f;
        int ix = 0;
#pragma unroll
        for (int w = 0; w < TM_W; ++w) {
            if (s_max[c][w] > mx) { mx = s_max[c][w]; ix = s_idx[c][w]; }
            sm += s_sum[c][w];
        }
        const float sc = mx + sm * (1.f / TM_C);
        s_score[c] = sc;
        score[(size_t)b * TM_R + c] = sc;
        argmax[(size_t)b * TM_R + c] = ix;
    }
    __syncthreads();
    if (c < 4) {
        const int n = group_n(c), base = c * TM_S;
        const float* W = c < 3 ? w5 : w2;
        const float* bias = c < 3 ? b5 : b2;
        float z[TM_S], zmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < TM_S; ++i) {
            if (i < n) {
                float acc = bias[i];
                for (int j = 0; j < n; ++j) acc = fmaf(W[i * n + j], s_score[base + j], acc);
                z[i] = acc;
                zmax = fmaxf(zmax, acc);
            }
        }
        float den = 0.f;
#pragma unroll
        for (int i = 0; i < TM_S; ++i) {
            if (i < n) { z[i] = expf(z[i] - zmax); den += z[i]; }
        }
#pragma unroll
        for (int i = 0; i < TM_S; ++i) {
            if (i < n) {
                const float a = z[i] / den;
                s_attn[base + i] = a;
                attn[(size_t)b * TM_R + base + i] = a;
            }
        }
    }
    __syncthreads();
    // the reference's order: each modality's weighted sum over its frames, then image + lidar + radar + gps
    float acc = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float f = 0.f;
#pragma unroll
        for (int i = 0; i < TM_S; ++i)
            if (i < group_n(g)) f = fmaf(s_attn[g * TM_S + i], v[g * TM_S + i], f);
        acc += f;
    }
    out[(size_t)b * TM_C + c] = acc;
}

// dy[r][c] = a[r] dout[c] + ds[r] / 512 + (c == argmax[r] ? ds[r] : 0),  ds = W^T (a (.) (da - sum a da)) per softmax group,
// da[r] = sum_c dout[c] row[r][c]
__global__ __launch_bounds__(TM_C) void time_attn_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ y,
                                                             const float* __restrict__ gps, size_t ld_gps,
                                                             const float* __restrict__ attn, const float* __restrict__ score,
                                                             const int* __restrict__ argmax, const float* __restrict__ w5,
                                                             const float* __restrict__ w2, float* __restrict__ dy,
                                                             float* __restrict__ dgps, size_t ld_dgps,
                                                             float* __restrict__ part, int B) {
    __shared__ float s_red[TM_R][TM_W];
    __shared__ float s_da[TM_R], s_attn[TM_R], s_score[TM_R], s_dz[TM_R], s_ds[TM_R];
    __shared__ int s_arg[TM_R];
    const int b = blockIdx.x, c = threadIdx.x, wave = c >> 6, lane = c & 63;
    const float g = dout[(size_t)b * TM_C + c];
    {
        float v[TM_R];
        load_rows(y, gps, ld_gps, B, b, c, v);
#pragma unroll
        for (int r = 0; r < TM_R; ++r) {
            const float p = wave_reduce_sum(g * v[r]);
            if (lane == 0) s_red[r][wave] = p;
        }
    }
    if (c < TM_R) {
        s_attn[c] = attn[(size_t)b * TM_R + c];
        s_score[c] = score[(size_t)b * TM_R + c];
        s_arg[c] = argmax[(size_t)b * TM_R + c];
    }
    __syncthreads();
    if (c < TM_R) {
        float sm = 0.f;
#pragma unroll
        for (int w = 0; w < TM_W; ++w) sm += s_red[c][w];
        s_da[c] = sm;
    }
    __syncthreads();
    if (c < 4) {
        const int n = group_n(c), base = c * TM_S;
        const float* W = c < 3 ? w5 : w2;
        float dot = 0.f;
        for (int i = 0; i < n; ++i) dot = fmaf(s_attn[base + i], s_da[base + i], dot);
        float dz[TM_S];
#pragma unroll
        for (int i = 0; i < TM_S; ++i) {
            dz[i] = i < n ? s_attn[base + i] * (s_da[base + i] - dot) : 0.f;
            if (i < n) s_dz[base + i] = dz[i];
        }
#pragma unroll
        for (int j = 0; j < TM_S; ++j) {
            if (j < n) {
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < TM_S; ++i)
                    if (i < n) acc = fmaf(W[i * n + j], dz[i], acc);
                s_ds[base + j] = acc;
            }
        }
    }
    __syncthreads();
    if (c < TM_NP) {
        // the sample's share of dW5 [5][5], db5 [5] (summed over its three modalities in index order), dW2 [2][2], db2 [2]
        float p;
        if (c < 30) {
            const int i = c < 25 ? c / TM_S : c - 25, j = c < 25 ? c - i * TM_S : -1;
            p = 0.f;
#pragma unroll
            for (int m = 0; m < 3; ++m) p += j >= 0 ? s_dz[m * TM_S + i] * s_score[m * TM_S + j] : s_dz[m * TM_S + i];
        } else if (c < 34) {
            const int i = (c - 30) >> 1, j = (c - 30) & 1;
            p = s_dz[TM_GPS + i] * s_score[TM_GPS + j];
        } else {
            p = s_dz[TM_GPS + c - 34];
        }
        part[(size_t)b * TM_NP + c] = p;
    }
#pragma unroll
    for (int r = 0; r < TM_R; ++r) {
        const float ds = s_ds[r];
        const float o = fmaf(s_attn[r], g, ds * (1.f / TM_C)) + (c == s_arg[r] ? ds : 0.f);
        if (r < TM_GPS) dy[y_off(B, b, r, c)] = o;
        else dgps[(size_t)b * ld_dgps + (r - TM_GPS) * TM_C + c] = o;
    }
}

// The sample shares of the 36 parameter-gradient values summed over b in index order (ds6g_batch_sum's arithmetic: the sum
// starts at 0, the old value is added last) and written to, or added to, the four parameters' own gradients.
struct TimeParamDst {
    float* p[4];
    int acc[4];
};

__global__ __launch_bounds__(64) void time_param_grads_kernel(const float* __restrict__ part, int B, TimeParamDst d) {
    const int c = threadIdx.x;
    if (c >= TM_NP) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[(size_t)b * TM_NP + c];
    const int k = c < 25 ? 0 : c < 30 ? 1 : c < 34 ? 2 : 3;
    const int i = c - (k == 0 ? 0 : k == 1 ? 25 : k == 2 ? 30 : 34);
    float* o = d.p[k] + i;
    if (d.acc[k]) s += *o;
    *o = s;
}

// ---- the grouped head pool: the frames of the three 8 x 8 modality maps <-> the head's modality-major rows --------------------
// rows[m * N + n][c] = mean over the 64 positions of map m's frame n.  One launch for the three maps (blockIdx.z = m), a
// thread per (frame, 4 channels): 64 coalesced 16-byte loads summed in position order - ds6g_global_pool's arithmetic.
// Both kernels are templates on the storage type T of the MAPS (feat_m; dfeat_in_m and dfeat_m): float behind
// ds6g_pool_rows3_*, __bf16 / _Float16 behind ds6g_h16_pool_rows3_* (the maps of a model walk on 16-bit storage).  rows and
// drows - the temporal head's input and its gradient - and all arithmetic are fp32 for every T.  A thread moves one 16-byte
// piece of a map: 4 floats, or 8 elements of a 16-bit type as two f32x4 halves.
template <typename T>
struct PoolRows3 {
    const T* in[3];
    T* out[3];
};

template <typename T> struct PoolPiece {
    static constexpr int SH = sizeof(T) == 4 ? 2 : 3;   // log2 of the elements per piece
    static constexpr int N = 1 << SH, NV = N / 4;
};
__device__ __forceinline__ void ld_piece(const float* p, f32x4 (&v)[1]) { v[0] = ld4(p); }
__device__ __forceinline__ void st_piece(float* p, const f32x4 (&v)[1]) { st4(p, v[0]); }
template <typename H>
__device__ __forceinline__ void ld_piece(const H* p, f32x4 (&v)[2]) {     // widening is exact
    const typename H16<H>::x8 t = *reinterpret_cast<const typename H16<H>::x8*>(p);
    v[0] = f32x4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
    v[1] = f32x4{(float)t[4], (float)t[5], (float)t[6], (float)t[7]};
}
template <typename H>
__device__ __forceinline__ void st_piece(H* p, const f32x4 (&v)[2]) {     // round to nearest even, ONE rounding per element
    typename H16<H>::x8 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) { t[e] = (H)v[0][e]; t[4 + e] = (H)v[1][e]; }
    *reinterpret_cast<typename H16<H>::x8*>(p) = t;
}

template <typename T>
__global__ __launch_bounds__(256) void pool_rows3_fwd_kernel(PoolRows3<T> g, float* __restrict__ rows, int N, int C) {
    constexpr int PN = PoolPiece<T>::N, NV = PoolPiece<T>::NV;
    const int cg = C >> PoolPiece<T>::SH;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * cg) return;
    const int m = blockIdx.z;
    const T* __restrict__ feat = g.in[m];
    const int c4 = (int)(i % cg) * PN;
    const long n = i / cg;
    f32x4 s[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < 64; ++p) {
        f32x4 v[NV];
        ld_piece(feat + (n * 64 + p) * C + c4, v);
#pragma unroll
        for (int j = 0; j < NV; ++j) s[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) st4(rows + ((long)m * N + n) * C + c4 + 4 * j, s[j] * (1.0f / 64.0f));
}

// out_m[n][p][c] = (in_m or 0) + drows[m * N + n][c] / 64: a thread per 16 bytes of a map, every element written exactly once
// (in_m may be out_m: the thread that writes an element is the one that read it, so neither pointer is __restrict__)
template <typename T>
__global__ __launch_bounds__(256) void pool_rows3_bwd_kernel(PoolRows3<T> g, const float* __restrict__ drows, int N, int C) {
    constexpr int PN = PoolPiece<T>::N, NV = PoolPiece<T>::NV;
    const int cg = C >> PoolPiece<T>::SH;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * 64 * cg) return;
    const int m = blockIdx.z;
    const int c4 = (int)(i % cg) * PN;
    const long n = i / ((long)64 * cg);
    f32x4 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = ld4(drows + ((long)m * N + n) * C + c4 + 4 * j) * (1.0f / 64.0f);
    const T* in = g.in[m];
    if (in) {
        f32x4 a[NV];
        ld_piece(in + i * PN, a);
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] += a[j];
    }
    st_piece(g.out[m] + i * PN, v);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
template <typename T>
inline bool pool_rows3_dims_ok(int N, int C) {
    constexpr int PN = PoolPiece<T>::N;
    return N >= 1 && C >= PN && C % PN == 0 && (long)N * 64 * C <= (1L << 31);
}
inline bool tm_dims_ok(int B, int S, int C) { return B >= 1 && B <= (1 << 20) && S == TM_S && C == TM_C; }
inline bool tm_ld_ok(long ld) { return ld >= 2 * TM_C && ld % 4 == 0; }

}  // namespace

extern "C" {

int ds6g_time_attn_fwd(const float* y, const float* gps, long ld_gps_sample, const float* w5, const float* b5,
                       const float* w2, const float* b2, float* out, float* attn, float* score, int* argmax, int B, int S,
                       int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(y && gps && w5 && b5 && w2 && b2 && out && attn && score && argmax);
    DS6G_CHECK_ARG(tm_dims_ok(B, S, C) && tm_ld_ok(ld_gps_sample));
    DS6G_CHECK_ARG(al16(y) && al16(gps) && al16(w5) && al16(b5) && al16(w2) && al16(b2) && al16(out) && al16(attn) &&
                   al16(score) && al16(argmax));
    hipLaunchKernelGGL(time_attn_fwd_kernel, dim3(B), dim3(TM_C), 0, (hipStream_t)stream, y, gps, (size_t)ld_gps_sample, w5,
                       b5, w2, b2, out, attn, score, argmax, B);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_time_attn_bwd(const float* dout, const float* y, const float* gps, long ld_gps_sample, const float* attn,
                       const float* score, const int* argmax, const float* w5, const float* w2, float* dy, float* dgps,
                       long ld_dgps_sample, float* dparam_part, int B, int S, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dout && y && gps && attn && score && argmax && w5 && w2 && dy && dgps && dparam_part);
    DS6G_CHECK_ARG(tm_dims_ok(B, S, C) && tm_ld_ok(ld_gps_sample) && tm_ld_ok(ld_dgps_sample));
    DS6G_CHECK_ARG(al16(dout) && al16(y) && al16(gps) && al16(attn) && al16(score) && al16(argmax) && al16(w5) && al16(w2) &&
                   al16(dy) && al16(dgps) && al16(dparam_part));
    hipLaunchKernelGGL(time_attn_bwd_kernel, dim3(B), dim3(TM_C), 0, (hipStream_t)stream, dout, y, gps,
                       (size_t)ld_gps_sample, attn, score, argmax, w5, w2, dy, dgps, (size_t)ld_dgps_sample, dparam_part, B);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_temporal_param_grads(const float* dparam_part, int B, float* dw5, int acc_w5, float* db5, int acc_b5, float* dw2,
                          int acc_w2, float* db2, int acc_b2, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dparam_part && dw5 && db5 && dw2 && db2 && B >= 1 && B <= (1 << 20));
    DS6G_CHECK_ARG(((uintptr_t)dparam_part & 3) == 0 && ((uintptr_t)dw5 & 3) == 0 && ((uintptr_t)db5 & 3) == 0 &&
                   ((uintptr_t)dw2 & 3) == 0 && ((uintptr_t)db2 & 3) == 0);
    const TimeParamDst d = {{dw5, db5, dw2, db2}, {acc_w5 != 0, acc_b5 != 0, acc_w2 != 0, acc_b2 != 0}};
    hipLaunchKernelGGL(time_param_grads_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, dparam_part, B, d);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

// The head pool over the storage type T of the maps: float behind the fp32 entry points, __bf16 / _Float16 behind the
// ds6g_h16_* ones.  Same checks and the same one launch for every T; a thread per 16-byte piece (C % 4, or C % 8 on 16-bit).
extern "C++" template <typename T>
static int pool_rows3_fwd(const void* feat0, const void* feat1, const void* feat2, float* rows, int N, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(feat0 && feat1 && feat2 && rows && pool_rows3_dims_ok<T>(N, C));
    DS6G_CHECK_ARG(al16(feat0) && al16(feat1) && al16(feat2) && al16(rows));
    const PoolRows3<T> g = {{(const T*)feat0, (const T*)feat1, (const T*)feat2}, {nullptr, nullptr, nullptr}};
    hipLaunchKernelGGL(pool_rows3_fwd_kernel<T>, dim3(cdiv((long)N * (C / PoolPiece<T>::N), 256), 1, 3), dim3(256), 0,
                       (hipStream_t)stream, g, rows, N, C);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_pool_rows3_fwd(const float* feat0, const float* feat1, const float* feat2, float* rows, int N, int C, void* stream) {
    return pool_rows3_fwd<float>(feat0, feat1, feat2, rows, N, C, stream);
}
int ds6g_h16_pool_rows3_fwd(int st16, const void* feat0, const void* feat1, const void* feat2, float* rows, int N, int C,
                            void* stream) {
    DS6G_RETURN_H16(st16, pool_rows3_fwd, feat0, feat1, feat2, rows, N, C, stream);
}

extern "C++" template <typename T>
static int pool_rows3_bwd(const float* drows, const void* dfeat_in0, const void* dfeat_in1, const void* dfeat_in2,
                          void* dfeat0, void* dfeat1, void* dfeat2, int N, int C, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(drows && dfeat0 && dfeat1 && dfeat2 && pool_rows3_dims_ok<T>(N, C));
    DS6G_CHECK_ARG(al16(drows) && al16(dfeat_in0) && al16(dfeat_in1) && al16(dfeat_in2) && al16(dfeat0) && al16(dfeat1) &&
                   al16(dfeat2));
    const PoolRows3<T> g = {{(const T*)dfeat_in0, (const T*)dfeat_in1, (const T*)dfeat_in2},
                            {(T*)dfeat0, (T*)dfeat1, (T*)dfeat2}};
    hipLaunchKernelGGL(pool_rows3_bwd_kernel<T>, dim3(cdiv((long)N * 64 * (C / PoolPiece<T>::N), 256), 1, 3), dim3(256), 0,
                       (hipStream_t)stream, g, drows, N, C);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_pool_rows3_bwd(const float* drows, const float* dfeat_in0, const float* dfeat_in1, const float* dfeat_in2,
                        float* dfeat0, float* dfeat1, float* dfeat2, int N, int C, void* stream) {
    return pool_rows3_bwd<float>(drows, dfeat_in0, dfeat_in1, dfeat_in2, dfeat0, dfeat1, dfeat2, N, C, stream);
}
int ds6g_h16_pool_rows3_bwd(int st16, const float* drows, const void* dfeat_in0, const void* dfeat_in1, const void* dfeat_in2,
                            void* dfeat0, void* dfeat1, void* dfeat2, int N, int C, void* stream) {
    DS6G_RETURN_H16(st16, pool_rows3_bwd, drows, dfeat_in0, dfeat_in1, dfeat_in2, dfeat0, dfeat1, dfeat2, N, C, stream);
}

}  // extern "C"
