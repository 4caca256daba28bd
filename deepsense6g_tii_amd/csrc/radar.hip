// Raw radar cube -> range-angle and range-velocity maps, the offline numpy step of the reference
// (Data_Preprocessing/Radar_data_preprocessing.py:7-23,41-42) done on the device for a whole batch of frames and written
// straight into the NHWC x4 tensor the radar stem reads.  For one frame's cube x[a][s][k] (a < A antennas, 256 samples,
// 128 chirps, complex64 as interleaved floats):
//   R[a][r][k] = sum_s x[a][s][k] e^(-2 pi i r s / 256)                                      range FFT
//   m[a][r]    = (1/128) sum_k R[a][r][k]
//   ang[r][th] = sum_k | sum_a (R[a][r][k] - m[a][r]) e^(-2 pi i th a / 256) |                angle FFT, A -> 256 zero-padded
//   vel[r][v]  = sum_a | sum_k  R[a][r][k]            e^(-2 pi i v k / 256) |                 Doppler FFT, 128 -> 256 zero-padded
//   map        = (map - min) / (max - min)                                                    per map and frame
// Three launches: range FFT (LDS tiles of 16 chirps), one workgroup per range row for both raw maps and the row's
// min / max, and a finish pass that re-reduces the 256 row partials in a fixed order and normalises.  fp32 arithmetic,
// no float atomics: results are bit-reproducible.  Every twiddle is exp(-2 pi i j / 256) from one table, each entry
// taken from sincospi in double and rounded once - never from a recurrence; the length-256 FFTs are four radix-4
// decimation-in-frequency stages in LDS, whose output sits in base-4 digit-reversed order and is read back through
// rev4().  Sums of magnitudes run over eight interleaved partial sums that are combined as a tree.
#include "common.h"

namespace {

constexpr int RS = 256;   // samples per chirp = range bins
constexpr int RK = 128;   // chirps per frame
constexpr int RW = 256;   // angle / velocity bins
constexpr int RMAXA = 8;  // antennas
constexpr int RCB = 16;   // chirps per range-FFT tile (128-byte row segments)

__device__ __forceinline__ f32x2 cmul(const f32x2 a, const f32x2 w) {
    return f32x2{fmaf(a.x, w.x, -(a.y * w.y)), fmaf(a.x, w.y, a.y * w.x)};
}

// tw[j] = exp(-2 pi i j / 256), j < 256 (one entry per thread of a 256-thread workgroup)
__device__ __forceinline__ void fill_twiddles(f32x2* tw, int tid) {
    double s, c;
    sincospi((double)tid * (1.0 / 128.0), &s, &c);
    tw[tid] = f32x2{(float)c, (float)-s};
}

// position of output bin k after the four radix-4 DIF stages (and the bin held at position k): the base-4 digits reversed
__device__ __forceinline__ int rev4(int k) {
    return ((k & 3) << 6) | ((k & 0xc) << 2) | ((k & 0x30) >> 2) | ((k >> 6) & 3);
}

// butterfly j (< 64) of stage st (< 4) of an in-place radix-4 decimation-in-frequency FFT of length 256 over
// x[i * es], i < 256.  Stage st works on sub-sequences of length 4 L, L = 64 >> 2 st.
__device__ __forceinline__ void bfly4(f32x2* x, int es, int j, int st, const f32x2* tw) {
    const int sh = 6 - 2 * st;
    const int L = 1 << sh;
    const int p = j & (L - 1);
    const int b = ((j >> sh) << (sh + 2)) + p;
    f32x2* x0 = x + b * es;
    f32x2* x1 = x0 + L * es;
    f32x2* x2 = x1 + L * es;
    f32x2* x3 = x2 + L * es;
    const f32x2 a0 = *x0, a1 = *x1, a2 = *x2, a3 = *x3;
    const f32x2 s02 = a0 + a2, d02 = a0 - a2, s13 = a1 + a3, d13 = a1 - a3;
    const f32x2 y0 = s02 + s13;
    f32x2 y2 = s02 - s13;
    f32x2 y1 = f32x2{d02.x + d13.y, d02.y - d13.x};  // d02 - i d13
    f32x2 y3 = f32x2{d02.x - d13.y, d02.y + d13.x};  // d02 + i d13
    if (st < 3) {                                     // the last stage's twiddles are all 1
        const int q = p << (2 * st);                  // p * 256 / (4 L)
        y1 = cmul(y1, tw[q]);
        y2 = cmul(y2, tw[2 * q]);
        y3 = cmul(y3, tw[3 * q]);
    }
    *x0 = y0;
    *x1 = y1;
    *x2 = y2;
    *x3 = y3;
}

// grid (8 chirp blocks, N * A): cube / R [N * A][256][128] complex.  The 256 x 16 tile is 32 KB of LDS, [sample][chirp].
__global__ __launch_bounds__(256) void radar_range_fft_kernel(const f32x2* __restrict__ cube, f32x2* __restrict__ R) {
    __shared__ __attribute__((aligned(16))) f32x2 x[RS * RCB];
    __shared__ f32x2 tw[256];
    const int tid = threadIdx.x;
    const long base = (long)blockIdx.y * RS * RK + (long)blockIdx.x * RCB;
    fill_twiddles(tw, tid);
    const int c2 = (tid & 7) * 2, s0 = tid >> 3;      // 8 lanes x 16 B = one 128-byte row segment
#pragma unroll
    for (int i = 0; i < RS / 32; ++i) {
        const int s = i * 32 + s0;
        *reinterpret_cast<f32x4*>(x + s * RCB + c2) = *reinterpret_cast<const f32x4*>(cube + base + (long)s * RK + c2);
    }
    __syncthreads();
    const int c = tid & (RCB - 1), j0 = tid >> 4;     // 16 FFTs x 64 butterflies per stage, 4 per thread
#pragma unroll
    for (int st = 0; st < 4; ++st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) bfly4(x + c, RCB, j0 + 16 * i, st, tw);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < RS / 32; ++i) {
        const int s = i * 32 + s0;                    // LDS row s holds range bin rev4(s)
        *reinterpret_cast<f32x4*>(R + base + (long)rev4(s) * RK + c2) = *reinterpret_cast<const f32x4*>(x + s * RCB + c2);
    }
}

__device__ __forceinline__ float cabs32(const f32x2 z) { return sqrtf(fmaf(z.x, z.x, z.y * z.y)); }

// min and max of v over the 256 threads of the workgroup (values are never NaN here or NaN everywhere); red: 8 floats
__device__ __forceinline__ void block_minmax(float v, float* red, int tid, float& mn, float& mx) {
    float lo = v, hi = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        red[tid >> 6] = lo;
        red[4 + (tid >> 6)] = hi;
    }
    __syncthreads();
    mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

// grid (256 range rows, N).  raw: [N][2][256][256] (plane 0 angle, plane 1 velocity), part: [N][256][2][2] (min, max).
template <int A>
__global__ __launch_bounds__(256) void radar_maps_raw_kernel(const f32x2* __restrict__ R, float* __restrict__ raw,
                                                             float* __restrict__ part, int nch) {
    __shared__ __attribute__((aligned(16))) f32x2 D[RK * A];   // [chirp][antenna]: R, then R - m
    __shared__ f32x2 F[A * RW];                                 // Doppler FFT buffers, one per antenna
    __shared__ f32x2 tw[256];
    __shared__ f32x2 mean[A];
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const long n = blockIdx.y;
    fill_twiddles(tw, tid);
    for (int i = tid; i < A * RK; i += 256) {
        const int a = i >> 7, k = i & (RK - 1);
        const f32x2 v = R[((n * A + a) * RS + r) * RK + k];
        D[k * A + a] = v;
        if (nch > 1) {
            F[a * RW + k] = v;
            F[a * RW + RK + k] = f32x2{0.f, 0.f};
        }
    }
    __syncthreads();
    for (int a = wave; a < A; a += 4) {
        f32x2 s = D[lane * A + a] + D[(lane + 64) * A + a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s.x += __shfl_xor(s.x, o, 64);
            s.y += __shfl_xor(s.y, o, 64);
        }
        if (lane == 0) mean[a] = s * (1.f / RK);
    }
    __syncthreads();
    for (int i = tid; i < A * RK; i += 256) D[(i & (RK - 1)) * A + (i >> 7)] -= mean[i >> 7];
    float vel = 0.f;
    if (nch > 1) {
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            for (int i = tid; i < A * 64; i += 256) bfly4(F + (i >> 6) * RW, 1, i & 63, st, tw);
            __syncthreads();
        }
        const int pv = rev4(tid);
#pragma unroll
        for (int a = 0; a < A; ++a) vel += cabs32(F[a * RW + pv]);
    }
    __syncthreads();
    // angle half: thread th keeps exp(-2 pi i th a / 256) in registers; every read of D is a broadcast
    f32x2 w[A];
#pragma unroll
    for (int a = 0; a < A; ++a) w[a] = tw[(tid * a) & 255];
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < RK; k0 += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const f32x2* d = D + (k0 + u) * A;
            f32x2 z = cmul(d[0], w[0]);
#pragma unroll
            for (int a = 1; a < A; ++a) {
                const f32x2 t = d[a];
                z.x = fmaf(t.x, w[a].x, fmaf(-t.y, w[a].y, z.x));
                z.y = fmaf(t.x, w[a].y, fmaf(t.y, w[a].x, z.y));
            }
            acc[u] += cabs32(z);
        }
    }
    const float ang = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    const long row = (n * 2 * RS + r) * RW;
    float* p = part + (n * RS + r) * 4;
    float mn, mx;
    raw[row + tid] = ang;
    block_minmax(ang, red, tid, mn, mx);
    if (tid == 0) { p[0] = mn; p[1] = mx; }
    if (nch > 1) {
        raw[row + (long)RS * RW + tid] = vel;
        block_minmax(vel, red, tid, mn, mx);
        if (tid == 0) { p[2] = mn; p[3] = mx; }
    }
}

constexpr int RFROWS = 8;  // map rows per workgroup of the finish pass

// grid (256 / 8, N).  Every workgroup re-reduces the frame's 256 row partials (2 KB, fixed order), then normalises its rows.
// planar == 0: dst[(n * fps + t)][r][w][Cd], channel 0 angle, 1 velocity (nch == 2), the rest zero.
// planar != 0: dst[n][nch][r][w].  flip mirrors the w axis.
__global__ __launch_bounds__(256) void radar_finish_kernel(const float* __restrict__ raw, const float* __restrict__ part,
                                                           float* __restrict__ dst, int nch, int Cd, int fps, int t,
                                                           int flip, int planar) {
    __shared__ float red[8];
    const int tid = threadIdx.x;
    const long n = blockIdx.y;
    float mn[2] = {0.f, 0.f}, den[2] = {1.f, 1.f};
    for (int c = 0; c < nch; ++c) {
        const float* p = part + ((n * RS + tid) * 2 + c) * 2;
        const float lo = p[0], hi = p[1];
        float a, b, unused;
        block_minmax(lo, red, tid, a, unused);
        block_minmax(hi, red, tid, unused, b);
        mn[c] = a;
        den[c] = b - a;
    }
    const int ws = flip ? RW - 1 - tid : tid;
    for (int i = 0; i < RFROWS; ++i) {
        const int r = blockIdx.x * RFROWS + i;
        float v[2] = {0.f, 0.f};
        for (int c = 0; c < nch; ++c) v[c] = (raw[((n * 2 + c) * RS + r) * RW + ws] - mn[c]) / den[c];
        if (planar) {
            for (int c = 0; c < nch; ++c) dst[((n * nch + c) * RS + r) * RW + tid] = v[c];
        } else {
            float* o = dst + (((n * fps + t) * RS + r) * RW + tid) * Cd;
            if (Cd == 4) {
                *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], 0.f, 0.f};
            } else {
                for (int c = 0; c < Cd; ++c) o[c] = c < nch ? v[c] : 0.f;
            }
        }
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ds6g_radar_range_fft(const float* cube, long cube_elems, float* R, long r_elems, int N, int A, int S, int K,
                         void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(cube && R && N > 0 && A >= 1 && A <= RMAXA && S == RS && K == RK);
    DS6G_CHECK_ARG(aligned16(cube) && aligned16(R) && (long)N * A <= 65535);
    const long need = (long)N * A * RS * RK * 2;
    DS6G_CHECK_WS(cube_elems >= need && r_elems >= need);
    hipLaunchKernelGGL(radar_range_fft_kernel, dim3(RK / RCB, N * A), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x2*>(cube), reinterpret_cast<f32x2*>(R));
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_radar_maps_raw(const float* R, long r_elems, float* raw, long raw_elems, float* part, long part_elems, int N,
                        int A, int S, int K, int nch, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(R && raw && part && N > 0 && N <= 65535 && A >= 1 && A <= RMAXA && S == RS && K == RK);
    DS6G_CHECK_ARG(nch == 1 || nch == 2);
    DS6G_CHECK_WS(r_elems >= (long)N * A * RS * RK * 2 && raw_elems >= (long)N * 2 * RS * RW &&
                  part_elems >= (long)N * RS * 4);
    const dim3 grid(RS, N), block(256);
    const f32x2* Rc = reinterpret_cast<const f32x2*>(R);
    hipStream_t st = (hipStream_t)stream;
    switch (A) {
#define DS6G_RADAR_CASE(a) case a: hipLaunchKernelGGL(radar_maps_raw_kernel<a>, grid, block, 0, st, Rc, raw, part, nch); break;
        DS6G_RADAR_CASE(1) DS6G_RADAR_CASE(2) DS6G_RADAR_CASE(3) DS6G_RADAR_CASE(4)
        DS6G_RADAR_CASE(5) DS6G_RADAR_CASE(6) DS6G_RADAR_CASE(7) DS6G_RADAR_CASE(8)
#undef DS6G_RADAR_CASE
    }
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

int ds6g_radar_finish(const float* raw, long raw_elems, const float* part, long part_elems, float* dst, long dst_elems,
                      int N, int nch, int Cd, int frames_per_sample, int t, int flip, int planar, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(raw && part && dst && N > 0 && N <= 65535 && (nch == 1 || nch == 2));
    DS6G_CHECK_ARG(Cd >= nch && frames_per_sample >= 1 && t >= 0 && t < frames_per_sample);
    DS6G_CHECK_ARG(!planar || (Cd == nch && frames_per_sample == 1));
    DS6G_CHECK_ARG(Cd != 4 || aligned16(dst));
    DS6G_CHECK_WS(raw_elems >= (long)N * 2 * RS * RW && part_elems >= (long)N * RS * 4 &&
                  dst_elems >= (long)N * frames_per_sample * RS * RW * Cd);
    hipLaunchKernelGGL(radar_finish_kernel, dim3(RS / RFROWS, N), dim3(256), 0, (hipStream_t)stream, raw, part, dst, nch,
                       Cd, frames_per_sample, t, flip, planar);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}

}  // extern "C"
