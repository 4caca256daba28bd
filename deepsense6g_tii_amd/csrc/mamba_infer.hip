// The Mamba layer's conv and scan for a FROZEN model (mamba_infer.py): forward only, no tape, and grouped - one launch
// covers ndir = 1 or 2 directions, each with operands, row strides and walk direction of its own (ds6g_mamba_conv_dir /
// ds6g_mamba_scan_dir of ds6g_types.h, handed to the kernel by value).  A bi-directional block then makes one conv launch
// and three scan launches where two layers make two and six, and dt_proj runs inside the scan:
//   conv   blockIdx.z = direction; per lane the arithmetic of mamba.hip's conv1d_silu_fwd_kernel (conv1d_silu_fwd_lane)
//   scan   blockIdx.z = direction * B + sample.  mamba.hip's mapping (lane = (channel, state), 16 channels x 16 states per
//          workgroup, one chunk of SCAN_CHUNK positions staged in LDS), its three passes (state, carry, emit) and its
//          recurrences (scan_state_walk / scan_carry_walk / scan_emit_walk of mamba_dev.h).  What differs is where delta
//          comes from: the workgroup stages its chunk's dt rows [32][r] and its 16 rows of dt_proj.weight [16][r] and evaluates
//              delta[s][ch] = softplus(bias[ch] + sum_j dt[s][j] W[ch][j])
//          as ONE fmaf chain over j = 0 .. r - 1 from 0, the bias added last (the operand order of softplus_(raw + dt_bias)),
//          once per (token, channel).  No delta_raw tensor, no dt copy, no dt_proj GEMM.
// T is the storage type of x / y (conv) and u / z / y (scan): float, __bf16 or _Float16; x_dbl, the parameters, the chunk
// states and all arithmetic are fp32.  The chunk-start states and delta sums live in the caller's workspace
// (ds6g_mamba_scan_fwd_grouped_workspace_size).  No float atomics: two runs are bit-identical, and a two-direction launch
// equals the two one-direction launches bit for bit (a workgroup never reads another direction's data).
#include "mamba_dev.h"

namespace {

constexpr int DT_LD = 36;   // LDS row stride of the dt and dt_proj.weight tiles: r <= 32 columns + 4, so rows stay 16-byte
                            // aligned (ds_read_b128) and the 16 channel rows a 16-lane group reads start in 16 different
                            // 16-byte slots (9 ch mod 16 is a permutation)

template <typename T>
struct ScanG {
    ds6g_mamba_scan_dir dir[DS6G_MAMBA_MAX_DIR];
    float* hin;      // [ndir * B][nc][D][16] states at chunk starts (slot 0 of a sample is never touched: it is zero)
    float* sumd;     // [ndir * B][nc][D]
    int B, L, D, nc, r;
};

struct ConvG {
    ds6g_mamba_conv_dir dir[DS6G_MAMBA_MAX_DIR];
    int B, L, D;
};

// s_dt[s][0 .. r) <- x_dbl[row(s0 + s)][0 .. r) (zeros for s >= len), s_W[ch][0 .. r) <- dt_w[d0 + ch][0 .. r).  One 16-byte
// piece per thread and tile: 32 * r / 4 <= 256 and 16 * r / 4 <= 128 pieces.
__device__ __forceinline__ void stage_dt(float* s_dt, float* s_W, const float* __restrict__ x_dbl, int ld_x,
                                         const float* __restrict__ dt_w, size_t rowbase, int L, int s0, int len, int rev,
                                         int d0, int r) {
    const int i = (int)threadIdx.x, r4 = r >> 2;
    if (i < SCAN_CHUNK * r4) {
        const int s = i / r4, q = i % r4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (s < len) {
            const int t = rev ? L - 1 - (s0 + s) : s0 + s;
            v = ld4(x_dbl + (rowbase + t) * (size_t)ld_x + q * 4);
        }
        st4(s_dt + s * DT_LD + q * 4, v);
    }
    if (i < CPB * r4) {
        const int ch = i / r4, q = i % r4;
        st4(s_W + ch * DT_LD + q * 4, ld4(dt_w + (size_t)(d0 + ch) * r + q * 4));
    }
}
// delta of the two tile elements a thread owns, (s, ch) and (s + 16, ch) with s = tid / 16, ch = tid % 16: they share the
// weight row, read once.  Each is ONE fmaf chain over j = 0 .. r - 1 from 0, the bias added last.
__device__ __forceinline__ void delta_pair(const float* s_dt, const float* s_W, int tid, int r, float bias, float& d0v,
                                           float& d1v) {
    const float* a = s_dt + (tid >> 4) * DT_LD;
    const float* b = a + 16 * DT_LD;
    const float* w = s_W + (tid & 15) * DT_LD;
    float acc0 = 0.f, acc1 = 0.f;
    for (int j = 0; j < r; j += 4) {
        const f32x4 wv = ld4(w + j), av = ld4(a + j), bv = ld4(b + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc0 = fmaf(av[e], wv[e], acc0);
            acc1 = fmaf(bv[e], wv[e], acc1);
        }
    }
    d0v = softplus_(acc0 + bias);
    d1v = softplus_(acc1 + bias);
}

#define SCANG_IDS()                                                                        \
    const int g = blockIdx.x, c = blockIdx.y, bz = blockIdx.z;                             \
    const ds6g_mamba_scan_dir& q = p.dir[bz / p.B];                                        \
    const int b = bz % p.B, rev = q.reverse;                                               \
    const int tid = threadIdx.x, dl = tid >> 4, n = tid & 15;                              \
    const int d0 = g * CPB, d = d0 + dl;                                                   \
    const int s0 = c * SCAN_CHUNK;                                                         \
    const int len = min(SCAN_CHUNK, p.L - s0);                                             \
    const size_t rowbase = (size_t)b * p.L;                                                \
    const float A2 = -expf(q.A_log[d * NS + n]) * LOG2E;   /* exp(delta A) = exp2(delta A2) */ \
    const size_t chunk_id = (size_t)bz * p.nc + c

// state pass: chunk c (< nc - 1) from h = 0 -> hin slot c + 1 (its end state), sumd[c]
template <typename T>
__global__ __launch_bounds__(256) void scang_state_kernel(const ScanG<T> p) {
    __shared__ float s_dl[TILE], s_u[TILE], s_B[TILE];
    __shared__ __attribute__((aligned(16))) float s_dt[SCAN_CHUNK * DT_LD], s_W[CPB * DT_LD];
    SCANG_IDS();
    const float* xd = q.x_dbl;
    stage_dt(s_dt, s_W, xd, q.ld_x, q.dt_w, rowbase, p.L, s0, len, rev, d0, p.r);
    stage16(s_u, (const T*)q.u, q.ld_u, rowbase, p.L, s0, len, rev, d0, 1);
    stage16(s_B, xd + p.r, q.ld_x, rowbase, p.L, s0, len, rev, 0, 0);
    __syncthreads();
    {
        float dt0, dt1;
        delta_pair(s_dt, s_W, tid, p.r, q.dt_b[d0 + n], dt0, dt1);
        s_dl[tid] = dt0; s_dl[tid + 256] = dt1;
        s_u[tid] *= dt0; s_u[tid + 256] *= dt1;
    }
    __syncthreads();
    float h, sd;
    scan_state_walk(s_dl, s_u, s_B, len, dl, n, A2, h, sd);
    p.hin[((chunk_id + 1) * p.D + d) * NS + n] = h;
    if (n == 0) p.sumd[chunk_id * p.D + d] = sd;
}

// one thread per (direction, sample, channel, state)
template <typename T>
__global__ __launch_bounds__(256) void scang_carry_kernel(const ScanG<T> p, int nbz) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)p.D * NS;
    if (i >= (size_t)nbz * per) return;
    const int bz = (int)(i / per);
    const int dn = (int)(i % per);
    scan_carry_walk(p.hin, p.sumd, p.dir[bz / p.B].A_log, (size_t)bz * p.nc, p.nc, p.D, per, dn);
}

// emit pass
template <typename T>
__global__ __launch_bounds__(256) void scang_emit_kernel(const ScanG<T> p) {
    __shared__ float s_dl[TILE], s_u[TILE], s_z[TILE], s_B[TILE], s_C[TILE];
    __shared__ __attribute__((aligned(16))) float s_dt[SCAN_CHUNK * DT_LD], s_W[CPB * DT_LD];
    SCANG_IDS();
    const float* xd = q.x_dbl;
    stage_dt(s_dt, s_W, xd, q.ld_x, q.dt_w, rowbase, p.L, s0, len, rev, d0, p.r);
    stage16(s_u, (const T*)q.u, q.ld_u, rowbase, p.L, s0, len, rev, d0, 1);
    stage16(s_z, (const T*)q.z, q.ld_z, rowbase, p.L, s0, len, rev, d0, 0);
    __syncthreads();
    stage16(s_B, xd + p.r, q.ld_x, rowbase, p.L, s0, len, rev, 0, 1);
    stage16(s_C, xd + p.r + NS, q.ld_x, rowbase, p.L, s0, len, rev, 0, 0);
    delta_pair(s_dt, s_W, tid, p.r, q.dt_b[d0 + n], s_dl[tid], s_dl[tid + 256]);
    for (int i = tid; i < TILE; i += 256) { const float zz = s_z[i]; s_z[i] = zz * sigmoid_(zz); }
    __syncthreads();
    const float h = c > 0 ? p.hin[(chunk_id * p.D + d) * NS + n] : 0.f;
    scan_emit_walk(s_dl, s_u, s_z, s_B, s_C, len, dl, n, A2, q.D[d], h);
    __syncthreads();
    unstage16(s_z, (T*)q.y, p.D, rowbase, p.L, s0, len, rev, d0, 0);
}

template <typename T>
__global__ __launch_bounds__(256) void convg_fwd_kernel(const ConvG p) {
    const ds6g_mamba_conv_dir& q = p.dir[blockIdx.z];
    conv1d_silu_fwd_lane<T>((const T*)q.x, q.ld_x, q.w, q.bias, (T*)q.y, p.D, p.B, p.L, p.D, q.reverse,
                            (size_t)blockIdx.x * 256 + threadIdx.x);
}

inline bool ndir_ok(int ndir, int B) { return ndir >= 1 && ndir <= DS6G_MAMBA_MAX_DIR && (long)ndir * B <= 65535; }

}  // namespace

extern "C" {

size_t ds6g_mamba_scan_fwd_grouped_workspace_size(int B, int L, int D, int ndir) {
    if (B <= 0 || L <= 0 || D <= 0 || ndir <= 0) return 0;
    return (size_t)ndir * B * nchunks(L) * D * (NS + 1) * sizeof(float);
}

extern "C++" template <typename T>
static int mamba_conv_fwd_grouped(const ds6g_mamba_conv_dir* dirs, int ndir, int B, int L, int D, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dirs && dims_ok(B, L, D) && ndir_ok(ndir, B));
    ConvG p{};
    for (int k = 0; k < ndir; ++k) {
        const ds6g_mamba_conv_dir& q = dirs[k];
        DS6G_CHECK_ARG(q.x && q.w && q.bias && q.y && ld_okT<T>(q.ld_x, D));
        DS6G_CHECK_ARG(al16(q.x) && al16(q.w) && al16(q.bias) && al16(q.y));
        p.dir[k] = q;
        p.dir[k].reverse = q.reverse ? 1 : 0;
    }
    p.B = B; p.L = L; p.D = D;
    const size_t n = (size_t)B * L * (D / 4);
    hipLaunchKernelGGL(convg_fwd_kernel<T>, dim3((unsigned)((n + 255) / 256), 1, ndir), dim3(256), 0, (hipStream_t)stream, p);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_mamba_conv_fwd_grouped(const ds6g_mamba_conv_dir* dirs, int ndir, int B, int L, int D, void* stream) {
    return mamba_conv_fwd_grouped<float>(dirs, ndir, B, L, D, stream);
}
int ds6g_h16_mamba_conv_fwd_grouped(int st16, const ds6g_mamba_conv_dir* dirs, int ndir, int B, int L, int D, void* stream) {
    DS6G_RETURN_H16(st16, mamba_conv_fwd_grouped, dirs, ndir, B, L, D, stream);
}

extern "C++" template <typename T>
static int mamba_scan_fwd_grouped(const ds6g_mamba_scan_dir* dirs, int ndir, int B, int L, int D, int r, void* ws,
                                  size_t ws_bytes, void* stream) {
    DS6G_ENTER();
    DS6G_CHECK_ARG(dirs && ws && dims_ok(B, L, D) && ndir_ok(ndir, B) && r >= 4 && r <= 32 && r % 4 == 0 && al16(ws));
    ScanG<T> p{};
    for (int k = 0; k < ndir; ++k) {
        const ds6g_mamba_scan_dir& q = dirs[k];
        DS6G_CHECK_ARG(q.u && q.z && q.x_dbl && q.dt_w && q.dt_b && q.A_log && q.D && q.y);
        DS6G_CHECK_ARG(ld_okT<T>(q.ld_u, D) && ld_okT<T>(q.ld_z, D) && ld_ok(q.ld_x, r + 2 * NS));
        DS6G_CHECK_ARG(al16(q.u) && al16(q.z) && al16(q.x_dbl) && al16(q.dt_w) && al16(q.y));
        p.dir[k] = q;
        p.dir[k].reverse = q.reverse ? 1 : 0;
    }
    DS6G_CHECK_WS(ws_bytes >= ds6g_mamba_scan_fwd_grouped_workspace_size(B, L, D, ndir));
    hipStream_t st = (hipStream_t)stream;
    const int nbz = ndir * B;
    p.B = B; p.L = L; p.D = D; p.nc = nchunks(L); p.r = r;
    p.sumd = (float*)ws;
    p.hin = p.sumd + (size_t)nbz * p.nc * D;
    if (p.nc > 1) {
        hipLaunchKernelGGL(scang_state_kernel<T>, dim3(D / CPB, p.nc - 1, nbz), dim3(256), 0, st, p);
        DS6G_LAUNCH_CHECK();
        hipLaunchKernelGGL(scang_carry_kernel<T>, dim3(cdiv((long)nbz * D * NS, 256)), dim3(256), 0, st, p, nbz);
        DS6G_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(scang_emit_kernel<T>, dim3(D / CPB, p.nc, nbz), dim3(256), 0, st, p);
    DS6G_LAUNCH_CHECK();
    return DS6G_OK;
}
int ds6g_mamba_scan_fwd_grouped(const ds6g_mamba_scan_dir* dirs, int ndir, int B, int L, int D, int r, void* ws,
                                size_t ws_bytes, void* stream) {
    return mamba_scan_fwd_grouped<float>(dirs, ndir, B, L, D, r, ws, ws_bytes, stream);
}
int ds6g_h16_mamba_scan_fwd_grouped(int st16, const ds6g_mamba_scan_dir* dirs, int ndir, int B, int L, int D, int r, void* ws,
                                    size_t ws_bytes, void* stream) {
    DS6G_RETURN_H16(st16, mamba_scan_fwd_grouped, dirs, ndir, B, L, D, r, ws, ws_bytes, stream);
}

}  // extern "C"
