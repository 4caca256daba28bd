// Device and host helpers shared by the Mamba layer's kernels (mamba.hip: training forward and backward) and the grouped
// forward-only kernels of the frozen inference engine (mamba_infer.hip): the scan's lane mapping and constants, the DPP row
// sum, the activation spellings, the LDS staging of 16-column row pieces, the recurrences of the forward passes, the conv's
// per-lane body and the argument rules.  ONE definition, so the two files cannot drift apart in arithmetic.
#pragma once
#include "common.h"

namespace {

constexpr int SCAN_CHUNK = 32;   // positions per chunk = registers of h history per lane in the backward
constexpr int NS = 16;           // d_state
constexpr int CPB = 16;          // channels per workgroup (256 threads)
constexpr int TILE = SCAN_CHUNK * CPB;
constexpr float LOG2E = 1.4426950408889634f;

constexpr int CONV_TT = 64;      // positions per workgroup of the conv backward
constexpr int CONV_CB = 128;     // channels per workgroup of the conv backward (32 quads x 8 position lanes)

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over the 16 lanes of a DPP row, delivered to all of them: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror,
// row_mirror.  Fixed order.
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return v;
}

__device__ __forceinline__ float sigmoid_(float v) { return 1.f / (1.f + expf(-v)); }
// mamba_ssm's softplus: v for v > 20, else log1p(exp(v))
__device__ __forceinline__ float softplus_(float v) { return v > 20.f ? v : log1pf(expf(v)); }

// one 16-byte piece of a row as fp32: 4 floats, or 8 elements of a 16-bit type
template <typename S> struct Piece { static constexpr int N = 16 / (int)sizeof(S); };
__device__ __forceinline__ void ld_piece(const float* p, float (&v)[4]) {
    const f32x4 t = ld4(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t[e];
}
__device__ __forceinline__ void st_piece(float* p, const float (&v)[4]) { st4(p, f32x4{v[0], v[1], v[2], v[3]}); }
template <typename H>
__device__ __forceinline__ void ld_piece(const H* p, float (&v)[8]) {
    const typename H16<H>::x8 t = *reinterpret_cast<const typename H16<H>::x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
}
template <typename H>
__device__ __forceinline__ void st_piece(H* p, const float (&v)[8]) {   // round to nearest even, one rounding per element
    typename H16<H>::x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (H)v[e];
    *reinterpret_cast<typename H16<H>::x8*>(p) = t;
}

// tile[s][0..15] <- src[row(s0 + s)][col0 .. col0 + 16) as fp32, zeros for s >= len.  One 16-byte piece per thread: 128
// threads for an fp32 source (part selects which half of the workgroup), the first 64 of them for a 16-bit one.
template <typename S>
__device__ __forceinline__ void stage16(float* tile, const S* __restrict__ src, int ld, size_t rowbase, int L, int s0,
                                        int len, int rev, int col0, int part) {
    constexpr int PN = Piece<S>::N, PPR = 16 / PN;   // elements per piece, pieces per row
    const int i = (int)threadIdx.x - part * 128;
    if (i < 0 || i >= SCAN_CHUNK * PPR) return;
    const int s = i / PPR, q = i % PPR;
    float v[PN];
#pragma unroll
    for (int e = 0; e < PN; ++e) v[e] = 0.f;
    if (s < len) {
        const int t = rev ? L - 1 - (s0 + s) : s0 + s;
        ld_piece(src + (rowbase + t) * (size_t)ld + col0 + q * PN, v);
    }
#pragma unroll
    for (int e = 0; e < PN; e += 4) st4(tile + s * 16 + q * PN + e, f32x4{v[e], v[e + 1], v[e + 2], v[e + 3]});
}
// dst[row(s0 + s)][col0 .. col0 + 16) <- tile[s][0..15] for s < len, rounded to dst's type
template <typename S>
__device__ __forceinline__ void unstage16(const float* tile, S* __restrict__ dst, int ld, size_t rowbase, int L, int s0,
                                          int len, int rev, int col0, int part) {
    constexpr int PN = Piece<S>::N, PPR = 16 / PN;
    const int i = (int)threadIdx.x - part * 128;
    if (i < 0 || i >= SCAN_CHUNK * PPR) return;
    const int s = i / PPR, q = i % PPR;
    if (s < len) {
        const int t = rev ? L - 1 - (s0 + s) : s0 + s;
        float v[PN];
#pragma unroll
        for (int e = 0; e < PN; e += 4) {
            const f32x4 w = ld4(tile + s * 16 + q * PN + e);
            v[e] = w[0]; v[e + 1] = w[1]; v[e + 2] = w[2]; v[e + 3] = w[3];
        }
        st_piece(dst + (rowbase + t) * (size_t)ld + col0 + q * PN, v);
    }
}

// ---- the forward recurrences over one staged chunk; lane = (channel dl, state n), A2 = A log2(e) ----------------------
// state pass: from h = 0 -> the chunk's end state and its sum of delta.  s_du holds delta * u
__device__ __forceinline__ void scan_state_walk(const float* s_dl, const float* s_du, const float* s_B, int len, int dl, int n,
                                                float A2, float& h, float& sd) {
    h = 0.f; sd = 0.f;
    for (int s = 0; s < len; ++s) {
        const float dt = s_dl[s * 16 + dl];
        h = fmaf(exp2f(dt * A2), h, s_du[s * 16 + dl] * s_B[s * 16 + n]);
        sd += dt;
    }
}
// emit pass: from the chunk's true incoming state h; s_z holds silu(z) and receives y = (<h, C> + D u) silu(z)
__device__ __forceinline__ void scan_emit_walk(const float* s_dl, const float* s_u, float* s_z, const float* s_B,
                                               const float* s_C, int len, int dl, int n, float A2, float Dd, float h) {
    for (int s = 0; s < len; ++s) {
        const float dt = s_dl[s * 16 + dl], uu = s_u[s * 16 + dl];
        h = fmaf(exp2f(dt * A2), h, dt * uu * s_B[s * 16 + n]);
        const float yv = row16_sum(h * s_C[s * 16 + n]);
        if (n == 0) s_z[s * 16 + dl] = fmaf(Dd, uu, yv) * s_z[s * 16 + dl];
    }
}
// carry of one (sample, channel, state): hin[c + 1] = exp(A sum_delta_c) hin[c] + hin[c + 1] for c = 0 .. nc - 2 (hin[0] = 0,
// never stored).  cid0: the sample's first chunk id; per = D * NS; dn = channel * NS + state
__device__ __forceinline__ void scan_carry_walk(float* hin, const float* sumd, const float* A_log, size_t cid0, int nc,
                                                int D, size_t per, int dn) {
    const float A2 = -expf(A_log[dn]) * LOG2E;
    float h = 0.f;
    for (int c = 0; c + 1 < nc; ++c) {
        const size_t cid = cid0 + c;
        float* slot = hin + (cid + 1) * per + dn;
        h = fmaf(exp2f(sumd[cid * D + (dn >> 4)] * A2), h, *slot);
        *slot = h;
    }
}

// ---- causal depthwise conv1d (4 taps) + bias + SiLU: the body of one lane --------------------------------------------
// lane i of B * L * D / 4 owns four channels of one token.  position s of the walk is token t = s (forward) or L - 1 - s
// (reverse); y_s = silu(bias + sum_k w[k] x_{s - 3 + k})
template <typename T>
__device__ __forceinline__ void conv1d_silu_fwd_lane(const T* __restrict__ x, int ld_x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, T* __restrict__ y, int ld_y, int B,
                                                     int L, int D, int rev, size_t i) {
    const int q4 = D >> 2;
    if (i >= (size_t)B * L * q4) return;
    const size_t row = i / q4;
    const int d = (int)(i % q4) * 4;
    const int b = (int)(row / L), t = (int)(row % L);
    const int s = rev ? L - 1 - t : t;
    f32x4 wv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wv[j] = ld4(w + (d + j) * 4);
    f32x4 acc = ld4(bias + d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sk = s - 3 + k;
        if (sk < 0) continue;
        const int tk = rev ? L - 1 - sk : sk;
        const f32x4 xv = ld4(x + ((size_t)b * L + tk) * ld_x + d);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(wv[j][k], xv[j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] *= sigmoid_(acc[j]);
    st4(y + row * ld_y + d, acc);
}

// ---- argument rules -----------------------------------------------------------------------------------------------
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool ld_ok(int ld, int width) { return ld >= width && ld % 4 == 0; }
// row stride of an operand stored as T, in elements: whole 16-byte pieces (4 floats, 8 elements of a 16-bit type)
template <typename T> inline bool ld_okT(int ld, int width) { return ld >= width && ld % (16 / (int)sizeof(T)) == 0; }
inline int nchunks(int L) { return (L + SCAN_CHUNK - 1) / SCAN_CHUNK; }
inline bool dims_ok(int B, int L, int D) {
    // grid limits (blockIdx.y / .z), the int token arithmetic of the kernels, and the conv backward's 128-channel tile (the
    // scan kernels alone would need D % 16; the layer's D = 2 * d_model, d_model % 64 == 0, always satisfies both)
    return B > 0 && L > 0 && D > 0 && B <= 65535 && L <= (1 << 20) && D % CONV_CB == 0 && D <= (1 << 16) &&
           (long)B * L < (1L << 31) / 64;
}

}  // namespace
