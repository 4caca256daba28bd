// The launch planner of the conv / linear GEMM entry points of igemm.hip (fp32 storage) and bgemm.hip (16-bit storage).
// Every entry point states its call as a GemmProblem, gemm_plan() decides the launch - refusals, GEMM extents, tile, k-tile,
// walk, epilogue, split-K, XCD mapping, grid, variant code - as a pure function of (problem, knobs), and the entry point runs
// exactly what it returns; ds6g_gemm_plan (ds6g.h) shows the same plan to tests without a launch.  DESIGN.md 3.1 has the rules
// as one table.  Plain host C++17: no HIP include, nothing __device__, so a host compiler alone builds it.
#ifndef DS6G_GEMM_PLAN_H
#define DS6G_GEMM_PLAN_H
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include "../../include/ds6g_types.h"

typedef struct ds6g_gemm_plan GemmPlan;

enum { GEMM_FWD = 0, GEMM_DGRAD = 1, GEMM_WGRAD = 2 };  // GemmPlan::mode, the MODE template value of both kernels
constexpr int GEMM_ERR_ARG = 1, GEMM_ERR_WORKSPACE = 3; // DS6G_ERR_ARG, DS6G_ERR_WORKSPACE (common.h)
constexpr size_t GEMM_OOB = 0x80000000u;                // OOB_OFF (common.h): every tensor, and an fp32 output, stays below it

// what the caller asked for
struct GemmProblem {
    int family, op;                          // DS6G_GEMM_F32 / _H16, DS6G_GEMM_CONV_FWD ...
    int N, H, W, C, K, R, S, stride, pad;    // a Linear over M rows: the 1x1 conv of ONE 1 x M image (N = H = 1, W = M): the
                                             // kernels' per-k-tile pixel walk then never wraps
    int epilogue;                            // a fused epilogue is needed: bias, ReLU, ReLU mask, dropout or residual
    int out16, accumulate, want_dbias;
    size_t ws_bytes;
};

// every input of the decision that is not the problem; one filler per family (igemm_knobs, bgemm_knobs)
struct GemmKnobs {
    int operand_mode = 0;          // ds6g_set_compute_mode: operand mode of the fp32-storage kernels (their BF template value)
    // ds6g_set_debug_flags; fp32 storage only
    int dbg = 0;                   // flags & 0xbf: 0x80 forces the general (FAST 0) walk; the rest are the kernel's ablation bits
    int min_blocks = 2560;        // bits 8-19: many small (64x64, 8 waves/SIMD) workgroups beat larger tiles up to here (measured)
    int wgrad_tile = 1;            // 0x40 -> 2: 64x64 wgrad tiles
    int bf16_bk32 = 1;             // 0x10000000 -> 0: no 32-column k-tiles in the bf16 operand modes
    int f32_bk32 = 2;              // 0 never (0x40000000), 1 wherever the walk allows it (0x20000000), 2 small-spatial convs only
    // environment, fp32 storage: wgrad workgroups aimed at (measured, tools/bench_igemm.py: convs are fastest with ~2048
    // workgroups in flight, the GPT linears - large outputs, costlier slab reduction - with ~1024) and the XCD mapping
    long wgrad_target_lin = 1024;  // DS6G_WGRAD_TARGET_LIN
    long wgrad_target_conv = 2048; // DS6G_WGRAD_TARGET_CONV
    int wgrad_xcd = 1;             // DS6G_WGRAD_XCD: 0 off, 1 few-tile convs, 2 every conv wgrad (experiment)
    // environment, 16-bit storage
    int h16_tile = -1;             // DS6G_BG_TILE: >= 0 forces the fwd / dgrad tile code
    int h16_min_blocks = 200;      // DS6G_BG_MINBLOCKS: 128x128 tiles once they give this many workgroups, else 64x64
                                   // (tools/bench_bgemm.py: the large tile wins from ~240 workgroups up)
    int h16_wgrad_target = 0;      // DS6G_BG_WTARGET: > 0 replaces the targets 512 (linear) / 384 (conv): few, long splits win
    int h16_wgrad_xcd = 1;         // DS6G_BG_WXCD: 0 plain, 1 contiguous (split, tile) runs where they measured faster
                                   // (tools/bench_bwgrad.py), 2 every conv, 3 everything
};
inline void gemm_env(const char* name, int* v) { if (const char* e = getenv(name)) *v = atoi(e); }
inline void gemm_env(const char* name, long* v) { if (const char* e = getenv(name)) *v = atol(e); }

// what differs between the families in the split-K arithmetic and the walk rule
struct GemmFamily { int wgrad_bk, min_k_per_split, k_round, elem_bytes; };
constexpr GemmFamily GEMM_FAMILY[2] = {{16, 64, 32, 4},        // fp32 storage: >= 4 k-tiles of 16 per split
                                       {64, 4 * 64, 64, 2}};   // 16-bit storage: >= 4 k-tiles of 64 per split

inline long gemm_cdiv(long a, long b) { return (a + b - 1) / b; }

// uniform wgrad walk: the bk pixels of a k-tile share one (image, output row) -> 0, or cover whole output rows of one image
// -> rows per k-tile; -1: neither (fp32 storage takes the general walk, 16-bit storage refuses)
inline int gemm_wgrad_rows(int N, int Ho, int Wo, int bk) {
    if (Wo % bk == 0 || N * Ho == 1) return 0;
    if (bk % Wo == 0 && Ho % (bk / Wo) == 0) return bk / Wo;
    return -1;
}

// fwd / dgrad tile: the largest that still yields min_blocks workgroups.  fp32 storage: 128x128, 128x64, 64x64; 16-bit: no 128x64
inline void gemm_pick_tile(bool h16, int Mg, int Ng, long splits, const GemmKnobs& kn, int* BM, int* BN) {
    const long t128 = gemm_cdiv(Mg, 128) * gemm_cdiv(Ng, 128) * splits;
    *BM = *BN = 64;
    if (h16) {
        if (kn.h16_tile >= 0 ? kn.h16_tile == 0 : (t128 >= kn.h16_min_blocks && Mg > 64 && Ng > 64)) *BM = *BN = 128;
    } else if (Ng > 64 && Mg > 64 && t128 >= kn.min_blocks) {
        *BM = *BN = 128;
    } else if (Mg > 64 && gemm_cdiv(Mg, 128) * gemm_cdiv(Ng, 64) * splits >= kn.min_blocks) {
        *BM = 128;
    }
}

// wgrad: the output (a weight tensor) has few tiles and the reduction (pixels) is long: split K until the grid holds `target`
// workgroups, bounded by >= 4 k-tiles per split and by the workspace; then the tile -> XCD mapping, and direct launch or slabs
inline int gemm_plan_wgrad(const GemmProblem& q, const GemmKnobs& kn, bool linear, GemmPlan& pl) {
    const bool h16 = q.family == DS6G_GEMM_H16;
    const GemmFamily& f = GEMM_FAMILY[h16];
    const long out_elems = (long)pl.Mg * pl.Ng;
    if (pl.Mg <= 0 || pl.Ng <= 0 || pl.Kg <= 0 || out_elems % 4 != 0 || pl.Mg % 4 != 0) return GEMM_ERR_ARG;
    const long slab_elems = out_elems + (q.want_dbias ? pl.Mg : 0);
    long target;
    if (h16) {
        pl.BM = pl.BN = (pl.Mg >= 128 && pl.Ng >= 128) ? 128 : 64;
        target = kn.h16_wgrad_target > 0 ? kn.h16_wgrad_target : (linear ? 512 : 384);
    } else {
        pl.BM = (pl.Mg >= 128 && kn.wgrad_tile == 1) ? 128 : 64;
        pl.BN = 64;
        target = linear ? kn.wgrad_target_lin : kn.wgrad_target_conv;
    }
    const long tiles = gemm_cdiv(pl.Mg, pl.BM) * gemm_cdiv(pl.Ng, pl.BN);
    long splits = (target + tiles - 1) / tiles;
    const long max_by_k = gemm_cdiv(pl.Kg, f.min_k_per_split);
    if (splits > max_by_k) splits = max_by_k;
    const long max_by_ws = (long)(q.ws_bytes / (slab_elems * sizeof(float)));
    if (splits > max_by_ws) splits = max_by_ws;
    if (splits < 1) splits = 1;
    pl.k_per_split = (int)gemm_cdiv(gemm_cdiv(pl.Kg, splits), f.k_round) * f.k_round;
    splits = gemm_cdiv(pl.Kg, pl.k_per_split);
    pl.splits = (int)splits;
    pl.slab_elems = (size_t)slab_elems;
    pl.want_colsum = q.want_dbias != 0;
    // the column tiles of ONE split read the same dy rows and overlapping x rows: keep them on one XCD where that measured faster
    if (h16) {  // convs with <= 24 output tiles, and the large linears whose workgroup count is a multiple of 8 (whole splits per XCD)
        const bool pays = linear ? ((tiles * splits) % 8 == 0 && out_elems >= 512L * 512) : tiles <= 24;
        const int x = kn.h16_wgrad_xcd;
        pl.xcd_splits = splits >= 2 && ((x == 1 && pays) || (x == 2 && (!linear || pays)) || x >= 3);
    } else {    // few output tiles x many splits, i.e. the 64-channel 3x3 layers
        pl.xcd_splits = !linear && splits >= 8 && ((kn.wgrad_xcd == 1 && tiles <= 12) || kn.wgrad_xcd == 2);
    }
    pl.reduce = !(splits == 1 && !q.accumulate && !q.want_dbias);
    if (pl.reduce) {
        pl.ws_bytes_used = (size_t)splits * slab_elems * sizeof(float);
        if (pl.ws_bytes_used > q.ws_bytes) return GEMM_ERR_ARG;
    }
    return 0;
}

// -> 0 and *out, or the entry point's refusal
inline int gemm_plan(const GemmProblem& q, const GemmKnobs& kn, GemmPlan* out) {
    const bool h16 = q.family == DS6G_GEMM_H16;
    if (!out || (q.family != DS6G_GEMM_F32 && !h16) || q.op < DS6G_GEMM_CONV_FWD || q.op > DS6G_GEMM_CONV_FWD_BNSTATS) return GEMM_ERR_ARG;
    const bool linear_op = q.op >= DS6G_GEMM_LINEAR_FWD && q.op <= DS6G_GEMM_LINEAR_WGRAD;
    const bool bias_act = q.op == DS6G_GEMM_CONV_BIAS_ACT_FWD, bnstats = q.op == DS6G_GEMM_CONV_FWD_BNSTATS;
    if ((bnstats && !h16) || q.stride <= 0) return GEMM_ERR_ARG;
    if (linear_op && !(q.N == 1 && q.H == 1 && q.R == 1 && q.S == 1 && q.stride == 1 && q.pad == 0)) return GEMM_ERR_ARG;
    const GemmFamily& f = GEMM_FAMILY[h16];
    GemmPlan pl = {};
    pl.family = q.family;
    pl.mode = (bias_act || bnstats) ? GEMM_FWD : q.op % 3;
    pl.operand_mode = h16 ? 0 : kn.operand_mode;
    const int Ho = (q.H + 2 * q.pad - q.R) / q.stride + 1, Wo = (q.W + 2 * q.pad - q.S) / q.stride + 1;

    // the channel-multiple rules: fp32 storage moves 16-byte pieces (4 floats), the 16-bit kernels 8 elements of the row-
    // contiguous operand and whole 64-element k-tiles of the K-contiguous one (they have the uniform walk only)
    const int kmult = h16 ? 64 : 4, omult = h16 ? 8 : 4;
    bool ok;
    if (pl.mode == GEMM_FWD) ok = q.C % kmult == 0 && (!h16 || q.K % omult == 0) && q.N > 0 && (!linear_op || q.W > 0);
    else if (pl.mode == GEMM_DGRAD) ok = q.K % kmult == 0 && q.C % omult == 0;
    else ok = q.C % omult == 0 && q.K % omult == 0;
    if (h16 && pl.mode == GEMM_DGRAD) ok = ok && (q.stride == 1 || (q.stride == 2 && q.H % 2 == 0 && q.W % 2 == 0));
    if (h16 && bias_act) ok = ok && Ho > 0 && Wo > 0;
    // the three tensors stay below the out-of-bounds sentinel of the buffer descriptors
    const size_t x_bytes = (size_t)q.N * q.H * q.W * q.C * f.elem_bytes, y_bytes = (size_t)q.N * Ho * Wo * q.K * f.elem_bytes,
                 w_bytes = (size_t)q.K * q.R * q.S * q.C * f.elem_bytes;
    if (!ok || x_bytes >= GEMM_OOB || y_bytes >= GEMM_OOB || w_bytes >= GEMM_OOB) return GEMM_ERR_ARG;

    pl.bk = f.wgrad_bk;
    pl.walk = 1;
    pl.splits = 1;
    if (pl.mode == GEMM_WGRAD) {
        pl.Mg = q.K; pl.Ng = q.R * q.S * q.C; pl.Kg = q.N * Ho * Wo;
        const int rows = gemm_wgrad_rows(q.N, Ho, Wo, pl.bk);
        if (h16 && rows < 0) return GEMM_ERR_ARG;
        pl.walk = rows >= 0 && !(kn.dbg & 0x80);
        pl.wg_rows = pl.walk ? rows : 0;
        // fp32 storage: "linear" is the entry point; 16-bit storage: any single-row problem
        if (const int rc = gemm_plan_wgrad(q, kn, h16 ? q.N * Ho == 1 : linear_op, pl)) return rc;
    } else {
        if (pl.mode == GEMM_FWD) {
            pl.Mg = q.N * Ho * Wo; pl.Ng = q.K; pl.Kg = q.R * q.S * q.C;
        } else if (!linear_op && q.stride == 2 && q.H % 2 == 0 && q.W % 2 == 0) {
            // stride-2 dgrad: the four input-pixel parity classes in grid_y of ONE launch (each class only visits the taps that
            // hit a real output pixel; its parameters are derived in the kernel).  The plan describes the largest class.
            pl.nclass = 4;
            pl.Mg = q.N * (q.H / 2) * (q.W / 2); pl.Ng = q.C; pl.Kg = ((q.R + 1) / 2) * ((q.S + 1) / 2) * q.K;
        } else {
            pl.Mg = q.N * q.H * q.W; pl.Ng = q.C; pl.Kg = q.R * q.S * q.K;
        }
        gemm_pick_tile(h16, pl.Mg, pl.Ng, h16 && pl.nclass ? pl.nclass : 1, kn, &pl.BM, &pl.BN);
        pl.slab_elems = (size_t)pl.Mg * pl.Ng;
        if (bnstats) {  // the size ds6g_h16_conv_bnstats_workspace_bytes states (64-row tiles), also where 128-row tiles need half
            if (q.ws_bytes < (size_t)gemm_cdiv(pl.Mg, 64) * 2 * q.K * sizeof(double)) return GEMM_ERR_WORKSPACE;
            pl.ws_bytes_used = (size_t)gemm_cdiv(pl.Mg, pl.BM) * 2 * q.K * sizeof(double);
        }
        if (!h16) {
            const int kch = pl.mode == GEMM_FWD ? q.C : q.K;  // a k-tile never straddles a filter tap
            pl.walk = kch % 16 == 0 && !(kn.dbg & 0x80);
            // 32-column k-tiles wherever the uniform walk allows them.  bf16 operand modes: one MFMA per 16 columns makes the
            // k-tile bookkeeping the bottleneck; fp32: pays on the small-spatial conv layers only (measured, tools/bench_igemm.py)
            const bool wide = kn.operand_mode ? kn.bf16_bk32 != 0
                                              : (kn.f32_bk32 == 1 || (kn.f32_bk32 == 2 && !linear_op && q.R * q.S > 1 &&
                                                                      gemm_cdiv(pl.Mg, 64) * gemm_cdiv(pl.Ng, 64) <= 1024));
            if (pl.walk && kch % 32 == 0 && wide) pl.bk = 32;
        }
        pl.k_per_split = (int)gemm_cdiv(pl.Kg, f.k_round) * f.k_round;
    }
    if ((size_t)pl.Mg * pl.Ng * sizeof(float) >= GEMM_OOB) return GEMM_ERR_ARG;

    pl.tile = h16 ? (pl.BM == 128 ? 0 : 1) : (pl.BN == 128 ? 0 : pl.BM == 128 ? 1 : 2);
    if (pl.mode != GEMM_WGRAD) {
        pl.out16 = h16 && (bias_act || bnstats || q.out16);
        // fp32 storage: the row remap of the parity classes lives in the fused epilogue
        pl.epilogue = (h16 && bias_act) ? 2 : (q.epilogue || (!h16 && pl.nclass > 1));
    }
    pl.tiles_n = (int)gemm_cdiv(pl.Ng, pl.BN);
    pl.grid_x = (int)gemm_cdiv(pl.Mg, pl.BM) * pl.tiles_n;
    pl.grid_y = pl.nclass > 1 ? pl.nclass : 1;
    pl.grid_z = pl.splits;
    if (!h16) pl.variant = 10000 * (pl.bk == 32) + 1000 * pl.epilogue + 100 * pl.walk + 10 * pl.mode + pl.tile;
    else pl.variant = pl.epilogue == 2 ? 30200 + pl.tile : 30000 + 100 * pl.out16 + 10 * pl.mode + pl.tile;
    *out = pl;
    return 0;
}

// The kernel parameters that the problem and the plan determine, for IgemmParams and BgemmParams alike (same field names);
// the entry point adds its pointers and epilogue values.
template <class P>
void gemm_fill_params(P& p, const GemmProblem& q, const GemmPlan& pl) {
    p = P{};
    p.N = q.N; p.H = q.H; p.W = q.W; p.C = q.C; p.K = q.K; p.R = q.R; p.S = q.S; p.stride = q.stride; p.pad = q.pad;
    p.Ho = (q.H + 2 * q.pad - q.R) / q.stride + 1;
    p.Wo = (q.W + 2 * q.pad - q.S) / q.stride + 1;
    p.drop_scale = 1.f;
    p.h0 = 0; p.hstep = 1; p.Hs = q.H; p.w0 = 0; p.wstep = 1; p.Ws = q.W;
    p.r0 = 0; p.rstep = 1; p.nr = q.R; p.s0 = 0; p.sstep = 1; p.ns = q.S;
    if (pl.nclass > 1) {  // host-side values describe the largest class; the kernel derives each class's own
        p.nclass = pl.nclass;
        p.hstep = 2; p.Hs = q.H / 2; p.wstep = 2; p.Ws = q.W / 2; p.rstep = 2; p.sstep = 2;
        p.nr = (q.R + 1) / 2; p.ns = (q.S + 1) / 2;
    }
    p.Mg = pl.Mg; p.Ng = pl.Ng; p.Kg = pl.Kg;
    // sizes of the a_src / b_src tensors for the buffer descriptors: fwd x, w; dgrad dy, w; wgrad dy, x
    const size_t eb = GEMM_FAMILY[pl.family == DS6G_GEMM_H16].elem_bytes, x = (size_t)q.N * q.H * q.W * q.C * eb,
                 y = (size_t)q.N * p.Ho * p.Wo * q.K * eb, w = (size_t)q.K * q.R * q.S * q.C * eb;
    p.a_bytes = (unsigned)(pl.mode == GEMM_FWD ? x : y);
    p.b_bytes = (unsigned)(pl.mode == GEMM_WGRAD ? x : w);
    p.accumulate = pl.mode == GEMM_WGRAD ? 0 : q.accumulate;  // a wgrad accumulates in the slab reduction
    p.tiles_n = pl.tiles_n;
    if (pl.mode == GEMM_WGRAD) {
        p.k_per_split = pl.k_per_split;
        p.split_stride = pl.slab_elems;
        p.wg_rows = pl.wg_rows;
        p.want_colsum = pl.want_colsum;
        p.xcd_splits = pl.xcd_splits;
    }
}

// steps 3 and 4 of every entry point: plan the problem (a refusal is reported and returned), then fill the kernel parameters
template <class P>
int gemm_plan_params(const GemmProblem& q, const GemmKnobs& kn, GemmPlan& pl, P& p) {
    if (const int rc = gemm_plan(q, kn, &pl)) {
        fprintf(stderr, "[ds6g] gemm_plan refuses op %d of family %d, N %d H %d W %d C %d K %d R %d S %d stride %d pad %d: code %d\n",
                q.op, q.family, q.N, q.H, q.W, q.C, q.K, q.R, q.S, q.stride, q.pad, rc);
        return rc;
    }
    gemm_fill_params(p, q, pl);
    return 0;
}

// runs f(std::integral_constant<int, I>) for the I in [0, n) that equals `code`: the runtime plan -> a template instantiation
template <class F, int... I>
bool gemm_dispatch(int code, F&& f, std::integer_sequence<int, I...>) {
    return ((code == I ? (f(std::integral_constant<int, I>{}), true) : false) || ...);
}

#endif  // DS6G_GEMM_PLAN_H
