// The launch planner of the Winograd entry points of winograd.hip.  Every entry point states its call as a WinoProblem,
// wino_plan() decides the launch - refusals, tile-block geometry, kernel, items / rounds / grid of the persistent kernel, its XCD
// item order, the division constants, the wgrad splits, the profile variant - as a pure function of (problem, knobs), and the
// entry point runs exactly what it returns; ds6g_winograd_plan (ds6g.h) shows the same plan to tests without a launch.
// DESIGN.md 3.1b has the rules as one table.  Plain host C++17: no HIP include, nothing __device__.
#pragma once
#include <cstddef>
#include "../../include/ds6g_types.h"

typedef struct ds6g_wino_plan WinoPlan;

constexpr int WINO_ERR_ARG = 1, WINO_ERR_LAUNCH = 2, WINO_ERR_WORKSPACE = 3;  // DS6G_ERR_* (common.h)
// the kernels' tile constants (winograd.hip asserts them equal to its own): 32 tiles x 32 channels per MFMA block, 16-channel
// chunks, 64 channels per persistent item; wgrad: 16 tiles per chunk, 64 x 64 channels per workgroup
constexpr int WINO_TILES = 32, WINO_KB = 32, WINO_CH = 16, WINO_PC_KB = 64, WINO_WW_T = 16, WINO_WW_CB = 64;
constexpr int WINO_PC_LDS_BYTES = (2 * 16 * WINO_TILES * WINO_CH + 4 * 2 * WINO_TILES * WINO_PC_KB) * 4;  // two V images + S
// A PLAIN buffer resource (base = the tensor: x and U of winograd_fwd_kernel, U of winograd_pc_kernel, dy of
// winograd_wgrad_kernel) marks an out-of-image lane with the offset OOB_OFF (common.h): the tensor must end below it.
constexpr size_t WINO_PLAIN_END = 0x80000000u;
// The SHIFTED x resource of winograd_pc_kernel and winograd_wgrad_kernel (base = x - (W + 1) C floats) marks "row outside" and
// "column outside" by adding 2^30 each (the kernels' BAD): x plus its (W + 1) C lead must end below 2^30.
constexpr size_t WINO_SHIFTED_END = 0x40000000u;

// what the caller asked for; op: DS6G_WINO_*
struct WinoProblem { int op, N, H, W, C, K, accumulate; size_t ws_bytes; };

// every input of the decision that is not the problem (winograd.hip: wino_knobs reads the environment once per process)
struct WinoKnobs {
    int n_cu = 0;        // CUs of the current device = persistent workgroups; <= 0: unknown (a persistent plan then fails)
    int kb64 = 0;        // ds6g_set_debug_flags 0x02000000: winograd_fwd_kernel<2> where the persistent kernel does not run
    int pc = 1;          // DS6G_WINO_PC: 0 never plans the persistent producer / consumer kernel
    int cu_reserve = 0;  // DS6G_PC_CU_RESERVE: CUs left to other resident kernels (RCCL channels under data parallelism)
    int pc_xcd = -1;     // DS6G_PC_XCD: -1 pick gk by cost, 0 plain item order, 1 / 2 / 4 / 8 force gk
    int ww_xcd = 1;      // DS6G_WW_XCD: 0 switches the XCD-contiguous wgrad workgroup order off
};

inline long wino_cdiv(long a, long b) { return (a + b - 1) / b; }
inline size_t wino_bytes(int N, int H, int W, int C) { return (size_t)N * H * W * C * 4; }               // an NHWC fp32 tensor
inline size_t wino_slab(int K, int C) { return (size_t)16 * K * C * 4; }                                 // U, or one dU slab
inline bool wino_shifted_x_ok(int N, int H, int W, int C) { return wino_bytes(N, H, W, C) + (size_t)(W + 1) * C * 4 < WINO_SHIFTED_END; }

// the shapes an entry point takes: ds6g_winograd_supported / ds6g_winograd_wgrad_supported are this predicate
// (an empty extent is refused here: the geometry below would divide by zero)
inline bool wino_shape_ok(int op, int N, int H, int W, int C, int K) {
    if (op < DS6G_WINO_FWD || op > DS6G_WINO_WGRAD || H % 2 || W % 2 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0) return false;
    if (op == DS6G_WINO_WGRAD)
        return C % WINO_WW_CB == 0 && K % WINO_WW_CB == 0 && wino_shifted_x_ok(N, H, W, C) && wino_bytes(N, H, W, K) < WINO_PLAIN_END;
    const int TW = W / 2;
    return C % WINO_CH == 0 && K % WINO_KB == 0 && (TW >= 8 ? TW % 8 == 0 : WINO_TILES % TW == 0) &&
           wino_bytes(N, H, W, C) < WINO_PLAIN_END && wino_slab(K, C) < WINO_PLAIN_END;
}

// the persistent kernel runs 64-channel items over at least two chunks, through the shifted x resource
inline bool wino_wants_pc(const WinoProblem& q, const WinoKnobs& kn) {
    return q.op != DS6G_WINO_WGRAD && kn.pc && q.K % WINO_PC_KB == 0 && q.C >= 2 * WINO_CH && wino_shifted_x_ok(q.N, q.H, q.W, q.C);
}

// weight gradient: ~1024 workgroups, at least 12 chunks per split, bounded by the scratch; then no empty split
inline int wino_plan_wgrad(const WinoProblem& q, const WinoKnobs& kn, WinoPlan& pl) {
    const size_t slab = wino_slab(q.K, q.C);
    if (q.ws_bytes < slab) return WINO_ERR_WORKSPACE;
    pl.kernel = DS6G_WINO_K_WGRAD;
    pl.variant = 20001;
    pl.dy_bytes = (unsigned)wino_bytes(q.N, q.H, q.W, q.K);
    pl.tiles_total = q.N * pl.TH * pl.TW;
    pl.grid_x = (q.K / WINO_WW_CB) * (q.C / WINO_WW_CB);
    pl.grid_y = 4;
    const long chunks = wino_cdiv(pl.tiles_total, WINO_WW_T);
    long splits = wino_cdiv(1024, pl.grid_x * 4);
    if (splits > chunks / 12) splits = chunks / 12;
    if (splits > (long)(q.ws_bytes / slab)) splits = (long)(q.ws_bytes / slab);
    if (splits < 1) splits = 1;
    const long cps = wino_cdiv(chunks, splits);
    pl.tiles_per_split = (int)cps * WINO_WW_T;
    pl.grid_z = pl.splits = (int)wino_cdiv(chunks, cps);
    pl.xcd = kn.ww_xcd;
    pl.ws_bytes_used = pl.splits * slab;
    return 0;
}

// -> 0 and *out, or the entry point's refusal
inline int wino_plan(const WinoProblem& q, const WinoKnobs& kn, WinoPlan* out) {
    if (!out || !wino_shape_ok(q.op, q.N, q.H, q.W, q.C, q.K)) return WINO_ERR_ARG;
    WinoPlan pl = {};
    pl.op = q.op;
    pl.TH = q.H / 2; pl.TW = q.W / 2;
    pl.x_bytes = (unsigned)wino_bytes(q.N, q.H, q.W, q.C);
    pl.flops = 2.0 * q.N * q.H * q.W * (double)q.K * 9.0 * q.C;  // those of the direct 3x3 convolution it replaces
    pl.variant = 20000;
    pl.grid_y = pl.grid_z = 1;
    pl.block = 256;
    if (q.op == DS6G_WINO_WGRAD) {
        if (const int rc = wino_plan_wgrad(q, kn, pl)) return rc;
        *out = pl;
        return 0;
    }
    pl.BTW = pl.TW >= 8 ? 8 : pl.TW;
    pl.BTH = WINO_TILES / pl.BTW;
    pl.rows_total = q.N * pl.TH;
    pl.row_blocks = (int)wino_cdiv(pl.rows_total, pl.BTH);
    pl.col_blocks = pl.TW / pl.BTW;
    pl.u_bytes = (unsigned)wino_slab(q.K, q.C);
    const long blocks = (long)pl.row_blocks * pl.col_blocks;
    if (!wino_wants_pc(q, kn)) {
        pl.kernel = (q.K % (2 * WINO_KB) == 0 && kn.kb64) ? DS6G_WINO_K_FWD2 : DS6G_WINO_K_FWD1;
        pl.grid_x = (int)(blocks * (q.K / (pl.kernel == DS6G_WINO_K_FWD2 ? 2 * WINO_KB : WINO_KB)));
        *out = pl;
        return 0;
    }
    if (kn.n_cu <= 0) return WINO_ERR_LAUNCH;
    pl.kernel = DS6G_WINO_K_PC;
    pl.variant = 20002;
    pl.block = 512;
    pl.lds_bytes = WINO_PC_LDS_BYTES;
    const int kblocks = q.K / WINO_PC_KB;
    pl.items = (int)blocks * kblocks;
    pl.btw_shift = __builtin_ctz((unsigned)pl.BTW);
    pl.th_magic = (unsigned)(((1ull << 32) + (unsigned)pl.TH - 1) / (unsigned)pl.TH);
    // one persistent workgroup per CU that is not reserved (a workgroup needs a whole CU: all its VGPRs, 128 KiB of LDS; beside
    // other resident kernels a full-size grid would run its last workgroups in a second round), then the smallest grid that
    // needs no more rounds than all those CUs would: at the model's batch (60 frames) every layer has a multiple of 240
    // items, so 240 workgroups are as fast as 256 (measured: 175.5 vs 176.1 samples/s) and 16 CUs stay free
    const int cus = kn.n_cu - kn.cu_reserve > 1 ? kn.n_cu - kn.cu_reserve : 1;
    pl.rounds = (pl.items + cus - 1) / cus;
    pl.grid_x = (pl.items + pl.rounds - 1) / pl.rounds;
    // XCD-aware item order (see the kernel): gk channel-block groups x gt = 8 / gk tile-block groups of XCDs; per launch the L2s
    // then fetch about |U| gt + |x| gk bytes (every XCD of a tile-block group reads that group's x once per channel group it is
    // in; every U slice is read by the gt XCDs that share it) - the minimum wins
    const bool xcd_order = kn.pc_xcd != 0 && pl.grid_x % 8 == 0 && pl.items % pl.grid_x == 0;
    double best = 0;
    for (int gk = 1; xcd_order && gk <= 8; gk *= 2) {
        const int gt = 8 / gk;
        if (kblocks % gk || blocks % gt || (kn.pc_xcd > 0 && gk != kn.pc_xcd)) continue;
        const double cost = (double)pl.u_bytes * gt + (double)pl.x_bytes * gk;
        if (!pl.xcd || cost < best) { best = cost; pl.xcd = gk; }
    }
    *out = pl;
    return 0;
}
