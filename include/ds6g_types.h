/* Descriptor structs of the batched entry points of ds6g.h and the attention, GEMM and Winograd launch plans, in a header of their own so that
 * the public header and the kernel sources (csrc/common.h) share ONE definition.  The host reads a caller's descriptor
 * array during the call and hands the descriptors to the kernel by value, in its arguments. */
#ifndef DS6G_TYPES_H
#define DS6G_TYPES_H

#define DS6G_LN_FINALIZE_MAX 24
/* one LayerNorm of ds6g_layernorm_finalize_batched */
typedef struct {
    const float* partial; /* [nblk][2 C] row-block partials written by ds6g_layernorm_bwd_partial / _h16_partial */
    int nblk, C;
    float* dgamma;
    float* dbeta;
    int accumulate;
} ds6g_ln_finalize_desc;
/* one modality map of the grouped stage-glue entry points (ds6g_*3) */
typedef struct {
    const void* in; /* the map read (nullable where the single-map entry point allows it) */
    void* out;      /* the map written (unused by the kernels that write tokens) */
    int frames_per_sample, mod_off;
} ds6g_map_desc;

/* one direction of the grouped forward-only Mamba kernels (ds6g_mamba_conv_fwd_grouped / ds6g_mamba_scan_fwd_grouped and
 * their ds6g_h16_ forms): a launch covers ndir = 1 or 2 of them, each with operands, row strides and walk direction of its own */
#define DS6G_MAMBA_MAX_DIR 2
typedef struct {
    const void* x;     /* [B L][D] of the storage type, a column block of a wider buffer: row stride ld_x elements */
    const float* w;    /* conv1d.weight [D][1][4] */
    const float* bias; /* conv1d.bias [D] */
    void* y;           /* [B L][D] of the storage type, contiguous */
    int ld_x, reverse;
} ds6g_mamba_conv_dir;
typedef struct {
    const void* u;      /* the conv's output xc, [B L][D] of the storage type, row stride ld_u elements */
    const void* z;      /* the gate half of in_proj's output, same type, row stride ld_z */
    const float* x_dbl; /* fp32 [B L][>= r + 32], row stride ld_x: dt = columns [0, r), Bm = [r, r + 16), Cm = [r + 16, r + 32) */
    const float* dt_w;  /* dt_proj.weight [D][r] */
    const float* dt_b;  /* dt_proj.bias [D] */
    const float* A_log; /* [D][16] */
    const float* D;     /* [D] */
    void* y;            /* [B L][D] of the storage type, contiguous */
    int ld_u, ld_z, ld_x, reverse;
} ds6g_mamba_scan_dir;

/* ---- the launch plan of one attention call (ds6g_attention_plan; csrc/attention.hip plans every call with it, then runs it) */
#define DS6G_ATTN_MAX_STEPS 8
/* operand storage of the three entry-point pairs */
enum { DS6G_ATTN_KIND_F32 = 0,     /* ds6g_attention_fwd / _bwd */
       DS6G_ATTN_KIND_OUT16 = 1,   /* _fwd_bf16out / _bwd_bf16: fp32 q / k / v / dO, 16-bit o and gradients */
       DS6G_ATTN_KIND_H16 = 2 };   /* _fwd_h16 / _bwd_h16io: every operand 16-bit */
/* kernel family of a step */
enum { DS6G_ATTN_FWD = 0, DS6G_ATTN_FWD_MERGE, DS6G_ATTN_DELTA, DS6G_ATTN_DQ_RECOMPUTE, DS6G_ATTN_DKV_RECOMPUTE,
       DS6G_ATTN_DKV_HANDOVER, DS6G_ATTN_DKV_FUSED128, DS6G_ATTN_DK_TWO_PASS, DS6G_ATTN_DV_FROM_P, DS6G_ATTN_DQ_FROM_DS,
       DS6G_ATTN_SLAB_SUM };
/* tensors a step writes.  ML: the split forward's (max, sum) partials, merged into lse; HS / HP: the dS / dropped-P tiles
 * the hand-over forms pass from the dK(/dV) kernel to the dQ / dV kernels through the front of the workspace */
enum { DS6G_ATTN_T_O = 0, DS6G_ATTN_T_ML, DS6G_ATTN_T_DQ, DS6G_ATTN_T_DK, DS6G_ATTN_T_DV, DS6G_ATTN_T_DELTA, DS6G_ATTN_T_HS,
       DS6G_ATTN_T_HP, DS6G_ATTN_T_COUNT };
/* what ran */
enum { DS6G_ATTN_FORM_FWD = 0, DS6G_ATTN_FORM_RECOMPUTE, DS6G_ATTN_FORM_HANDOVER, DS6G_ATTN_FORM_HANDOVER_FUSED128,
       DS6G_ATTN_FORM_HANDOVER_TWO_PASS };
typedef struct {
    int tensor;        /* DS6G_ATTN_T_* */
    int slabs;         /* 0: the step writes the caller's tensor itself.  > 0 in a kernel step: it writes ws[off, off + bytes)
                        * instead - one slab per split (1 for hand-over tiles).  > 0 in a merge / slab-sum step: it reduces
                        * that many slabs of ws[off, off + bytes) into the caller's tensor */
    size_t off, bytes;
} ds6g_attn_out;
typedef struct {
    int family;                  /* DS6G_ATTN_* */
    int splits, tiles_per_split; /* of a kernel's key (query) loop; 0 in delta / merge / slab-sum steps */
    int nout;                    /* tensors written; in a slab-sum step: its (slabs, tensor) pairs */
    ds6g_attn_out out[3];
} ds6g_attn_step;
typedef struct {
    int form;                    /* DS6G_ATTN_FORM_* */
    int merged_sum;              /* hand-over: ONE slab sum after the dQ kernel reduces the dK, dV and dQ slabs */
    int nsteps;
    int slab_sums;               /* slab-sum steps = what ds6g_last_attention_bwd_slab_sums reports after the call */
    size_t handover_bytes;       /* the hand-over forms keep ws[0, handover_bytes) for the tiles; slabs start behind it */
    ds6g_attn_step steps[DS6G_ATTN_MAX_STEPS];
} ds6g_attn_plan;

/* ---- the launch of one conv / linear GEMM call, fully decided (ds6g_gemm_plan; csrc/gemm_plan.h plans every call of
 * csrc/igemm.hip and csrc/bgemm.hip with it, then the entry point runs it).  DESIGN.md 3.1 has the table of the rules. */
enum { DS6G_GEMM_F32 = 0,  /* fp32 storage: ds6g_conv2d_* / ds6g_linear_* */
       DS6G_GEMM_H16 = 1 }; /* 16-bit storage: ds6g_h16_conv2d_* / ds6g_h16_linear_* */
/* the entry point; a linear over M rows is the 1x1 conv of ONE 1 x M image: N = H = 1, W = M, C = in, K = out features */
enum { DS6G_GEMM_CONV_FWD = 0, DS6G_GEMM_CONV_DGRAD, DS6G_GEMM_CONV_WGRAD, DS6G_GEMM_LINEAR_FWD, DS6G_GEMM_LINEAR_DGRAD,
       DS6G_GEMM_LINEAR_WGRAD, DS6G_GEMM_CONV_BIAS_ACT_FWD, DS6G_GEMM_CONV_FWD_BNSTATS /* 16-bit storage only */ };
/* what of a call's arguments besides the shape decides its launch (the `flags` of the query).  EPILOGUE: a fused epilogue
 * is needed (any of bias, ReLU, ReLU mask, dropout, residual; the 16-bit inference conv always has its own) */
enum { DS6G_GEMM_EPILOGUE = 1, DS6G_GEMM_OUT16 = 2, DS6G_GEMM_ACCUMULATE = 4, DS6G_GEMM_DBIAS = 8 };
struct ds6g_gemm_plan {
    int family;                  /* DS6G_GEMM_F32 / _H16 */
    int mode;                    /* the kernel's product: 0 fwd, 1 dgrad, 2 wgrad */
    int operand_mode;            /* fp32 storage: ds6g_set_compute_mode's matrix-core mode 0 .. 3 (the BF template value); else 0 */
    int Mg, Ng, Kg;              /* GEMM extents; of the largest parity class where nclass > 1 */
    int BM, BN, bk;              /* output tile and k-tile depth (16 / 32 fp32 storage, 64 16-bit storage) */
    int tile;                    /* the tile's code in `variant`: fp32 storage 0 128x128, 1 128x64, 2 64x64; 16-bit 0 128x128, 1 64x64 */
    int walk;                    /* 1 wave-uniform k walk, 0 general walk (fp32 storage only) */
    int epilogue;                /* 0 plain store, 1 fused epilogue, 2 the 16-bit inference conv's */
    int out16;                   /* 16-bit output (16-bit storage, fwd / dgrad) */
    int nclass;                  /* 4: the parity classes of a stride-2 dgrad in grid_y; else 0 */
    int grid_x, grid_y, grid_z;  /* grid_x = cdiv(Mg, BM) * tiles_n, grid_y = max(nclass, 1), grid_z = splits */
    int tiles_n;                 /* cdiv(Ng, BN) */
    int splits, k_per_split;     /* wgrad: split-K; else 1 and Kg rounded up */
    int wg_rows;                 /* uniform wgrad walk: 0 = a k-tile stays inside one output row, else output rows per k-tile */
    int xcd_splits;              /* wgrad: the XCD-contiguous (split, tile) mapping */
    int want_colsum;             /* wgrad: bias-gradient column sums behind each slab */
    int reduce;                  /* wgrad: the kernel writes `splits` slabs into the workspace and the slab reduction follows */
    int variant;                 /* what ds6g_last_igemm_variant and the profile records carry (ds6g.h) */
    size_t slab_elems;           /* Mg * Ng (+ Mg with want_colsum): the split stride, in floats */
    size_t ws_bytes_used;        /* splits * slab_elems * 4 where reduce is set; the BatchNorm partials of conv2d_fwd_bnstats; else 0 */
};

/* ---- the launch of one Winograd call, fully decided (ds6g_winograd_plan; csrc/wino_plan.h plans every call of
 * csrc/winograd.hip with it, then the entry point runs it).  DESIGN.md 3.1b has the table of the rules. */
enum { DS6G_WINO_FWD = 0,      /* ds6g_conv3x3_winograd_fwd: the forward; on dy and the dgrad filter the data gradient */
       DS6G_WINO_BIAS_ACT = 1, /* ds6g_conv3x3_winograd_bias_act_fwd */
       DS6G_WINO_WGRAD = 2 };  /* ds6g_conv3x3_winograd_wgrad */
enum { DS6G_WINO_K_FWD1 = 0,   /* winograd_fwd_kernel<1>: one workgroup per 32 tiles x 32 output channels */
       DS6G_WINO_K_FWD2 = 1,   /* winograd_fwd_kernel<2>: 64 output channels (debug flag 0x02000000) */
       DS6G_WINO_K_PC = 2,     /* winograd_pc_kernel: persistent producer / consumer workgroups over 32-tile x 64-channel items */
       DS6G_WINO_K_WGRAD = 3 };/* winograd_wgrad_kernel (+ winograd_wgrad_finish_kernel over the split slabs) */
struct ds6g_wino_plan {
    int op, kernel;              /* DS6G_WINO_*, DS6G_WINO_K_* */
    int TH, TW;                  /* tiles per image column / row: H / 2, W / 2 */
    int BTW, BTH;                /* conv forms: tile columns / rows per tile block, BTW * BTH = 32 */
    int rows_total;              /* N * TH */
    int row_blocks, col_blocks;  /* cdiv(rows_total, BTH), TW / BTW */
    int items, rounds;           /* persistent kernel: tile blocks x K / 64 items in cdiv(items, CUs - reserve) rounds; else 0 */
    int grid_x, grid_y, grid_z;  /* persistent: cdiv(items, rounds); fwd<TNK>: tile blocks x K / (32 TNK); wgrad: (K/64 C/64, 4, splits) */
    int block, lds_bytes;        /* threads per workgroup; dynamic LDS (the persistent kernel's 128 KiB, else 0) */
    int xcd;                     /* persistent: gk of the XCD item order (0: plain order); wgrad: the XCD-contiguous order's flag */
    int btw_shift;               /* persistent: log2(BTW) */
    unsigned th_magic;           /* persistent: ceil(2^32 / TH): row / TH = umulhi(row, th_magic) */
    unsigned x_bytes, u_bytes, dy_bytes; /* sizes behind the buffer resources: x; U (conv forms); dy (wgrad) */
    int tiles_total;             /* wgrad: N * TH * TW */
    int splits, tiles_per_split; /* wgrad: splits of the tile range, each a multiple of 16 tiles, none empty */
    int variant;                 /* the profile record's: 20000 winograd_fwd_kernel, 20001 wgrad, 20002 persistent */
    double flops;                /* the profile record's: 2 N H W K 9 C, the direct convolution's */
    size_t ws_bytes_used;        /* wgrad: splits slabs of 16 K C floats */
};

#endif /* DS6G_TYPES_H */
