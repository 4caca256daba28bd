/* Descriptor structs of the batched entry points of ds6g.h and the attention launch plan, in a header of their own so that
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

#endif /* DS6G_TYPES_H */
