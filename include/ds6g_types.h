/* Descriptor structs of the batched entry points of ds6g.h, in a header of their own so that the public header and the
 * kernel sources (csrc/common.h) share ONE definition.  The host reads a caller's descriptor array during the call and hands
 * the descriptors to the kernel by value, in its arguments. */
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

#endif /* DS6G_TYPES_H */
