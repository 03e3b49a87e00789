/* =============================================================================
 * dbg_mi355x_groups.h -- companion of dbg_mi355x.h (ABI 7): the grouped-observation export, so that filter_kmers can run with
 * any KmerSummarizer.  Same conventions as dbg_mi355x.h (0 = success, dbg_last_error, library-allocated outputs released
 * with the matching dbg_free_* call).  The Rust binding is integration/dbg_mi355x_groups_sys.rs (tools/gen_rust_ffi.py --groups).
 * ========================================================================== */
#ifndef DBG_MI355X_GROUPS_H
#define DBG_MI355X_GROUPS_H

#include "dbg_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- grouped k-mer observations: filter_kmers with any KmerSummarizer (src/filter.rs:27-35, :139-231) ----------------
 * Everything the reference hands to S::summarize, group by group, for a range [bucket_lo, bucket_hi) of its 256 buckets
 * (filter.rs:18-23: the canonical k-mer's first four bases = the top byte of its 2k key bits): the distinct canonical k-mers
 * in ascending order, and per k-mer its observations (Exts, D1) in input order -- the order sort_by_key, a stable sort, leaves
 * them in (filter.rs:205-211).  A caller runs its own summarizer over the groups on the host.  Passes over ascending bucket
 * ranges concatenate to the whole input; dbg_kmer_groups_plan_dev cuts the ranges so that one pass stays under 2^32
 * observations and fits the scratch budget (dbg_ctx_set_scratch_budget).  Per observation a pass needs about 2 x (key + 4)
 * bytes of sort records, 5 bytes of instance arrays and 13 bytes of grouping scratch and output (+ about 40 bytes per group). */
typedef struct {
    uint32_t k;                 /* 4 <= k <= 64 (as dbg_filter_params) */
    int32_t  stranded;          /* filter.rs:142: !stranded = canonical k-mers, an observation's Exts flipped with its k-mer */
    uint32_t bucket_lo, bucket_hi;      /* 0 <= lo < hi <= 256 */
    uint64_t min_obs_export;    /* 0 = every group's observations.  Otherwise a group of fewer observations keeps its key, nobs and
                                   exts_or, but its observation segment is empty -- only right for a summarizer that rejects such
                                   groups anyway (CountFilter-like min counts); what it saves is the error k-mers' observations */
    int32_t  obs_seq_index;     /* 1: obs_data holds the index of each observation's source sequence instead of its D1 (for a D1
                                   that is no integer: the caller looks its value up; more than 2^32 sequences are an error) */
} dbg_group_params;

typedef struct {
    uint64_t  n;                /* distinct k-mers of the range */
    uint64_t* key_hi;           /* [n] zero when k <= 32 */
    uint64_t* key_lo;           /* [n] ascending (hi, lo) */
    uint32_t* nobs;             /* [n] observations of the k-mer (exact, whatever min_obs_export) */
    uint8_t*  exts_or;          /* [n] OR of the observations' Exts */
    uint64_t* obs_off;          /* [n + 1] observations of group i: obs_off[i] .. obs_off[i + 1] (empty below min_obs_export) */
    uint8_t*  obs_exts;         /* [n_obs] Exts of each observation, in input order within its group */
    uint32_t* obs_data;         /* [n_obs] D1 zero-extended to u32 (or the sequence index); NULL when D1 is unit and no index asked */
    uint64_t  n_obs;            /* = obs_off[n] */
    uint64_t  n_kmer_instances; /* k-mer instances of the range = the sum of nobs */
    uint32_t  bucket_lo, bucket_hi;
    int32_t   on_device;        /* 1 when the arrays are device pointers */
} dbg_kmer_groups;

/* Ascending bucket ranges for the passes: bounds[0] = 0 < bounds[1] < ... < bounds[*n_passes] = 256, each range at most
 * max_obs_per_pass k-mer instances (0 = what the device's budget allows, at most 2^32 - 1).  A bucket that alone exceeds a pass is
 * an error. */
int  dbg_kmer_groups_plan_dev(dbg_ctx* ctx, const dbg_seqset* dev_seqs, uint32_t k, int stranded, uint64_t max_obs_per_pass,
                              uint32_t* bounds /* [257] */, uint32_t* n_passes);
/* One pass: the groups of [p->bucket_lo, p->bucket_hi), device arrays (release with dbg_free_groups). */
int  dbg_kmer_groups_dev(dbg_ctx* ctx, const dbg_seqset* dev_seqs, const dbg_group_params* p, dbg_kmer_groups* out_dev);
/* copy to host arrays from the ctx's pinned pool (as dbg_table_to_host; release with dbg_free_groups before dbg_ctx_destroy) */
int  dbg_groups_to_host(dbg_ctx* ctx, const dbg_kmer_groups* dev, dbg_kmer_groups* out_host);
void dbg_free_groups(dbg_ctx* ctx, dbg_kmer_groups* g);

#ifdef __cplusplus
}
#endif
#endif /* DBG_MI355X_GROUPS_H */
