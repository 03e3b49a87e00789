// Grouped k-mer observations: what filter_kmers hands to KmerSummarizer::summarize (src/filter.rs:27-35, :186-231), group by
// group, for a caller whose summarizer is not one of the two the device runs itself.
//   extract (extract.hip, payload = the record's index in the pass) -> stable LSD radix sort on the key bits alone (radix.hip;
//   a sort on (key, D1) would lose the input order the reference's stable sort_by_key keeps) -> head flags -> scan (group ids)
//   -> group starts and keys -> nobs by differences -> scan of the exported segment sizes -> one per-element pass that gathers
//   each observation's Exts / D1 through its payload and ORs the Exts by a segmented wave reduction.
// No kernel walks a run with one lane: a k-mer with 10^7 observations costs what 10^7 observations of distinct k-mers cost.
#include "dbg_internal.hpp"
#include "../../include/dbg_mi355x_groups.h"
#include <algorithm>

namespace {

template <bool HAS_HI>
__global__ void __launch_bounds__(256) grp_heads_kernel(const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo, uint32_t n,
                                                        uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool h = i == 0;
    if (!h) {
        h = lo[i] != lo[i - 1];
        if (HAS_HI) h = h || hi[i] != hi[i - 1];
    }
    head[i] = h ? 1u : 0u;
}

// gx: exclusive scan of the head flags, [n + 1]; gx[n] = groups
template <bool HAS_HI>
__global__ void __launch_bounds__(256) grp_starts_kernel(const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo, uint32_t n,
                                                         const uint32_t* __restrict__ head, const uint32_t* __restrict__ gx,
                                                         uint32_t* __restrict__ gstart, uint64_t* __restrict__ key_hi,
                                                         uint64_t* __restrict__ key_lo) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) gstart[gx[n]] = n;
    if (i >= n || !head[i]) return;
    const uint32_t g = gx[i];
    gstart[g] = i;
    key_hi[g] = HAS_HI ? hi[i] : 0ull;
    key_lo[g] = lo[i];
}

__global__ void __launch_bounds__(256) grp_nobs_kernel(const uint32_t* __restrict__ gstart, uint32_t ng, uint64_t min_export,
                                                       uint32_t* __restrict__ nobs, uint32_t* __restrict__ cnt, uint32_t* __restrict__ ex32) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ng) return;
    const uint32_t c = gstart[g + 1] - gstart[g];
    nobs[g] = c;
    cnt[g] = (uint64_t)c >= min_export ? c : 0u;
    ex32[g] = 0;
}

// One lane per sorted record.  The Exts OR is a segmented inclusive scan over the wave (group ids ascend along the records, so
// "same id as the lane d below" is the segment test) and the last lane of each segment in the wave does the one atomic.
template <bool HAS_DATA>
__global__ void __launch_bounds__(256) grp_decode_kernel(uint32_t n, const uint32_t* __restrict__ pay, const uint32_t* __restrict__ gx,
                                                         const uint32_t* __restrict__ gstart, const uint32_t* __restrict__ cnt,
                                                         const uint64_t* __restrict__ obs_off, const uint8_t* __restrict__ inst_exts,
                                                         const uint32_t* __restrict__ inst_val, uint32_t* __restrict__ ex32,
                                                         uint8_t* __restrict__ obs_exts, uint32_t* __restrict__ obs_data) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    const bool valid = i < n;
    uint32_t g = 0xffffffffu, q = 0, v = 0;
    if (valid) {
        g = gx[i + 1] - 1;                                              // heads among records 0..i, minus one
        q = pay[i];
        v = inst_exts[q];
    }
    const uint32_t e = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ov = __shfl_up(v, d, 64), og = __shfl_up(g, d, 64);
        if (lane >= (uint32_t)d && og == g) v |= ov;
    }
    const uint32_t gn = __shfl_down(g, 1, 64);
    if (!valid) return;
    if (lane == 63 || gn != g) atomicOr(&ex32[g], v);
    if (cnt[g]) {
        const uint64_t o = obs_off[g] + (i - gstart[g]);
        obs_exts[o] = (uint8_t)e;
        if (HAS_DATA) obs_data[o] = inst_val[q];
    }
}

__global__ void __launch_bounds__(256) grp_exts_kernel(const uint32_t* __restrict__ ex32, uint32_t ng, uint8_t* __restrict__ exts_or) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < ng) exts_or[g] = (uint8_t)ex32[g];
}

constexpr uint64_t PASS_LIMIT = (1ull << 32) - 1;

// bytes of device memory one observation of a pass needs at the peak (sort records a + b, instance arrays, grouping scratch and
// the exported arrays, and the per-group arrays for the worst case of one group per observation)
uint64_t bytes_per_obs(bool has_hi) {
    const uint64_t key = has_hi ? 16 : 8;
    return 2 * (key + 4) + 5 + 8 + 5 + (key + 4 + 1 + 8 + 4 + 4 + 4 + 4);
}
// ... and per input sequence, whatever the pass: its k-mer count (u32) and record offset (u64) in the range
constexpr uint64_t BYTES_PER_SEQ = 4 + 8;

int validate_groups(dbg_ctx* c, const dbg_seqset* s, uint32_t k) {
    if (!s) return c->fail(10, "null argument");
    if (k < 4 || k > 64) return c->fail(11, "k must be in 4..=64 (filter.rs:18-23 reads the first 4 bases)");
    if (s->data && !(s->data_width == 1 || s->data_width == 2 || s->data_width == 4)) return c->fail(14, "data_width must be 1, 2 or 4");
    if (s->n_seqs && (!s->words || !s->start || !s->length)) return c->fail(15, "null sequence arrays");
    return 0;
}
}  // namespace

extern "C" int dbg_kmer_groups_plan_dev(dbg_ctx* c, const dbg_seqset* ds, uint32_t k, int stranded, uint64_t max_obs_per_pass,
                                        uint32_t* bounds, uint32_t* n_passes) {
    DBG_TRY(validate_groups(c, ds, k));
    if (!bounds || !n_passes) return c->fail(10, "null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    SeqDev s{ds->words, ds->start, ds->length, ds->exts, ds->data, ds->data ? ds->data_width : 0u, ds->n_seqs, ds->n_words};
    uint64_t n_kmers = 0;
    DBG_TRY(kmer_total(c, s, (int)k, &n_kmers));
    uint64_t pass_max = PASS_LIMIT;
    if (max_obs_per_pass) pass_max = std::min<uint64_t>(pass_max, max_obs_per_pass);
    else {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            uint64_t budget = c->scratch_budget ? c->scratch_budget : (uint64_t)((free_b + c->pooled_bytes) * 0.6);
            const uint64_t per_seq = (ds->n_seqs + 1) * BYTES_PER_SEQ;
            budget = budget > per_seq ? budget - per_seq : 0;
            pass_max = std::min<uint64_t>(pass_max, std::max<uint64_t>(budget / bytes_per_obs(k > 32), 1u << 20));
        } else (void)hipGetLastError();
    }
    bounds[0] = 0;
    if (n_kmers <= pass_max) { bounds[1] = 256; *n_passes = 1; return 0; }
    DBuf<unsigned long long> d_hist;
    ALLOC_OR_FAIL(c, d_hist, 256);
    DBG_TRY(kmer_top_byte_hist(c, s, (int)k, stranded != 0, d_hist.p));
    unsigned long long hist[256];
    HIP_TRY(c, hipMemcpyAsync(hist, d_hist.p, sizeof(hist), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t np = 0;
    uint64_t acc = 0;
    for (uint32_t b = 0; b < 256; b++) {
        if (hist[b] > pass_max) {
            char m[200];
            snprintf(m, sizeof(m), "kmer groups: bucket %u alone holds %llu k-mer instances, more than a pass can hold (%llu)", b, hist[b],
                     (unsigned long long)pass_max);
            return c->fail(20, m);
        }
        if (acc + hist[b] > pass_max) { bounds[++np] = b; acc = 0; }
        acc += hist[b];
    }
    bounds[++np] = 256;
    *n_passes = np;
    return 0;
}

extern "C" int dbg_kmer_groups_dev(dbg_ctx* c, const dbg_seqset* ds, const dbg_group_params* p, dbg_kmer_groups* out) {
    if (!p || !out) return c->fail(10, "null argument");
    DBG_TRY(validate_groups(c, ds, p->k));
    if (p->bucket_lo >= p->bucket_hi || p->bucket_hi > 256) return c->fail(16, "bucket range must satisfy bucket_lo < bucket_hi <= 256");
    if (p->obs_seq_index && ds->n_seqs > (1ull << 32)) return c->fail(17, "obs_seq_index: more than 2^32 sequences do not fit a u32 index");
    HIP_TRY(c, hipSetDevice(c->device));
    c->t_clear();
    memset(out, 0, sizeof(*out));
    const int k = (int)p->k;
    const bool has_hi = k > 32, stranded = p->stranded != 0;
    const bool full = p->bucket_lo == 0 && p->bucket_hi == 256;
    const bool has_data = p->obs_seq_index || (ds->data && ds->data_width);
    SeqDev s{ds->words, ds->start, ds->length, ds->exts, ds->data, ds->data ? ds->data_width : 0u, ds->n_seqs, ds->n_words};

    // records of the range, per sequence in input order
    DBuf<uint32_t> kcount;
    DBuf<uint64_t> koff;
    ALLOC_OR_FAIL(c, kcount, std::max<uint64_t>(s.n, 1));
    ALLOC_OR_FAIL(c, koff, s.n + 1);
    if (full) DBG_TRY(kmer_counts(c, s, k, kcount.p));
    else DBG_TRY(kmer_counts_range(c, s, k, stranded, p->bucket_lo, p->bucket_hi, kcount.p));
    DBG_TRY(scan_exclusive_u32_u64(c, kcount.p, koff.p, s.n));
    uint64_t n64 = 0;
    HIP_TRY(c, hipMemcpyAsync(&n64, koff.p + s.n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    kcount.release();
    if (n64 > PASS_LIMIT) return c->fail(20, "kmer groups: the bucket range holds 2^32 or more k-mer instances (plan the passes with dbg_kmer_groups_plan_dev)");
    const uint32_t n = (uint32_t)n64;
    const size_t na = std::max<uint64_t>(n64, 1);

    DBuf<uint64_t> a_hi, a_lo, b_hi, b_lo;
    DBuf<uint32_t> a_pay, b_pay, inst_val;
    DBuf<uint8_t> inst_exts;
    if (has_hi) { ALLOC_OR_FAIL(c, a_hi, na); ALLOC_OR_FAIL(c, b_hi, na); }
    ALLOC_OR_FAIL(c, a_lo, na); ALLOC_OR_FAIL(c, b_lo, na);
    ALLOC_OR_FAIL(c, a_pay, na); ALLOC_OR_FAIL(c, b_pay, na);
    ALLOC_OR_FAIL(c, inst_exts, na);
    if (has_data) ALLOC_OR_FAIL(c, inst_val, na);
    RecArrays A{a_hi.p, a_lo.p, a_pay.p}, B{b_hi.p, b_lo.p, b_pay.p};
    DBG_TRY(extract_kmers_obs(c, s, koff.p, n64, k, stranded, p->bucket_lo, p->bucket_hi, p->obs_seq_index != 0, A, inst_exts.p, inst_val.p));
    koff.release();
    bool in_b = false;
    if (n) DBG_TRY(radix_sort_records(c, n64, A, B, 2 * k, 8, 0, &in_b));          // key bits only: equal keys stay in input order
    const RecArrays R = in_b ? B : A;
    if (in_b) { a_hi.release(); a_lo.release(); a_pay.release(); }
    else { b_hi.release(); b_lo.release(); b_pay.release(); }

    DBuf<uint32_t> head, gx;
    ALLOC_OR_FAIL(c, head, na);
    ALLOC_OR_FAIL(c, gx, na + 1);
    uint32_t ng = 0;
    if (n) {
        c->t_begin("groups_heads", n);
        if (has_hi) grp_heads_kernel<true><<<cdiv(n, 256), 256, 0, c->stream>>>(R.hi, R.lo, n, head.p);
        else grp_heads_kernel<false><<<cdiv(n, 256), 256, 0, c->stream>>>(R.hi, R.lo, n, head.p);
        c->t_end();
        LAUNCH_CHECK(c, "grp_heads");
        DBG_TRY(scan_exclusive_u32(c, head.p, gx.p, n));
        HIP_TRY(c, hipMemcpyAsync(&ng, gx.p + n, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const size_t ga = std::max<uint32_t>(ng, 1);
    DBuf<uint64_t> key_hi, key_lo, obs_off;
    DBuf<uint32_t> gstart, nobs, cnt, ex32, obs_data;
    DBuf<uint8_t> exts_or, obs_exts;
    ALLOC_OR_FAIL(c, key_hi, ga); ALLOC_OR_FAIL(c, key_lo, ga);
    ALLOC_OR_FAIL(c, gstart, (size_t)ng + 1);
    ALLOC_OR_FAIL(c, nobs, ga); ALLOC_OR_FAIL(c, cnt, ga); ALLOC_OR_FAIL(c, ex32, ga);
    ALLOC_OR_FAIL(c, exts_or, ga);
    ALLOC_OR_FAIL(c, obs_off, (size_t)ng + 1);
    uint64_t n_obs = 0;
    if (n) {
        c->t_begin("groups_starts", n);
        if (has_hi) grp_starts_kernel<true><<<cdiv(n, 256), 256, 0, c->stream>>>(R.hi, R.lo, n, head.p, gx.p, gstart.p, key_hi.p, key_lo.p);
        else grp_starts_kernel<false><<<cdiv(n, 256), 256, 0, c->stream>>>(R.hi, R.lo, n, head.p, gx.p, gstart.p, key_hi.p, key_lo.p);
        c->t_end();
        LAUNCH_CHECK(c, "grp_starts");
        head.release();
        grp_nobs_kernel<<<cdiv(ng, 256), 256, 0, c->stream>>>(gstart.p, ng, p->min_obs_export, nobs.p, cnt.p, ex32.p);
        LAUNCH_CHECK(c, "grp_nobs");
    }
    DBG_TRY(scan_exclusive_u32_u64(c, cnt.p, obs_off.p, ng));
    HIP_TRY(c, hipMemcpyAsync(&n_obs, obs_off.p + ng, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ALLOC_OR_FAIL(c, obs_exts, std::max<uint64_t>(n_obs, 1));
    if (has_data) ALLOC_OR_FAIL(c, obs_data, std::max<uint64_t>(n_obs, 1));
    if (n) {
        c->t_begin("groups_decode", n);
        if (has_data) grp_decode_kernel<true><<<cdiv(n, 256), 256, 0, c->stream>>>(n, R.pay, gx.p, gstart.p, cnt.p, obs_off.p, inst_exts.p,
                                                                                    inst_val.p, ex32.p, obs_exts.p, obs_data.p);
        else grp_decode_kernel<false><<<cdiv(n, 256), 256, 0, c->stream>>>(n, R.pay, gx.p, gstart.p, cnt.p, obs_off.p, inst_exts.p,
                                                                           nullptr, ex32.p, obs_exts.p, nullptr);
        c->t_end();
        LAUNCH_CHECK(c, "grp_decode");
        grp_exts_kernel<<<cdiv(ng, 256), 256, 0, c->stream>>>(ex32.p, ng, exts_or.p);
        LAUNCH_CHECK(c, "grp_exts");
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out->n = ng;
    out->key_hi = key_hi.take(); out->key_lo = key_lo.take();
    out->nobs = nobs.take(); out->exts_or = exts_or.take(); out->obs_off = obs_off.take();
    out->obs_exts = obs_exts.take(); out->obs_data = has_data ? obs_data.take() : nullptr;
    out->n_obs = n_obs;
    out->n_kmer_instances = n64;
    out->bucket_lo = p->bucket_lo; out->bucket_hi = p->bucket_hi;
    out->on_device = 1;
    return 0;
}

extern "C" void dbg_free_groups(dbg_ctx* c, dbg_kmer_groups* g) {
    if (!g) return;
    void* ptrs[] = {g->key_hi, g->key_lo, g->nobs, g->exts_or, g->obs_off, g->obs_exts, g->obs_data};
    for (void* q : ptrs) {
        if (!q) continue;
        if (g->on_device) { if (c) c->dfree(q); } else ctx_hfree(c, q);
    }
    memset(g, 0, sizeof(*g));
}

extern "C" int dbg_groups_to_host(dbg_ctx* c, const dbg_kmer_groups* d, dbg_kmer_groups* h) {
    if (!d || !h) return c->fail(10, "null argument");
    if (!d->on_device) return c->fail(10, "dbg_groups_to_host: the groups are already on the host");
    *h = *d;
    h->on_device = 0;
    h->key_hi = h->key_lo = h->obs_off = nullptr;
    h->nobs = h->obs_data = nullptr;
    h->exts_or = h->obs_exts = nullptr;
    hipError_t e = hipSuccess;
#define CP(field, T, cnt)                                                                                     \
    if (d->field && e == hipSuccess) {                                                                        \
        h->field = (T*)ctx_halloc(c, (size_t)(cnt) * sizeof(T));                                              \
        if (!h->field) e = hipErrorOutOfMemory;                                                               \
        else if ((cnt)) e = hipMemcpyAsync(h->field, d->field, (size_t)(cnt) * sizeof(T), hipMemcpyDeviceToHost, c->stream); \
    }
    CP(key_hi, uint64_t, d->n) CP(key_lo, uint64_t, d->n) CP(nobs, uint32_t, d->n) CP(exts_or, uint8_t, d->n)
    CP(obs_off, uint64_t, d->n + 1) CP(obs_exts, uint8_t, d->n_obs) CP(obs_data, uint32_t, d->n_obs)
#undef CP
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        dbg_free_groups(c, h);
        return c->fail(100, std::string("HIP error while copying the groups to the host: ") + hipGetErrorString(e));
    }
    return 0;
}
