"""Pure-Python restatement of filter_kmers (src/filter.rs:139-231) with an arbitrary KmerSummarizer (src/filter.rs:27-35).

Starts from refgen.naive_filter (lib.rs:812-841 + filter.rs:190-196), but keeps every observation (Exts, d) of a k-mer in input
order -- what the reference's stable sort_by_key leaves inside a group (filter.rs:205-211) -- and visits the groups in ascending
canonical-key order (bucket = the first four bases, then the key: the same order).  Python re-implementations of the two
summarizers the device runs itself (CountFilter, CountFilterSet) and a few that depend on order and multiplicity live here too,
each in both host protocols of the package's filter_kmers (summarize, summarize_groups).
"""
import numpy as np

from refgen import exts_rc_py, kmer_rc_int, kmers_of


def model_groups(seqs, seq_exts, data, k, stranded):
    """[(kmer, [(exts, d), ...])] ascending by kmer; data: per-sequence D1 (None = unit, d is None)"""
    groups = {}
    for si, (s, e) in enumerate(zip(seqs, seq_exts)):
        s = [int(x) for x in s]
        n = len(s)
        if n < k:
            continue
        d = None if data is None else data[si]
        for j, v in enumerate(kmers_of(s, k)):
            left = (e & 0x0F) if j == 0 else (1 << s[j - 1])
            right = (e & 0xF0) if j + k == n else (1 << (4 + s[j + k]))
            ex = left | right
            if not stranded:
                r = kmer_rc_int(k, v)
                if not (v < r):
                    v, ex = r, exts_rc_py(ex)
            groups.setdefault(v, []).append((ex, d))
    return sorted(groups.items())


def model_filter(groups, summarizer, report_all_kmers=True):
    """(valid keys, their Exts, their DS, all keys) -- the loop of filter.rs:204-221 over model_groups"""
    keys, exts, ds, all_keys = [], [], [], []
    for kmer, obs in groups:
        v, e, d = summarizer.summarize((kmer, ex, dd) for ex, dd in obs)
        if report_all_kmers:
            all_keys.append(kmer)
        if v:
            keys.append(kmer)
            exts.append(int(e))
            ds.append(d)
    return keys, exts, ds, all_keys


# ---- summarizers in the trait's protocol: summarize(items) -> (valid, Exts, DS) -------------------------------------
class PyCountFilter:
    """CountFilter (filter.rs:40-63): u16 saturating count, valid iff count >= min"""

    def __init__(self, min_kmer_obs):
        self.min_kmer_obs = min_kmer_obs

    def summarize(self, items):
        count, ex = 0, 0
        for _, e, _ in items:
            count = min(count + 1, 65535)
            ex |= int(e)
        return count >= self.min_kmer_obs, ex, count


class PyCountFilterSet:
    """CountFilterSet (filter.rs:68-101): sorted de-duplicated D1 list, valid iff nobs >= min"""

    def __init__(self, min_kmer_obs):
        self.min_kmer_obs = min_kmer_obs

    def summarize(self, items):
        n, ex, ds = 0, 0, set()
        for _, e, d in items:
            n += 1
            ex |= int(e)
            ds.add(d)
        return n >= self.min_kmer_obs, ex, sorted(ds)


class FirstLabel:
    """the label of the first observation (depends on input order)"""

    def summarize(self, items):
        first, ex = None, 0
        for _, e, d in items:
            if first is None:
                first = d
            ex |= int(e)
        return True, ex, first


class LabelCounts:
    """read counts split by label ("haplotype"): sorted [(label, observations)]"""

    def __init__(self, min_kmer_obs=1):
        self.min_kmer_obs = min_kmer_obs

    def summarize(self, items):
        c, ex, n = {}, 0, 0
        for _, e, d in items:
            c[d] = c.get(d, 0) + 1
            ex |= int(e)
            n += 1
        return n >= self.min_kmer_obs, ex, sorted(c.items())


class DistinctLabels:
    """distinct-label count ("UMI count"), valid iff at least min distinct labels"""

    def __init__(self, min_distinct=1):
        self.min_distinct = min_distinct

    def summarize(self, items):
        s, ex = set(), 0
        for _, e, d in items:
            s.add(d)
            ex |= int(e)
        return len(s) >= self.min_distinct, ex, len(s)


# ---- the same in the vectorised protocol: summarize_groups(KmerGroups) -> (valid, exts, data) ----------------------------
class VecCountFilter:
    """CountFilter over one pass's KmerGroups arrays; min_obs_export lets the export skip the observations it never reads"""

    def __init__(self, min_kmer_obs, export_all=False):
        self.min_kmer_obs = min_kmer_obs
        self.min_obs_export = 0 if export_all else min_kmer_obs

    def summarize_groups(self, g):
        count = np.minimum(g.nobs, 65535).astype(np.uint16)
        return count >= self.min_kmer_obs, g.exts_or, count


class VecCountFilterSet:
    def __init__(self, min_kmer_obs):
        self.min_kmer_obs = min_kmer_obs
        self.min_obs_export = min_kmer_obs

    def summarize_groups(self, g):
        valid = g.nobs >= self.min_kmer_obs
        data = []
        for i in range(len(g)):
            a, b = int(g.obs_off[i]), int(g.obs_off[i + 1])
            data.append(sorted(set(int(x) for x in g.obs_data[a:b])) if g.obs_data is not None else [None] if b > a else [])
        return valid, g.exts_or, data
