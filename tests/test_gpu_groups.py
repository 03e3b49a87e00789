"""GPU: the grouped-observation export (include/dbg_mi355x_groups.h) and filter_kmers with host-side summarizers.

Expectation: tests/summarizer_model.py, the pure-Python filter_kmers with an arbitrary summarizer, itself checked against the
oracle library on the CPU (test_summarizer_model.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import refgen
from pkg import dbg, capi
from summarizer_model import (DistinctLabels, FirstLabel, LabelCounts, PyCountFilter, PyCountFilterSet, VecCountFilter,
                              VecCountFilterSet, model_filter, model_groups)

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = dbg.Context(0)
    yield c
    c.close()


def _inputs(seed, width):
    """the reference's awkward shapes (test.rs:58-95 shared repeat + palindrome, test.rs:170-193 degenerate repeat), all-A,
    reads shorter than k, an empty read, repeated reads; random sequence Exts; labels of the given width with its extremes"""
    rng = np.random.default_rng(seed)
    seqs = refgen.simple_random_contigs(rng) + refgen.random_contigs(rng)[:5]
    seqs += [refgen.from_ascii(refgen.DEGEN), refgen.from_ascii(refgen.DEGEN), np.zeros(90, np.uint8), refgen.random_dna(rng, 3),
             np.zeros(0, np.uint8), refgen.random_dna(rng, 40)]
    seqs = seqs + seqs[:3]
    exts = [int(x) for x in rng.integers(0, 256, len(seqs))]
    if width == 0:
        return seqs, exts, None
    hi = {1: 255, 2: 65535, 4: 0xFFFFFFFF}[width]
    data = [int(x) for x in rng.integers(0, hi, len(seqs), dtype=np.uint64, endpoint=True)]
    data[0], data[1] = hi, 0
    if width == 4:
        data[2], data[3] = 1 << 24, (1 << 24) + 7
    return seqs, exts, data


def _host(seqs, exts, data, width):
    ps = dbg.PackedDnaStringSet.from_seqs(seqs)
    return dbg.HostSeqs(ps.words, ps.start, ps.length, exts, data, width if data is not None else 0)


def _model_arrays(groups):
    keys = [g[0] for g in groups]
    obs = [o for _, os_ in groups for o in os_]
    off = np.zeros(len(groups) + 1, np.uint64)
    off[1:] = np.cumsum([len(o) for _, o in groups]) if groups else []
    ex_or = []
    for _, os_ in groups:
        e = 0
        for x, _ in os_:
            e |= x
        ex_or.append(e)
    return dict(key_hi=np.array([q >> 64 for q in keys], np.uint64), key_lo=np.array([q & M64 for q in keys], np.uint64),
                nobs=np.array([len(o) for _, o in groups], np.uint32), exts_or=np.array(ex_or, np.uint8), obs_off=off,
                obs_exts=np.array([e for e, _ in obs], np.uint8),
                obs_data=None if not obs or obs[0][1] is None else np.array([d for _, d in obs], np.uint32))


def _assert_groups(g, want):
    for name in ("key_hi", "key_lo", "nobs", "exts_or", "obs_off", "obs_exts"):
        assert np.array_equal(getattr(g, name), want[name]), name
    if want["obs_data"] is None:
        assert g.obs_data is None
    else:
        assert np.array_equal(g.obs_data, want["obs_data"])


KS = [4, 15, 16, 31, 32, 33, 47, 63, 64]


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("k", KS)
def test_groups_match_model(ctx, k, stranded):
    for width in ((0, 1, 2, 4) if k in (4, 31, 33, 64) else ((1, 4) if stranded else (0, 2))):
        seqs, exts, data = _inputs(17 * k + width, width)
        g = dbg.kmer_groups(_host(seqs, exts, data, width), k, stranded, ctx=ctx)
        _assert_groups(g, _model_arrays(model_groups(seqs, exts, data, k, stranded)))
        assert g.n_kmer_instances == int(g.nobs.sum()) == sum(max(len(s) - k + 1, 0) for s in seqs)


def test_empty_and_short_inputs(ctx):
    g = dbg.kmer_groups(_host([], [], None, 0), 31, False, ctx=ctx)
    assert len(g) == 0 and list(g.obs_off) == [0] and len(g.obs_exts) == 0
    seqs = [np.zeros(10, np.uint8), np.ones(30, np.uint8)]
    g = dbg.kmer_groups(_host(seqs, [0x11, 0x22], [5, 6], 1), 31, False, ctx=ctx)
    assert len(g) == 0 and list(g.obs_off) == [0] and g.n_kmer_instances == 0


def test_long_homopolymer_groups(ctx):
    """one k-mer with more than 10^6 observations, one with more than 65 535: exact nobs, input-order Exts; the native CountFilter
    and a Python one through the export agree (u16 saturation)"""
    k = 31
    na, nc = 1_000_100, 70_000
    seqs = [np.zeros(na, np.uint8), np.ones(nc, np.uint8), refgen.from_ascii("ACGT" * 20)]
    exts = [0x28, 0x41, 0]
    hs = _host(seqs, exts, [9, 0xFFFFFFFF, 3], 4)
    g = dbg.kmer_groups(hs, k, False, ctx=ctx)
    keys = g.keys()
    ia, ic = keys.index(0), keys.index(int("01" * k, 2))
    for i, n, ex, base, lab in ((ia, na, 0x28, 0, 9), (ic, nc, 0x41, 1, 0xFFFFFFFF)):
        m = n - k + 1
        assert int(g.nobs[i]) == m
        a, b = int(g.obs_off[i]), int(g.obs_off[i + 1])
        inner = (1 << base) | (16 << base)
        want = np.full(m, inner, np.uint8)
        want[0] = (ex & 0x0F) | (16 << base)
        want[-1] = (1 << base) | (ex & 0xF0)
        assert np.array_equal(g.obs_exts[a:b], want)
        assert np.all(g.obs_data[a:b] == lab)
        assert int(g.exts_or[i]) == int(np.bitwise_or.reduce(want))
    native, all_n = dbg.filter_kmers(hs, dbg.CountFilter(2), False, True, 4, k=k, ctx=ctx)
    for summ in (VecCountFilter(2), VecCountFilter(2, export_all=True)):
        t, all_t = dbg.filter_kmers(hs, summ, False, True, 4, k=k, ctx=ctx)
        assert np.array_equal(t.key_lo, native.key_lo) and np.array_equal(t.exts, native.exts)
        assert np.array_equal(t.ds, native.count) and all_t == all_n
    assert 65535 in [int(x) for x in native.count]


def test_passes_concatenate(ctx):
    k = 31
    hs = dbg.synth_reads_host(n_reads=3000, read_len=150, error_rate=0.01, stranded=False, n_colours=7)
    total = int(np.maximum(hs.length.astype(np.int64) - k + 1, 0).sum())
    bounds = dbg.kmer_group_passes(hs, k, False, max_obs_per_pass=total // 12, ctx=ctx)
    assert bounds[0] == 0 and bounds[-1] == 256 and len(bounds) >= 9
    assert all(a < b for a, b in zip(bounds[:-1], bounds[1:]))
    assert dbg.kmer_group_passes(hs, k, False, ctx=ctx) == [0, 256]
    one = dbg.kmer_groups(hs, k, False, ctx=ctx)
    many = dbg.kmer_groups(hs, k, False, bounds=bounds, ctx=ctx)
    parts = list(dbg.iter_kmer_groups(hs, k, False, bounds=bounds, ctx=ctx))
    assert len(parts) == len(bounds) - 1 and all(p.bounds == [a, b] for p, a, b in zip(parts, bounds[:-1], bounds[1:]))
    for name in ("key_hi", "key_lo", "nobs", "exts_or", "obs_off", "obs_exts", "obs_data"):
        assert np.array_equal(getattr(one, name), getattr(many, name)), name
    assert one.n_kmer_instances == many.n_kmer_instances == total
    with pytest.raises(dbg.DbgError):                          # a bucket alone over the pass limit
        dbg.kmer_group_passes(hs, k, False, max_obs_per_pass=10, ctx=ctx)


def test_min_obs_export(ctx):
    k = 15
    seqs, exts, data = _inputs(5, 2)
    hs = _host(seqs, exts, data, 2)
    full = dbg.kmer_groups(hs, k, False, ctx=ctx)
    for m in (2, 3):
        g = dbg.kmer_groups(hs, k, False, min_obs_export=m, ctx=ctx)
        for name in ("key_hi", "key_lo", "nobs", "exts_or"):
            assert np.array_equal(getattr(g, name), getattr(full, name)), name
        seg = np.diff(g.obs_off.astype(np.int64))
        assert np.array_equal(seg, np.where(full.nobs >= m, full.nobs, 0))
        keep = np.repeat(full.nobs >= m, full.nobs)
        assert np.array_equal(g.obs_exts, full.obs_exts[keep]) and np.array_equal(g.obs_data, full.obs_data[keep])
        assert 0 < len(g.obs_exts) < len(full.obs_exts)


def test_sequence_index_flag(ctx):
    k = 33
    seqs, exts, data = _inputs(9, 1)
    g = dbg.kmer_groups(_host(seqs, exts, data, 1), k, False, obs_seq_index=True, ctx=ctx)
    want = _model_arrays(model_groups(seqs, exts, list(range(len(seqs))), k, False))
    _assert_groups(g, want)


def test_host_copy_equals_device(ctx):
    """dbg_groups_to_host returns the bytes dbg_kmer_groups_dev left in HBM"""
    hip = _loaded_hip_runtime()
    k = 47
    seqs, exts, data = _inputs(3, 4)
    hs = _host(seqs, exts, data, 4)
    host = hs.c_struct()
    dev = capi.SeqSet()
    ctx.check(ctx.lib.dbg_seqset_to_device(ctx.h, C.byref(host), C.byref(dev)))
    gd, gh = capi.KmerGroups(), capi.KmerGroups()
    try:
        gp = capi.GroupParams(k, 0, 0, 256, 0, 0)
        ctx.check(ctx.lib.dbg_kmer_groups_dev(ctx.h, C.byref(dev), C.byref(gp), C.byref(gd)))
        assert gd.on_device == 1 and gd.n > 0
        ctx.check(ctx.lib.dbg_groups_to_host(ctx.h, C.byref(gd), C.byref(gh)))
        assert gh.on_device == 0 and (gh.n, gh.n_obs, gh.n_kmer_instances) == (gd.n, gd.n_obs, gd.n_kmer_instances)
        assert hip.hipDeviceSynchronize() == 0
        for name, cnt, dt in (("key_hi", gd.n, np.uint64), ("key_lo", gd.n, np.uint64), ("nobs", gd.n, np.uint32),
                              ("exts_or", gd.n, np.uint8), ("obs_off", gd.n + 1, np.uint64), ("obs_exts", gd.n_obs, np.uint8),
                              ("obs_data", gd.n_obs, np.uint32)):
            buf = np.zeros(cnt, dt)
            assert hip.hipMemcpy(buf.ctypes.data, getattr(gd, name), buf.nbytes, 2) == 0, name
            hv = np.ctypeslib.as_array(C.cast(getattr(gh, name), C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(cnt,))
            assert np.array_equal(buf, hv), name
    finally:
        ctx.lib.dbg_free_groups(ctx.h, C.byref(gh))
        ctx.lib.dbg_free_groups(ctx.h, C.byref(gd))
        ctx.lib.dbg_seqset_free_device(ctx.h, C.byref(dev))


def _loaded_hip_runtime():
    """the HIP runtime this process already drives (torch's copy, which the library binds by its soname), whatever its version"""
    import glob
    import os
    import torch  # noqa: F401
    capi.load()
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64.so" in ln}
    paths = sorted(p for p in paths if os.path.basename(p).startswith("libamdhip64.so")) or sorted(glob.glob("/opt/rocm/lib/libamdhip64.so*"))
    assert paths, "no HIP runtime loaded"
    hip = C.CDLL(paths[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipDeviceSynchronize.argtypes = []
    return hip


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("k", [15, 31, 47])
def test_python_count_filters_match_native(ctx, k, stranded):
    seqs, exts, data = _inputs(100 + k, 1)
    hs = _host(seqs, exts, data, 1)
    for min_obs in (1, 2):
        native, all_n = dbg.filter_kmers(hs, dbg.CountFilter(min_obs), stranded, True, 4, k=k, ctx=ctx)
        for summ in (PyCountFilter(min_obs), VecCountFilter(min_obs)):
            t, all_t = dbg.filter_kmers(hs, summ, stranded, True, 4, k=k, ctx=ctx)
            assert isinstance(t, dbg.SummaryTable) and all_t == all_n
            assert np.array_equal(t.key_hi, native.key_hi) and np.array_equal(t.key_lo, native.key_lo)
            assert np.array_equal(t.exts, native.exts) and np.array_equal(t.ds, native.count)
            assert [t.data(i) for i in range(len(t))] == [native.data(i) for i in range(len(native))]
        native, all_n = dbg.filter_kmers(hs, dbg.CountFilterSet(min_obs), stranded, True, 4, k=k, ctx=ctx)
        for summ in (PyCountFilterSet(min_obs), VecCountFilterSet(min_obs)):
            t, all_t = dbg.filter_kmers(hs, summ, stranded, True, 4, k=k, ctx=ctx)
            assert all_t == all_n and np.array_equal(t.key_lo, native.key_lo) and np.array_equal(t.exts, native.exts)
            assert [t.data(i) for i in range(len(t))] == [native.data(i) for i in range(len(native))]
            assert [list(x) for x in t] == [list(x) for x in native]


@pytest.mark.parametrize("stranded", [False, True])
def test_order_and_multiplicity_summarizers(ctx, stranded):
    k = 31
    seqs, exts, data = _inputs(77, 4)
    hs = _host(seqs, exts, data, 4)
    groups = model_groups(seqs, exts, data, k, stranded)
    for summ in (FirstLabel(), LabelCounts(2), DistinctLabels(2)):
        keys, ex, ds, all_keys = model_filter(groups, summ, report_all_kmers=False)
        t, all_t = dbg.filter_kmers(hs, summ, stranded, False, 4, k=k, ctx=ctx)
        assert t.keys() == keys and [int(x) for x in t.exts] == ex and all_t == []
        assert [t.data(i) for i in range(len(t))] == ds
    # D1 that is no integer: the observations carry sequence indices, the values are looked up on the host
    labels = ["hap%d" % (i % 3) for i in range(len(seqs))]
    keys, ex, ds, all_keys = model_filter(model_groups(seqs, exts, labels, k, stranded), LabelCounts(1))
    t, all_t = dbg.filter_kmers(list(zip(seqs, exts, labels)), LabelCounts(1), stranded, True, 4, k=k, ctx=ctx)
    assert t.keys() == keys and [t.data(i) for i in range(len(t))] == ds and all_t == all_keys


def test_integer_summary_into_compress(ctx):
    """an integer DS table goes straight into compress_kmers_with_hash(data=...) and matches the oracle's compress of it"""
    k = 31
    hs = dbg.synth_reads_host(n_reads=1500, read_len=150, error_rate=0.002, stranded=False, n_colours=5)
    t, _ = dbg.filter_kmers(hs, DistinctLabels(1), False, False, 4, k=k, ctx=ctx)
    assert t.ds.dtype == np.uint32 and len(t) > 0
    g = dbg.compress_kmers_with_hash(False, dbg.SimpleCompress("max"), t, k=k, data=t.ds, ctx=ctx)
    og = O.compress_kmers(k, False, O.SPEC_MAX, t.key_hi, t.key_lo, t.exts, t.ds).arrays()
    ga = g.arrays()
    for name in ("start", "length", "exts", "data"):
        assert np.array_equal(ga[name], og[name]), name
    assert np.array_equal(ga["words"], og["words"][:len(ga["words"])])


def test_invalid_arguments(ctx):
    hs = _host([np.zeros(40, np.uint8)], [0], None, 0)
    with pytest.raises(dbg.DbgError):
        dbg.kmer_groups(hs, 3, False, ctx=ctx)
    with pytest.raises(dbg.DbgError):
        dbg.kmer_groups(hs, 31, False, bounds=[0, 300], ctx=ctx)
    with pytest.raises(dbg.DbgError):
        dbg.filter_kmers(hs, FirstLabel(), False, False, 0, k=31, ctx=ctx)
