"""filter_kmers with a host-side summarizer over D1 values that are not u8/u16/u32 integers: they are never converted (floats are
not truncated, numeric strings are not parsed); the observations carry their sequence's index and the value is looked up on the
host, for summarize and for summarize_groups (groups.seq_data) alike.  The CPU test checks which values may cross as themselves."""
import numpy as np
import pytest

import refgen
from pkg import dbg
from summarizer_model import FirstLabel, LabelCounts, model_filter, model_groups


class GroupsFirstLabel:
    """FirstLabel in the vectorised protocol: the D1 of each group's first observation, looked up through seq_data when the
    observations carry sequence indices"""

    def summarize_groups(self, g):
        data = []
        for i in range(len(g)):
            data.append(next((d for _, d in g.observations(i) if d is not None), None))     # as FirstLabel: the first label seen
        return np.ones(len(g), bool), g.exts_or, data


def test_only_u32_integers_cross_as_themselves():
    is_u32 = dbg._is_u32_label
    assert is_u32(0) and is_u32(0xFFFFFFFF) and is_u32(np.uint8(7)) and is_u32(np.int64(1 << 31))
    for d in (1.7, 2.0, "7", "300", True, -1, 1 << 32, (1,), None, np.float32(3)):
        assert not is_u32(d), d


def _reads(seed):
    rng = np.random.default_rng(seed)
    seqs = refgen.simple_random_contigs(rng) + refgen.random_contigs(rng)[:4] + [refgen.from_ascii(refgen.DEGEN)] * 2
    seqs = seqs + seqs[:3]
    exts = [int(x) for x in rng.integers(0, 256, len(seqs))]
    return seqs, exts


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["float", "numeric_str", "mixed"])
@pytest.mark.parametrize("stranded", [False, True])
def test_non_integer_labels_reach_the_summarizer_unchanged(kind, stranded):
    ctx = dbg.Context(0)
    try:
        k = 31
        seqs, exts = _reads(11 + len(kind))
        n = len(seqs)
        labels = {"float": [1.7 + 0.5 * (i % 4) for i in range(n)],
                  "numeric_str": [("7", "300", "0012", "4294967296")[i % 4] for i in range(n)],
                  "mixed": [(3, None, "3", 3.0)[i % 4] for i in range(n)]}[kind]
        groups = model_groups(seqs, exts, labels, k, stranded)
        for summ in ((FirstLabel(), LabelCounts(2)) if kind != "mixed" else (FirstLabel(),)):   # (mixed labels do not sort)
            keys, ex, ds, all_keys = model_filter(groups, summ)
            t, all_t = dbg.filter_kmers(list(zip(seqs, exts, labels)), summ, stranded, True, 4, k=k, ctx=ctx)
            assert t.keys() == keys and [int(x) for x in t.exts] == ex and all_t == all_keys
            got = [t.data(i) for i in range(len(t))]
            assert got == ds
            assert [type(x) for x in got] == [type(x) for x in ds]       # 3 stays int, "3" str, 3.0 float
        keys, ex, ds, _ = model_filter(groups, FirstLabel())
        t, _ = dbg.filter_kmers(list(zip(seqs, exts, labels)), GroupsFirstLabel(), stranded, False, 4, k=k, ctx=ctx)
        got = [t.data(i) for i in range(len(t))]
        assert t.keys() == keys and got == ds and [type(x) for x in got] == [type(x) for x in ds]
    finally:
        ctx.close()
