"""CPU: the pure-Python filter_kmers with an arbitrary summarizer (tests/summarizer_model.py), run with Python CountFilter /
CountFilterSet, equals the oracle library's filter_kmers exactly -- so that the GPU tests of the grouped-observation export can
take the model as their expectation for summarizers the oracle does not have."""
import numpy as np
import pytest

import oracle_lib as O
import refgen
from summarizer_model import PyCountFilter, PyCountFilterSet, model_filter, model_groups


def _inputs(seed):
    rng = np.random.default_rng(seed)
    seqs = refgen.simple_random_contigs(rng) + refgen.random_contigs(rng)[:6]
    seqs += [refgen.from_ascii(refgen.DEGEN), np.zeros(70, np.uint8), refgen.random_dna(rng, 3)]
    seqs = seqs + seqs[:4]                                       # repeated reads: multiplicity
    exts = [int(x) for x in rng.integers(0, 256, len(seqs))]
    data = [int(x) for x in rng.integers(0, 5, len(seqs))]
    return seqs, exts, data


@pytest.mark.parametrize("stranded", [False, True])
@pytest.mark.parametrize("k", [4, 15, 31, 47, 64])
def test_model_matches_oracle(k, stranded):
    seqs, exts, data = _inputs(1000 + k)
    ss = O.SeqSet.from_byte_seqs(seqs, exts, data, 1)
    groups = model_groups(seqs, exts, data, k, stranded)
    for min_obs in (1, 2, 3):
        want = O.filter_kmers(ss, k, O.COUNT_FILTER, min_obs, stranded=stranded, report_all=True)
        keys, ex, ds, all_keys = model_filter(groups, PyCountFilter(min_obs))
        assert keys == want.keys() and ex == [int(x) for x in want.exts] and ds == [int(x) for x in want.count]
        assert all_keys == [(int(h) << 64) | int(l) for h, l in zip(want.all_hi, want.all_lo)]
        want = O.filter_kmers(ss, k, O.COUNT_FILTER_SET, min_obs, stranded=stranded, report_all=True)
        keys, ex, ds, _ = model_filter(groups, PyCountFilterSet(min_obs))
        assert keys == want.keys() and ex == [int(x) for x in want.exts]
        assert ds == [[int(x) for x in want.set_val[int(want.set_off[i]):int(want.set_off[i + 1])]] for i in range(len(want))]


def test_model_keeps_input_order_and_multiplicity():
    """a k-mer seen in reads labelled 3, 1, 3 keeps exactly that sequence of observations"""
    k = 5
    s = refgen.from_ascii("ACGTTGCA")
    groups = dict(model_groups([s, s, s], [0, 0, 0], [3, 1, 3], k, True))
    assert [d for _, d in groups[refgen.kmer_int(s[:k])]] == [3, 1, 3]
