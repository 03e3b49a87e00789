// filter_kmers<K, S> with a summarizer of the caller's own (include/debruijn_mi355x.hpp over dbg_mi355x_groups.h): a user
// re-implementation of CountFilter gives the CountFilter overload's index and all_kmers, and an order-dependent summarizer sees
// each k-mer's observations in input order.
#include <cstdio>
#include <random>
#include <set>
#include "debruijn_mi355x.hpp"

using namespace debruijn;

struct MyCount {                 // CountFilter (filter.rs:40-63), written as a caller would
    size_t min_obs;
    template <class Obs> std::tuple<bool, Exts, uint16_t> summarize(const Obs& obs) const {
        uint32_t n = 0; uint8_t ex = 0;
        for (auto& o : obs) { n = n < 65535 ? n + 1 : n; ex |= std::get<1>(o).val; }
        return {n >= min_obs, Exts(ex), (uint16_t)n};
    }
};
struct FirstAndDistinct {        // (label of the first observation, number of distinct labels)
    template <class Obs> std::tuple<bool, Exts, std::pair<uint8_t, uint32_t>> summarize(const Obs& obs) const {
        std::set<uint8_t> s; uint8_t ex = 0;
        for (auto& o : obs) { s.insert(std::get<2>(o)); ex |= std::get<1>(o).val; }
        return {true, Exts(ex), {std::get<2>(obs.front()), (uint32_t)s.size()}};
    }
};

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    Context ctx(0);
    std::mt19937_64 rng(7);
    std::string genome;
    for (int i = 0; i < 3000; i++) genome.push_back("ACGT"[rng() & 3]);
    std::vector<std::tuple<DnaString, Exts, uint8_t>> seqs;
    for (int r = 0; r < 400; r++) {
        const size_t st = rng() % (genome.size() - 150);
        std::string read = genome.substr(st, 150);
        if (rng() % 10 == 0) read[rng() % 150] = 'A';
        seqs.emplace_back(DnaString::from_dna_string(read), Exts((uint8_t)(rng() & 0xff)), (uint8_t)(r % 7));
    }
    seqs.emplace_back(DnaString::from_dna_string(std::string(200, 'A')), Exts(0x21), (uint8_t)250);
    using K = Kmer<31>;
    for (size_t min_obs : {1, 2, 5}) {
        auto native = filter_kmers<K>(ctx, seqs, CountFilter(min_obs), false, true, 4);
        auto mine = filter_kmers<K>(ctx, seqs, MyCount{min_obs}, false, true, 4);
        CHECK(native.first.len() == mine.first.len() && native.first.len() > 0);
        for (size_t i = 0; i < native.first.len(); i++) {
            CHECK(native.first.keys[i] == mine.first.keys[i]);
            CHECK(native.first.exts[i] == mine.first.exts[i]);
            CHECK(native.first.data[i] == mine.first.data[i]);
        }
        CHECK(native.second.size() == mine.second.size());
        for (size_t i = 0; i < native.second.size(); i++) CHECK(native.second[i] == mine.second[i]);
    }
    // the poly-A k-mer: observations come from the last read only; a k-mer of read 0 that no other read has: label 0
    auto fd = filter_kmers<K>(ctx, seqs, FirstAndDistinct{}, false, false, 4);
    const K polya = K::from_hi_lo(0, 0);
    bool seen = false;
    for (size_t i = 0; i < fd.first.len(); i++)
        if (fd.first.keys[i] == polya) { seen = true; CHECK(fd.first.data[i].first == 250 && fd.first.data[i].second == 1); }
    CHECK(seen);
    std::printf("cpp groups ok: %zu k-mers\n", fd.first.len());
    return 0;
}
