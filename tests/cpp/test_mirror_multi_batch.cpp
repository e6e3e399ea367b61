// test_mirror_multi_batch.cpp -- MultiComposedSumcheckProver::prove_batch / prove_partial_batch of the C++ host mirror
// (include/zkhip.hpp): three [2, 2] claims of 2^3 entries, batched and singly, both against the CPU oracle.
// Built and run by tests/test_cpp_mirror_multi_batch.py.  Exit code 0 = all passed.
#include <cstdio>
#include <random>

#include "../../include/zkhip.hpp"
extern "C" {
#include "../../oracle/zkoracle.h"
}

using namespace zkc;
static int g_failed = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("  FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static std::vector<Fr> random_fr(size_t n, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::vector<Fr> v(n);
    for (auto& e : v) { for (int i = 0; i < 4; ++i) e.l[i] = g(); e.l[3] &= 0x3FFFFFFFFFFFFFFFULL; }
    return v;
}
static const fr_t* O(const std::vector<Fr>& v) { return reinterpret_cast<const fr_t*>(v.data()); }
static fr_t* O(std::vector<Fr>& v) { return reinterpret_cast<fr_t*>(v.data()); }

int main() {
    constexpr size_t B = 3, N = 8, NV = 3;
    size_t sizes[2] = {2, 2};
    std::vector<std::vector<Fr>> flats(B);
    std::vector<std::vector<ComposedMultilinear>> claims;
    std::vector<Fr> sums(B);
    for (size_t b = 0; b < B; ++b) {
        std::vector<Multilinear> t;
        for (size_t q = 0; q < 4; ++q) {
            auto e = random_fr(N, 14000 + 8 * b + q);
            flats[b].insert(flats[b].end(), e.begin(), e.end());
            t.emplace_back(e);
        }
        claims.push_back({ComposedMultilinear({t[0], t[1]}), ComposedMultilinear({t[2], t[3]})});
        ora_multi_composed_sum((fr_t*)&sums[b], O(flats[b]), sizes, 2, N);
        EXPECT(MultiComposedSumcheckProver::calculate_poly_sum(claims[b]) == sums[b]);
    }
    for (int partial = 0; partial <= 1; ++partial) {
        auto batch = partial ? MultiComposedSumcheckProver::prove_partial_batch(claims, sums) : MultiComposedSumcheckProver::prove_batch(claims, sums);
        EXPECT(batch.size() == B);
        for (size_t b = 0; b < B && b < batch.size(); ++b) {
            auto single = partial ? MultiComposedSumcheckProver::prove_partial(claims[b], sums[b]) : MultiComposedSumcheckProver::prove(claims[b], sums[b]);
            std::vector<ora_sparse_t> orp(NV);
            std::vector<Fr> och(NV);
            ora_multi_composed_prove(O(flats[b]), sizes, 2, N, (const fr_t*)&sums[b], partial, orp.data(), O(och));
            std::vector<uint8_t> obytes;
            for (auto& r : orp) { uint8_t buf[64 * ORA_SPARSE_MAX]; size_t n = ora_sparse_to_bytes(buf, &r); obytes.insert(obytes.end(), buf, buf + n); }
            EXPECT(batch[b].first.to_bytes() == obytes && batch[b].second == och && batch[b].first.sum == sums[b]);
            EXPECT(single.first.to_bytes() == obytes && single.second == och);
            EXPECT(batch[b].first.round_polys.size() == NV);
            // (the oracle's verifier replays prove()'s transcript, table bytes first: it accepts the full proofs only)
            if (!partial) EXPECT(ora_multi_composed_verify(O(flats[b]), sizes, 2, N, (const fr_t*)&sums[b], orp.data(), NV) == 1);
        }
    }
    EXPECT(MultiComposedSumcheckProver::prove_batch({}, {}).empty());
    bool threw = false;
    try { MultiComposedSumcheckProver::prove_partial_batch(claims, std::vector<Fr>(2)); } catch (const std::exception&) { threw = true; }
    EXPECT(threw);                                                                     // one claimed sum per claim
    std::printf("multi batch mirror: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
