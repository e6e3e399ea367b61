// test_mirror_mle_batch.cpp -- Multilinear::evaluation_batch of the C++ host mirror (include/zkhip.hpp): three tables of 2^3 and of
// 2^13 entries, each at its own point, batched and singly, both against the CPU oracle; one table at three points; the empty batch;
// what the mirror throws.  Built and run by tests/test_cpp_mirror_mle_batch.py.  Exit code 0 = all passed.
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

int main() {
    constexpr size_t B = 3;
    for (size_t nv : {(size_t)3, (size_t)13}) {
        const size_t n = (size_t)1 << nv;
        std::vector<std::vector<Fr>> evals(B), points(B);
        std::vector<Multilinear> tables;
        std::vector<Fr> want(B);
        for (size_t b = 0; b < B; ++b) {
            evals[b] = random_fr(n, 15000 + 16 * nv + b);
            points[b] = random_fr(nv, 16000 + 16 * nv + b);
            tables.emplace_back(evals[b]);
            EXPECT(ora_mle_evaluation((fr_t*)&want[b], O(evals[b]), n, O(points[b]), nv) == 0);
        }
        const auto batch = Multilinear::evaluation_batch(tables, points);
        EXPECT(batch.size() == B);
        for (size_t b = 0; b < B && b < batch.size(); ++b) {
            EXPECT(batch[b] == want[b]);
            EXPECT(tables[b].evaluation(points[b]) == want[b]);
        }
        // one table at every point: the pointer repeats
        const auto one_table = Multilinear::evaluation_batch({tables[1], tables[1], tables[1]}, points);
        for (size_t b = 0; b < B && b < one_table.size(); ++b) {
            Fr w;
            EXPECT(ora_mle_evaluation((fr_t*)&w, O(evals[1]), n, O(points[b]), nv) == 0);
            EXPECT(one_table[b] == w);
        }
        bool threw = false;
        try { Multilinear::evaluation_batch(tables, {points[0], points[1]}); } catch (const std::exception&) { threw = true; }
        EXPECT(threw);                                                                 // one point per table
        threw = false;
        try { Multilinear::evaluation_batch(tables, {points[0], points[1], std::vector<Fr>(nv + 1)}); } catch (const std::exception&) { threw = true; }
        EXPECT(threw);                                                                 // as many coordinates as variables
    }
    EXPECT(Multilinear::evaluation_batch({}, {}).empty());
    bool threw = false;
    try { Multilinear::evaluation_batch({Multilinear(random_fr(8, 1)), Multilinear(random_fr(4, 2))}, {random_fr(3, 3), random_fr(3, 4)}); }
    catch (const std::exception&) { threw = true; }
    EXPECT(threw);                                                                     // one length
    std::printf("mle batch mirror: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
