// test_mirror_univariate_open_batch.cpp -- UnivariateKZG::open_batch of the C++ host mirror (include/zkhip.hpp): three polynomials -- the
// reference data of univariate_kzg.rs:111-129, one of a single workgroup and one of several -- opened in one call and one at a time, plain
// and with the shifted-SRS table; the reference data against the CPU oracle; one polynomial at two points, the zero polynomial and a
// constant; the empty batch; what the mirror throws.
// Built and run by tests/test_cpp_mirror_univariate_open_batch.py.  Exit code 0 = all passed.
#include <cstdio>
#include <cstring>
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

static std::vector<Fr> F(std::initializer_list<long> v) { std::vector<Fr> o; for (long x : v) o.push_back(Fr::from(x)); return o; }
static std::vector<Fr> random_fr(size_t n, uint64_t seed) {
    std::mt19937_64 g(seed);
    std::vector<Fr> v(n);
    for (auto& e : v) { for (int i = 0; i < 4; ++i) e.l[i] = g(); e.l[3] &= 0x3FFFFFFFFFFFFFFFULL; }
    return v;
}
template <class Fn> static bool panics(Fn f) { try { f(); } catch (const std::exception&) { return true; } return false; }
static bool same(const G1Affine& a, const G1Affine& b) { return a.infinity == b.infinity && (a.infinity || std::memcmp(a.xy, b.xy, 96) == 0); }
static bool same(const UnivariateKZGProof& a, const UnivariateKZGProof& b) {
    return std::memcmp(a.evaluation.l, b.evaluation.l, 32) == 0 && same(a.proof, b.proof);
}

int main() {
    const Fr tau = Fr::from(10);
    TrustedSetup srs = UnivariateKZG::generate_srs(tau, 5000);
    const auto ref = F({1, 2, 3, 4, 5});
    std::vector<DenseUnivariatePolynomial> polys;
    polys.emplace_back(ref);
    polys.emplace_back(random_fr(300, 61));
    polys.emplace_back(random_fr(4999, 62));
    std::vector<Fr> zs = {Fr::from(2), random_fr(1, 63)[0], random_fr(1, 64)[0]};
    for (int with_table = 0; with_table < 2; ++with_table) {
        if (with_table) srs.precompute();
        const auto got = UnivariateKZG::open_batch(polys, zs, srs);
        EXPECT(got.size() == 3);
        for (size_t b = 0; b < got.size(); ++b) EXPECT(same(got[b], UnivariateKZG::open(polys[b], zs[b], srs)));
        // univariate_kzg.rs:111-129 against the oracle
        std::vector<g1_jac_t> osrs(5);
        ora_kzg_univariate_srs_g1(osrs.data(), (const fr_t*)&tau, 4);
        Fr want_ev;
        g1_jac_t want;
        EXPECT(ora_univariate_kzg_open((fr_t*)&want_ev, &want, (const fr_t*)ref.data(), 5, (const fr_t*)&zs[0], osrs.data(), 5) == 0);
        g1_affine_t a;
        ora_g1_to_affine(&a, &want);
        EXPECT(std::memcmp(got[0].evaluation.l, want_ev.l, 32) == 0 && !got[0].proof.infinity && !a.inf && std::memcmp(got[0].proof.xy, &a, 96) == 0);
        // one polynomial at two points, the zero polynomial and a constant between them
        const std::vector<DenseUnivariatePolynomial> mixed = {polys[2], DenseUnivariatePolynomial(std::vector<Fr>{}), DenseUnivariatePolynomial(F({7})), polys[2]};
        const std::vector<Fr> mz = {zs[1], zs[1], zs[2], zs[2]};
        const auto m = UnivariateKZG::open_batch(mixed, mz, srs);
        EXPECT(m.size() == 4);
        for (size_t b = 0; b < m.size(); ++b) EXPECT(same(m[b], UnivariateKZG::open(mixed[b], mz[b], srs)));
        EXPECT(m[1].proof.infinity && m[2].proof.infinity && std::memcmp(m[2].evaluation.l, Fr::from(7).l, 32) == 0);
        EXPECT(!same(m[0].proof, m[3].proof));
    }
    EXPECT(UnivariateKZG::open_batch({}, {}, srs).empty());
    EXPECT(panics([&] { UnivariateKZG::open_batch(polys, {zs[0]}, srs); }));                               // one point per polynomial
    polys.emplace_back(random_fr(5003, 65));
    zs.push_back(zs[0]);
    EXPECT(panics([&] { UnivariateKZG::open_batch(polys, zs, srs); }));                                    // index out of bounds :75
    std::printf("univariate open batch mirror: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
