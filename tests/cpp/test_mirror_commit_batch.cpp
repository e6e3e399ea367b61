// test_mirror_commit_batch.cpp -- MultilinearKZG::commitment_batch / UnivariateKZG::commitment_batch of the C++ host mirror
// (include/zkhip.hpp): the reference data of multilinear_kzg.rs:133-148 in a batch with two random polynomials, plain and with the
// shifted-SRS table; three polynomials of 2^13 scalars (the bucket route), batched and singly, against commit == p(tau) * G from the
// CPU oracle; polynomials of several lengths, the zero polynomial among them; the empty batch; what the mirror throws.
// Built and run by tests/test_cpp_mirror_commit_batch.py.  Exit code 0 = all passed.
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
static const fr_t* O(const std::vector<Fr>& v) { return reinterpret_cast<const fr_t*>(v.data()); }
template <class Fn> static bool panics(Fn f) { try { f(); } catch (const std::exception&) { return true; } return false; }
static bool same_point(const G1Affine& g, const g1_jac_t& want) {
    g1_affine_t a;
    ora_g1_to_affine(&a, &want);
    return (g.infinity == (a.inf != 0)) && (g.infinity || std::memcmp(g.xy, &a, 96) == 0);
}
static bool same(const G1Affine& a, const G1Affine& b) { return a.infinity == b.infinity && (a.infinity || std::memcmp(a.xy, b.xy, 96) == 0); }
// p(tau) * G, p(tau) from the oracle's multilinear evaluation
static g1_jac_t p_tau_g(const std::vector<Fr>& sc, const std::vector<Fr>& tau) {
    Fr p_tau;
    ora_mle_evaluation((fr_t*)&p_tau, O(sc), sc.size(), O(tau), tau.size());
    uint64_t canon[4];
    ora_fr_to_canonical(canon, (const fr_t*)&p_tau);
    g1_jac_t g, want;
    ora_g1_generator(&g);
    ora_g1_mul_bigint(&want, &g, canon, 4);
    return want;
}

int main() {
    {   // multilinear_kzg.rs:133-148 data, with two random polynomials; plain and table
        const auto tau = F({2, 3, 4});
        const std::vector<std::vector<Fr>> vals = {F({0, 7, 0, 5, 0, 7, 4, 9}), random_fr(8, 21), random_fr(8, 22)};
        std::vector<Multilinear> polys;
        for (const auto& v : vals) polys.emplace_back(v);
        TrustedSetup srs = TrustedSetup::setup(tau);
        for (int with_table = 0; with_table < 2; ++with_table) {
            if (with_table) srs.precompute();
            const auto got = MultilinearKZG::commitment_batch(polys, srs);
            EXPECT(got.size() == 3);
            for (size_t b = 0; b < got.size(); ++b) {
                EXPECT(same_point(got[b], p_tau_g(vals[b], tau)));
                EXPECT(same(got[b], MultilinearKZG::commitment(polys[b], srs)));
            }
        }
        EXPECT(panics([&] { MultilinearKZG::commitment_batch({polys[0], Multilinear(F({1, 2, 3, 4})), polys[1]}, srs); }));     // assert_eq! :36-41
        EXPECT(MultilinearKZG::commitment_batch({}, srs).empty());
    }
    {   // 2^13 x 3: one pass of the bucket pipeline; the pointer of polynomial 0 a second time
        const size_t nv = 13, n = (size_t)1 << nv;
        const auto tau = random_fr(nv, 31);
        std::vector<std::vector<Fr>> vals;
        std::vector<Multilinear> polys;
        for (size_t b = 0; b < 3; ++b) { vals.push_back(random_fr(n, 40 + b)); polys.emplace_back(vals.back()); }
        TrustedSetup srs = TrustedSetup::setup(tau);
        for (int with_table = 0; with_table < 2; ++with_table) {
            if (with_table) srs.precompute();
            const auto got = MultilinearKZG::commitment_batch({polys[0], polys[1], polys[2], polys[0]}, srs);
            EXPECT(got.size() == 4);
            for (size_t b = 0; b < got.size(); ++b) {
                EXPECT(same_point(got[b], p_tau_g(vals[b % 3], tau)));
                EXPECT(same(got[b], MultilinearKZG::commitment(polys[b % 3], srs)));
            }
        }
    }
    {   // univariate: several lengths in one call, the zero polynomial among them; univariate_kzg.rs:111-129 data first
        const Fr tau = Fr::from(10);
        TrustedSetup srs = UnivariateKZG::generate_srs(tau, 5000);
        const auto coeffs = random_fr(5001, 51);
        std::vector<DenseUnivariatePolynomial> polys;
        polys.emplace_back(F({1, 2, 3, 4, 5}));
        for (size_t len : {(size_t)0, (size_t)1, (size_t)300, (size_t)4097, (size_t)5001}) polys.emplace_back(std::vector<Fr>(coeffs.begin(), coeffs.begin() + len));
        const auto got = UnivariateKZG::commitment_batch(polys, srs);
        EXPECT(got.size() == polys.size());
        for (size_t b = 0; b < got.size(); ++b) EXPECT(same(got[b], UnivariateKZG::commitment(polys[b], srs)));
        EXPECT(got[1].infinity);
        std::vector<g1_jac_t> osrs(5);
        ora_kzg_univariate_srs_g1(osrs.data(), (const fr_t*)&tau, 4);
        g1_jac_t want;
        const auto ref = F({1, 2, 3, 4, 5});
        ora_kzg_commitment(&want, O(ref), 5, osrs.data(), 5, 0);
        EXPECT(same_point(got[0], want));
        polys.emplace_back(random_fr(5002, 52));
        EXPECT(panics([&] { UnivariateKZG::commitment_batch(polys, srs); }));                          // index out of bounds :53
        EXPECT(UnivariateKZG::commitment_batch({}, srs).empty());
    }
    std::printf("commit batch mirror: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
