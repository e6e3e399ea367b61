// test_verify.cpp -- the reference's KZG unit tests with their `verify` calls (kzg/src/multilinear_kzg.rs:132-197,
// kzg/src/univariate_kzg.rs:111-150), same inputs and expected booleans, through the C++ host mirror (include/zkhip.hpp).
// Built and run by tests/test_cpp_verify.py.  Exit code 0 = all passed.
#include <cstdio>

#include "../../include/zkhip.hpp"

using namespace zkc;
static int g_failed = 0, g_run = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("  FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static std::vector<Fr> F(std::initializer_list<long> v) { std::vector<Fr> o; for (long x : v) o.push_back(Fr::from(x)); return o; }

static void test_kzg_1() {                 // multilinear_kzg.rs:132-155
    auto prover_points = F({2, 3, 4});
    auto verifier_points = F({5, 9, 6});
    Multilinear poly(F({0, 7, 0, 5, 0, 7, 4, 9}));
    TrustedSetup tau = TrustedSetup::setup(prover_points, true);
    G1Affine commit = MultilinearKZG::commitment(poly, tau);
    MultilinearKZGProof proof = MultilinearKZG::open(poly, verifier_points, tau);
    EXPECT(MultilinearKZG::verify(commit, verifier_points, proof, tau) == true);
}

static void test_kzg_2() {                 // multilinear_kzg.rs:157-197
    auto prover_points = F({12, 9, 28, 40});
    auto tampered_prover_points = F({12, 19, 28, 40});
    auto verifier_points = F({54, 90, 76, 160});
    Multilinear poly(F({0, 0, 0, 2, 0, 0, 10, 12, 0, -12, 4, -6, 0, -12, 14, 4}));    // 4ac + 10bc + 2cd - 12ad
    TrustedSetup tau = TrustedSetup::setup(prover_points, true);
    TrustedSetup tampered_tau = TrustedSetup::setup(tampered_prover_points, true);
    G1Affine commit = MultilinearKZG::commitment(poly, tau);
    MultilinearKZGProof proof = MultilinearKZG::open(poly, verifier_points, tau);
    EXPECT(MultilinearKZG::verify(commit, verifier_points, proof, tau) == true);
    EXPECT(MultilinearKZG::verify(commit, verifier_points, proof, tampered_tau) == false);
}

static void test_univariate_kzg() {        // univariate_kzg.rs:111-129
    TrustedSetup srs = UnivariateKZG::generate_srs(Fr::from(10), 4, true);
    DenseUnivariatePolynomial poly(F({1, 2, 3, 4, 5}));
    G1Affine commitment = UnivariateKZG::commitment(poly, srs);
    UnivariateKZGProof proof = UnivariateKZG::open(poly, Fr::from(2), srs);
    EXPECT(UnivariateKZG::verify(commitment, Fr::from(2), proof, srs));
}

static void test_univariate_kzg_invalid_opening() {   // univariate_kzg.rs:131-150
    TrustedSetup srs = UnivariateKZG::generate_srs(Fr::from(10), 4, true);
    DenseUnivariatePolynomial poly(F({1, 2, 3, 4, 5}));
    G1Affine commitment = UnivariateKZG::commitment(poly, srs);
    UnivariateKZGProof proof = UnivariateKZG::open(poly, Fr::from(2), srs);
    EXPECT(UnivariateKZG::verify(commitment, Fr::from(4), proof, srs) == false);
}

static void test_verify_without_g2_half_throws() {
    TrustedSetup srs = TrustedSetup::setup(F({2, 3, 4}));
    Multilinear poly(F({0, 7, 0, 5, 0, 7, 4, 9}));
    G1Affine commit = MultilinearKZG::commitment(poly, srs);
    MultilinearKZGProof proof = MultilinearKZG::open(poly, F({5, 9, 6}), srs);
    bool threw = false;
    try { MultilinearKZG::verify(commit, F({5, 9, 6}), proof, srs); } catch (const std::invalid_argument&) { threw = true; }
    EXPECT(threw);
}

int main() {
    struct { const char* n; void (*f)(); } tests[] = {
        {"test_kzg_1", test_kzg_1}, {"test_kzg_2", test_kzg_2}, {"test_univariate_kzg", test_univariate_kzg},
        {"test_univariate_kzg_invalid_opening", test_univariate_kzg_invalid_opening},
        {"test_verify_without_g2_half_throws", test_verify_without_g2_half_throws}};
    for (auto& t : tests) {
        int before = g_failed;
        try { t.f(); } catch (const std::exception& e) { std::printf("  EXCEPTION in %s: %s\n", t.n, e.what()); ++g_failed; }
        std::printf("%s %s\n", g_failed == before ? "ok    " : "FAILED", t.n);
        ++g_run;
    }
    std::printf("%d tests, %d failed\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
