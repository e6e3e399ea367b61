// test_mirror_dense_points.cpp -- DenseUnivariatePolynomial::{evaluate(points), evaluate_batch, interpolate, interpolate_batch} of the
// C++ host mirror (include/zkhip.hpp) against the CPU oracle: a polynomial of 300 coefficients at 70 points; three polynomials at their
// own and at shared points; interpolation through 5 and 300 points checked by the oracle's Horner at every node; a batch with shared
// and with own nodes against the single calls; the all-zero values; what the mirror throws.
// Built and run by tests/test_cpp_mirror_dense_points.py.  Exit code 0 = all passed.
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
static Fr horner(const std::vector<Fr>& coeffs, const Fr& x) {
    Fr o;
    ora_dense_evaluate((fr_t*)&o, reinterpret_cast<const fr_t*>(coeffs.data()), coeffs.size(), reinterpret_cast<const fr_t*>(&x));
    return o;
}

int main() {
    // evaluation
    const std::vector<Fr> coeffs = random_fr(300, 17000);
    std::vector<Fr> points = random_fr(70, 17001);
    points[0] = Fr::zero();
    points[1] = Fr::one();
    points[2] = Fr::from(-1);
    const DenseUnivariatePolynomial poly(coeffs);
    const auto values = poly.evaluate(points);
    EXPECT(values.size() == points.size());
    for (size_t k = 0; k < values.size(); ++k) {
        EXPECT(values[k] == horner(coeffs, points[k]));
        if (k < 4) EXPECT(values[k] == poly.evaluate(points[k]));                       // the single call, limb for limb
    }
    EXPECT(poly.evaluate(std::vector<Fr>()).empty());
    const auto of_empty = DenseUnivariatePolynomial(std::vector<Fr>()).evaluate(points);
    for (const Fr& v : of_empty) EXPECT(v == Fr::zero());
    constexpr size_t B = 3;
    std::vector<DenseUnivariatePolynomial> polys;
    std::vector<std::vector<Fr>> cs(B), ps(B);
    for (size_t b = 0; b < B; ++b) {
        cs[b] = random_fr(40, 17100 + b);
        ps[b] = random_fr(9, 17200 + b);
        polys.emplace_back(cs[b]);
    }
    const auto own = DenseUnivariatePolynomial::evaluate_batch(polys, ps);
    const auto shared = DenseUnivariatePolynomial::evaluate_batch(polys, {ps[1]});
    EXPECT(own.size() == B && shared.size() == B);
    for (size_t b = 0; b < B && b < own.size() && b < shared.size(); ++b)
        for (size_t k = 0; k < 9; ++k) {
            EXPECT(own[b][k] == horner(cs[b], ps[b][k]));
            EXPECT(shared[b][k] == horner(cs[b], ps[1][k]));
        }
    // interpolation, checked by uniqueness: the interpolant has n coefficients and returns the values at the nodes
    for (size_t n : {(size_t)1, (size_t)5, (size_t)300}) {
        std::vector<Fr> xs = random_fr(n, 17300 + n), ys = random_fr(n, 17400 + n);
        xs[0] = Fr::zero();
        if (n > 1) xs[1] = Fr::one();
        const DenseUnivariatePolynomial p = DenseUnivariatePolynomial::interpolate(ys, xs);
        EXPECT(p.n == n);
        const auto c = p.coefficients();
        for (size_t i = 0; i < n; ++i) EXPECT(horner(c, xs[i]) == ys[i]);
        const DenseUnivariatePolynomial z = DenseUnivariatePolynomial::interpolate(std::vector<Fr>(n, Fr::zero()), xs);
        EXPECT(z.n == n && z.degree() == 0 && z.evaluate(xs[0]) == Fr::zero());
    }
    {
        const size_t n = 17;
        std::vector<std::vector<Fr>> xs(B), ys(B);
        for (size_t b = 0; b < B; ++b) { xs[b] = random_fr(n, 17500 + b); ys[b] = random_fr(n, 17600 + b); }
        const auto each = DenseUnivariatePolynomial::interpolate_batch(ys, xs);
        const auto one_set = DenseUnivariatePolynomial::interpolate_batch(ys, {xs[2]});
        EXPECT(each.size() == B && one_set.size() == B);
        for (size_t b = 0; b < B && b < each.size() && b < one_set.size(); ++b) {
            EXPECT(each[b] == DenseUnivariatePolynomial::interpolate(ys[b], xs[b]).coefficients());
            EXPECT(one_set[b] == DenseUnivariatePolynomial::interpolate(ys[b], xs[2]).coefficients());
        }
        bool threw = false;
        xs[1][7] = xs[1][3];
        try { DenseUnivariatePolynomial::interpolate_batch(ys, xs); } catch (const std::exception&) { threw = true; }
        EXPECT(threw);                                                                  // a repeated node in one job of three
        threw = false;
        try { DenseUnivariatePolynomial::interpolate(ys[0], random_fr(n + 1, 1)); } catch (const std::exception&) { threw = true; }
        EXPECT(threw);                                                                  // as many ys as xs
        threw = false;
        try { DenseUnivariatePolynomial::evaluate_batch(polys, {ps[0], ps[1]}); } catch (const std::exception&) { threw = true; }
        EXPECT(threw);                                                                  // one row of points, or one per polynomial
    }
    EXPECT(DenseUnivariatePolynomial::interpolate_batch({}, {}).empty());
    std::printf("dense points mirror: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
