// pairing.hpp -- the BLS12-381 optimal ate pairing for gfx950, device side.
//
// Replaces, on the GPU, the `P::pairing` / `PairingOutput` arithmetic the reference's verifiers reach
// (kzg/src/multilinear_kzg.rs:90-112, kzg/src/utils.rs:42-60, kzg/src/univariate_kzg.rs:83-104) and the G2 group law of
// `generate_powers_of_tau_in_g2` (kzg/src/trusted_setup.rs:37-45).
//
// Tower (arkworks / zkcrypto): Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - (u + 1)), Fq12 = Fq6[w]/(w^2 - v).
// G2: the M-type sextic twist y^2 = x^3 + 4 (u + 1).  Lines come from homogeneous projective doubling / addition steps and
// are sparse Fq12 elements in the coefficients c0.c0, c0.c1, c1.c1 ("014").  The Miller loop runs over |x| = 0xd201000000010000
// and conjugates (x < 0); the final exponentiation is exactly f^((p^12 - 1) / r): easy part (p^6 - 1)(p^2 + 1), hard part
// ((x - 1)^2 / 3)(x + p)(x^2 + p^2 - 1) + 1 with cyclotomic squarings.  GT values therefore have one encoding.
//
// Registers: an Fq12 is 144 VGPRs, a product of two needs both plus its result.  The Fq12 operations are out of line and take
// their operands by reference, so their values live in the lane's private memory at those boundaries; inside them the Fq2
// arithmetic runs in registers around the out-of-line Fq product of g1.hpp.
#pragma once
#include "g1.hpp"
#include "pairing_consts.hpp"

namespace zk {

__device__ __forceinline__ Fq fq_from(const uint32_t (&v)[12]) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 12; ++i) r.l[i] = v[i];
    return r;
}
// a^(p-2) (Fermat)
__device__ __noinline__ Fq pair_fq_inverse(Fq a) {
    Fq acc = Fq::one();
    for (int w = 11; w >= 0; --w) {
        uint32_t e = 0;
#pragma unroll
        for (int q = 0; q < 12; ++q) if (q == w) e = (q == 0) ? FqParams::p(0) - 2 : FqParams::p(q);
        for (int b = 31; b >= 0; --b) {
            acc = fq_sqr(acc);
            if ((e >> b) & 1) acc = fq_mul(acc, a);
        }
    }
    return acc;
}

// ---- Fq2 ------------------------------------------------------------------------------------------------------------
struct Fq2 {
    Fq c0, c1;
    __device__ __forceinline__ static Fq2 zero() { return {Fq::zero(), Fq::zero()}; }
    __device__ __forceinline__ static Fq2 one() { return {Fq::one(), Fq::zero()}; }
    __device__ __forceinline__ bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    __device__ __forceinline__ bool operator==(const Fq2& o) const { return c0 == o.c0 && c1 == o.c1; }
};
__device__ __forceinline__ Fq2 operator+(const Fq2& a, const Fq2& b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
__device__ __forceinline__ Fq2 operator-(const Fq2& a, const Fq2& b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
__device__ __forceinline__ Fq2 f2_neg(const Fq2& a) { return {a.c0.neg(), a.c1.neg()}; }
__device__ __forceinline__ Fq2 f2_dbl(const Fq2& a) { return {a.c0.dbl(), a.c1.dbl()}; }
__device__ __forceinline__ Fq2 f2_conj(const Fq2& a) { return {a.c0, a.c1.neg()}; }
__device__ __forceinline__ Fq2 operator*(const Fq2& a, const Fq2& b) {     // Karatsuba: 3 products
    const Fq v0 = fq_mul(a.c0, b.c0), v1 = fq_mul(a.c1, b.c1);
    return {v0 - v1, fq_mul(a.c0 + a.c1, b.c0 + b.c1) - v0 - v1};
}
__device__ __forceinline__ Fq2 f2_sqr(const Fq2& a) {                      // 2 products
    return {fq_mul(a.c0 + a.c1, a.c0 - a.c1), fq_mul(a.c0, a.c1).dbl()};
}
__device__ __forceinline__ Fq2 f2_mul_fq(const Fq2& a, const Fq& k) { return {fq_mul(a.c0, k), fq_mul(a.c1, k)}; }
__device__ __forceinline__ Fq2 f2_mul_xi(const Fq2& a) { return {a.c0 - a.c1, a.c0 + a.c1}; }   // * (u + 1)
__device__ __forceinline__ Fq2 f2_inverse(const Fq2& a) {
    const Fq t = pair_fq_inverse(fq_sqr(a.c0) + fq_sqr(a.c1));
    return {fq_mul(a.c0, t), fq_mul(a.c1, t).neg()};
}
__device__ __forceinline__ Fq2 load_fq2(const uint64_t* p) { return {load_fq(p), load_fq(p + 6)}; }
__device__ __forceinline__ void store_fq2(uint64_t* p, const Fq2& v) { store_fq(p, v.c0); store_fq(p + 6, v.c1); }

// ---- Fq6 ------------------------------------------------------------------------------------------------------------
struct Fq6 {
    Fq2 c0, c1, c2;
};
__device__ __forceinline__ Fq6 operator+(const Fq6& a, const Fq6& b) { return {a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
__device__ __forceinline__ Fq6 operator-(const Fq6& a, const Fq6& b) { return {a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
__device__ __forceinline__ Fq6 f6_neg(const Fq6& a) { return {f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
__device__ __forceinline__ Fq6 f6_mul_v(const Fq6& a) { return {f2_mul_xi(a.c2), a.c0, a.c1}; }   // * v
__device__ __forceinline__ Fq6 operator*(const Fq6& a, const Fq6& b) {     // Karatsuba: 6 Fq2 products
    const Fq2 v0 = a.c0 * b.c0, v1 = a.c1 * b.c1, v2 = a.c2 * b.c2;
    return {f2_mul_xi((a.c1 + a.c2) * (b.c1 + b.c2) - v1 - v2) + v0,
            (a.c0 + a.c1) * (b.c0 + b.c1) - v0 - v1 + f2_mul_xi(v2),
            (a.c0 + a.c2) * (b.c0 + b.c2) - v0 - v2 + v1};
}
// a * (b0 + b1 v)
__device__ __forceinline__ Fq6 f6_mul_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    const Fq2 v0 = a.c0 * b0, v1 = a.c1 * b1;
    return {f2_mul_xi((a.c1 + a.c2) * b1 - v1) + v0, (a.c0 + a.c1) * (b0 + b1) - v0 - v1, (a.c0 + a.c2) * b0 - v0 + v1};
}
// a * (b1 v)
__device__ __forceinline__ Fq6 f6_mul_1(const Fq6& a, const Fq2& b1) { return {f2_mul_xi(a.c2 * b1), a.c0 * b1, a.c1 * b1}; }
__device__ __forceinline__ Fq6 f6_inverse(const Fq6& a) {
    const Fq2 c0 = f2_sqr(a.c0) - f2_mul_xi(a.c1 * a.c2);
    const Fq2 c1 = f2_mul_xi(f2_sqr(a.c2)) - a.c0 * a.c1;
    const Fq2 c2 = f2_sqr(a.c1) - a.c0 * a.c2;
    const Fq2 t = f2_inverse(a.c0 * c0 + f2_mul_xi(a.c2 * c1 + a.c1 * c2));
    return {c0 * t, c1 * t, c2 * t};
}

// ---- Fq12 -----------------------------------------------------------------------------------------------------------
struct Fq12 {
    Fq6 c0, c1;
};
__device__ __forceinline__ Fq12 f12_one() {
    Fq12 r;
    r.c0 = {Fq2::one(), Fq2::zero(), Fq2::zero()};
    r.c1 = {Fq2::zero(), Fq2::zero(), Fq2::zero()};
    return r;
}
__device__ __forceinline__ bool f12_is_one(const Fq12& a) {
    return a.c0.c0 == Fq2::one() && a.c0.c1.is_zero() && a.c0.c2.is_zero() && a.c1.c0.is_zero() && a.c1.c1.is_zero() &&
           a.c1.c2.is_zero();
}
__device__ __forceinline__ void f12_conj(Fq12& a) { a.c1 = f6_neg(a.c1); }
__device__ __noinline__ void f12_mul(Fq12& r, const Fq12& a, const Fq12& b) {
    const Fq6 aa = a.c0 * b.c0, bb = a.c1 * b.c1;
    const Fq6 c1 = (a.c0 + a.c1) * (b.c0 + b.c1) - aa - bb;
    r.c0 = aa + f6_mul_v(bb);
    r.c1 = c1;
}
__device__ __noinline__ void f12_sqr(Fq12& a) {
    const Fq6 ab = a.c0 * a.c1;
    const Fq6 c0 = (a.c0 + a.c1) * (a.c0 + f6_mul_v(a.c1)) - ab - f6_mul_v(ab);
    a.c0 = c0;
    a.c1 = ab + ab;
}
// a *= c0 + c1 v + c4 v w  (a line)
__device__ __noinline__ void f12_mul_014(Fq12& a, const Fq2& c0, const Fq2& c1, const Fq2& c4) {
    const Fq6 aa = f6_mul_01(a.c0, c0, c1);
    const Fq6 bb = f6_mul_1(a.c1, c4);
    a.c1 = f6_mul_01(a.c1 + a.c0, c0, c1 + c4) - aa - bb;
    a.c0 = f6_mul_v(bb) + aa;
}
__device__ __noinline__ void f12_inverse(Fq12& a) {
    const Fq6 t = f6_inverse(a.c0 * a.c0 - f6_mul_v(a.c1 * a.c1));
    a.c0 = a.c0 * t;
    a.c1 = f6_neg(a.c1 * t);
}
// x -> x^(p^k), k = 1, 2: coefficient i is conjugated k times and multiplied by PAIR_GAMMA[k-1][i]
template <int K>
__device__ __noinline__ void f12_frobenius(Fq12& a) {
    Fq2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
#pragma unroll
    for (int i = 1; i < 6; ++i) {
        Fq2 v = *c[i];
        if (K & 1) v = f2_conj(v);
        *c[i] = v * Fq2{fq_from(PAIR_GAMMA[K - 1][i][0]), fq_from(PAIR_GAMMA[K - 1][i][1])};
    }
    if (K & 1) a.c0.c0 = f2_conj(a.c0.c0);
}
// Granger-Scott squaring of an element of the cyclotomic subgroup (after the easy part)
__device__ __forceinline__ void f2_sqr4(Fq2& t0, Fq2& t1, const Fq2& x, const Fq2& y) {   // (x + y s)^2, s^2 = xi
    const Fq2 tmp = x * y;
    t0 = (x + y) * (f2_mul_xi(y) + x) - tmp - f2_mul_xi(tmp);
    t1 = f2_dbl(tmp);
}
__device__ __noinline__ void f12_cyclotomic_sqr(Fq12& a) {
    Fq2 t0, t1, t2, t3, t4, t5;
    f2_sqr4(t0, t1, a.c0.c0, a.c1.c1);
    f2_sqr4(t2, t3, a.c1.c0, a.c0.c2);
    f2_sqr4(t4, t5, a.c0.c1, a.c1.c2);
    a.c0.c0 = f2_dbl(t0 - a.c0.c0) + t0;                 // 3 t0 - 2 z0
    a.c1.c1 = f2_dbl(t1 + a.c1.c1) + t1;                 // 3 t1 + 2 z1
    const Fq2 t5x = f2_mul_xi(t5);
    a.c1.c0 = f2_dbl(t5x + a.c1.c0) + t5x;               // 3 xi t5 + 2 z2
    a.c0.c2 = f2_dbl(t4 - a.c0.c2) + t4;                 // 3 t4 - 2 z3
    a.c0.c1 = f2_dbl(t2 - a.c0.c1) + t2;                 // 3 t2 - 2 z4
    a.c1.c2 = f2_dbl(t3 + a.c1.c2) + t3;                 // 3 t3 + 2 z5
}
// r = a^e for the NBITS-bit exponent e (top bit set), cyclotomic squarings
template <int NBITS, class Bit>
__device__ __forceinline__ void f12_cyclotomic_pow(Fq12& r, const Fq12& a, Bit bit) {
    r = a;
    for (int b = NBITS - 2; b >= 0; --b) {
        f12_cyclotomic_sqr(r);
        if (bit(b)) f12_mul(r, r, a);
    }
}
// r = a^x, x < 0 (the inverse of a unitary element is its conjugate)
__device__ __noinline__ void f12_exp_by_x(Fq12& r, const Fq12& a) {
    f12_cyclotomic_pow<64>(r, a, [](int b) { return (PAIR_X_ABS >> b) & 1; });
    f12_conj(r);
}
// f^((p^12 - 1) / r), exactly
__device__ __noinline__ void final_exponentiation(Fq12& f) {
    Fq12 t = f, u, a, b, d;
    f12_conj(t);
    f12_inverse(f);
    f12_mul(t, t, f);                         // f^(p^6 - 1)
    u = t;
    f12_frobenius<2>(u);
    f12_mul(f, u, t);                         // ^(p^2 + 1): f is now in the cyclotomic subgroup
    f12_cyclotomic_pow<126>(a, f, [](int b) { return (PAIR_HARD_C[b >> 5] >> (b & 31)) & 1; });   // a = f^((x-1)^2/3)
    f12_exp_by_x(b, a);
    f12_frobenius<1>(a);
    f12_mul(b, b, a);                         // b = a^(x + p)
    f12_exp_by_x(u, b);
    f12_exp_by_x(d, u);                       // b^(x^2)
    u = b;
    f12_frobenius<2>(u);
    f12_mul(d, d, u);                         // * b^(p^2)
    f12_conj(b);
    f12_mul(d, d, b);                         // * b^(-1)
    f12_mul(f, d, f);                         // * f
}

// ---- G2 -------------------------------------------------------------------------------------------------------------
struct G2Affine {   // 192 bytes in memory: x.c0, x.c1, y.c0, y.c1 (uint64 Montgomery limbs); infinity in a side array
    Fq2 x, y;
};
struct G2Jac {      // Jacobian (x = X/Z^2, y = Y/Z^3), Z = 0 is the identity
    Fq2 x, y, z;
    __device__ __forceinline__ bool is_identity() const { return z.is_zero(); }
};
__device__ __forceinline__ G2Affine g2_generator() {
    return {{fq_from(PAIR_G2_GEN[0]), fq_from(PAIR_G2_GEN[1])}, {fq_from(PAIR_G2_GEN[2]), fq_from(PAIR_G2_GEN[3])}};
}
__device__ __forceinline__ Fq2 g2_b() { const Fq f = fq_from(PAIR_FOUR); return {f, f}; }
__device__ __forceinline__ G2Affine load_g2(const uint64_t* p, size_t i) { return {load_fq2(p + 24 * i), load_fq2(p + 24 * i + 12)}; }
__device__ __forceinline__ void store_g2(uint64_t* p, size_t i, const G2Affine& a) {
    store_fq2(p + 24 * i, a.x);
    store_fq2(p + 24 * i + 12, a.y);
}
__device__ __forceinline__ bool g2_on_curve(const G2Affine& a) { return f2_sqr(a.y) == f2_sqr(a.x) * a.x + g2_b(); }
__device__ __forceinline__ G2Affine g2_neg(const G2Affine& a) { return {a.x, f2_neg(a.y)}; }

// dbl-2009-l (a = 0)
__device__ __noinline__ void g2_double(G2Jac& p) {
    if (p.is_identity()) return;
    const Fq2 a = f2_sqr(p.x), b = f2_sqr(p.y), c = f2_sqr(b);
    const Fq2 d = f2_dbl(f2_sqr(p.x + b) - a - c);
    const Fq2 e = f2_dbl(a) + a, f = f2_sqr(e);
    const Fq2 x3 = f - f2_dbl(d);
    const Fq2 c8 = f2_dbl(f2_dbl(f2_dbl(c)));
    p.z = f2_dbl(p.y * p.z);
    p.y = e * (d - x3) - c8;
    p.x = x3;
}
// acc += q (affine), complete: identity accumulator, doubling and inverse handled (madd-2007-bl)
__device__ __noinline__ void g2_madd(G2Jac& acc, const G2Affine& q) {
    if (acc.is_identity()) { acc = {q.x, q.y, Fq2::one()}; return; }
    const Fq2 z1z1 = f2_sqr(acc.z);
    const Fq2 u2 = q.x * z1z1, s2 = q.y * acc.z * z1z1;
    const Fq2 h = u2 - acc.x, r = f2_dbl(s2 - acc.y);
    if (h.is_zero()) {
        if (r.is_zero()) g2_double(acc);
        else acc.z = Fq2::zero();
        return;
    }
    const Fq2 hh = f2_sqr(h), i = f2_dbl(f2_dbl(hh)), j = h * i, v = acc.x * i;
    const Fq2 x3 = f2_sqr(r) - j - f2_dbl(v);
    const Fq2 y3 = r * (v - x3) - f2_dbl(acc.y * j);
    acc.z = f2_sqr(acc.z + h) - z1z1 - hh;
    acc.x = x3;
    acc.y = y3;
}
// k * q for a canonical scalar of NW 32-bit words, most significant bit first
template <int NW>
__device__ __forceinline__ G2Jac g2_mul(const G2Affine& q, const uint32_t (&k)[NW]) {
    G2Jac acc = {Fq2::zero(), Fq2::zero(), Fq2::zero()};
    for (int b = 32 * NW - 1; b >= 0; --b) {
        g2_double(acc);
        uint32_t word = k[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) if (w == (b >> 5)) word = k[w];
        if ((word >> (b & 31)) & 1) g2_madd(acc, q);
    }
    return acc;
}
// in the prime-order subgroup: r * q = O
__device__ __forceinline__ bool g2_in_subgroup(const G2Affine& q) {
    uint32_t r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = PAIR_R[i];
    return g2_mul<8>(q, r).is_identity();
}
__device__ __forceinline__ bool g2_to_affine(const G2Jac& p, G2Affine& out) {
    if (p.is_identity()) { out = {Fq2::zero(), Fq2::zero()}; return false; }
    const Fq2 zi = f2_inverse(p.z), zi2 = f2_sqr(zi);
    out = {p.x * zi2, p.y * zi2 * zi};
    return true;
}

// ---- checks for verifier inputs -------------------------------------------------------------------------------------
// limbs as the caller wrote them: below the modulus, or not a field element.  The arithmetic above is stated for reduced operands
// only, so this comes before any product of an input.
template <class P>
__device__ __forceinline__ bool fp_is_reduced(const Fp<P>& a) {
    bool lt = false, decided = false;
#pragma unroll
    for (int i = Fp<P>::N - 1; i >= 0; --i) {
        const uint32_t p = P::p(i);
        if (!decided && a.l[i] != p) { lt = a.l[i] < p; decided = true; }
    }
    return lt;
}
__device__ __forceinline__ bool fq_is_reduced(const Fq& a) { return fp_is_reduced(a); }
__device__ __forceinline__ bool fr_is_reduced(const Fr& a) { return fp_is_reduced(a); }
__device__ __forceinline__ bool g1_on_curve(const G1Affine& a) {
    return fq_sqr(a.y) == fq_mul(fq_sqr(a.x), a.x) + fq_from(PAIR_FOUR);
}
// k * p, canonical scalar of NW words, XYZZ
template <int NW>
__device__ __forceinline__ G1Xyzz g1_mul(const G1Affine& p, const uint32_t (&k)[NW], bool neg) {
    G1Xyzz acc = G1Xyzz::identity();
    for (int b = 32 * NW - 1; b >= 0; --b) {
        acc = g1_double(acc);
        uint32_t word = k[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) if (w == (b >> 5)) word = k[w];
        if ((word >> (b & 31)) & 1) g1_madd(acc, p, neg);
    }
    return acc;
}
__device__ __forceinline__ bool g1_in_subgroup(const G1Affine& p) {
    uint32_t r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = PAIR_R[i];
    return g1_mul<8>(p, r, false).is_identity();
}
// finite points only: coordinates reduced, on y^2 = x^3 + 4, of order r
__device__ __forceinline__ bool g1_point_valid(const G1Affine& p) {
    return fq_is_reduced(p.x) && fq_is_reduced(p.y) && g1_on_curve(p) && g1_in_subgroup(p);
}
// finite points only: the four coordinates reduced, on the twist, of order r
__device__ __forceinline__ bool g2_point_valid(const G2Affine& q) {
    return fq_is_reduced(q.x.c0) && fq_is_reduced(q.x.c1) && fq_is_reduced(q.y.c0) && fq_is_reduced(q.y.c1) && g2_on_curve(q) &&
           g2_in_subgroup(q);
}

// ---- Miller loop ----------------------------------------------------------------------------------------------------
// Line coefficients (c0, c1, c2) of one step, evaluated at P = (px, py) as c0 + (c1 px) v + (c2 py) v w.
struct Line {
    Fq2 c0, c1, c2;
};
constexpr int PAIR_LINES = 68;                             // 63 doubling steps + 5 addition steps over |x|
constexpr size_t PREP_LINE_U64 = 36;                       // one line: 3 Fq2 = 6 Fq
constexpr size_t PREP_STRIDE_U64 = PAIR_LINES * PREP_LINE_U64 + 8;   // + a header word: 1 = the point at infinity

// T = 2 T (homogeneous projective), line through T
__device__ __noinline__ void g2_double_step(Fq2 (&t)[3], Line& l) {
    const Fq two_inv = fq_from(PAIR_TWO_INV);
    const Fq2 a = f2_mul_fq(t[0] * t[1], two_inv), b = f2_sqr(t[1]), c = f2_sqr(t[2]);
    const Fq2 e = g2_b() * (f2_dbl(c) + c), f = f2_dbl(e) + e;
    const Fq2 g = f2_mul_fq(b + f, two_inv);
    const Fq2 h = f2_sqr(t[1] + t[2]) - (b + c);
    const Fq2 j = f2_sqr(t[0]), es = f2_sqr(e);
    l = {e - b, f2_dbl(j) + j, f2_neg(h)};
    t[0] = a * (b - f);
    t[1] = f2_sqr(g) - (f2_dbl(es) + es);
    t[2] = b * h;
}
// T = T + Q, line through T and Q
__device__ __noinline__ void g2_add_step(Fq2 (&t)[3], const G2Affine& q, Line& l) {
    const Fq2 theta = t[1] - q.y * t[2], lambda = t[0] - q.x * t[2];
    const Fq2 c = f2_sqr(theta), d = f2_sqr(lambda), e = lambda * d, f = t[2] * c, g = t[0] * d;
    const Fq2 h = e + f - f2_dbl(g);
    l = {theta * q.x - lambda * q.y, f2_neg(theta), lambda};
    t[0] = lambda * h;
    t[1] = theta * (g - h) - e * t[1];
    t[2] = t[2] * e;
}
__device__ __forceinline__ void f12_mul_line(Fq12& f, const Line& l, const G1Affine& p) {
    f12_mul_014(f, l.c0, f2_mul_fq(l.c1, p.x), f2_mul_fq(l.c2, p.y));
}
__device__ __forceinline__ Line load_line(const uint64_t* p) { return {load_fq2(p), load_fq2(p + 12), load_fq2(p + 24)}; }
__device__ __forceinline__ void store_line(uint64_t* p, const Line& l) {
    store_fq2(p, l.c0); store_fq2(p + 12, l.c1); store_fq2(p + 24, l.c2);
}

// f_{|x|, Q}(P), conjugated.  `prep`: the 68 lines of Q (zkhip_g2_prepare), or nullptr to compute them from `q` on the way.
__device__ __forceinline__ void miller_loop(Fq12& f, const G1Affine& p, const G2Affine& q, const uint64_t* prep) {
    f = f12_one();
    Fq2 t[3] = {q.x, q.y, Fq2::one()};
    int k = 0;
    for (int b = 62; b >= 0; --b) {
        f12_sqr(f);
        Line l;
        if (prep) l = load_line(prep + PREP_LINE_U64 * k);
        else g2_double_step(t, l);
        ++k;
        f12_mul_line(f, l, p);
        if ((PAIR_X_ABS >> b) & 1) {
            if (prep) l = load_line(prep + PREP_LINE_U64 * k);
            else g2_add_step(t, q, l);
            ++k;
            f12_mul_line(f, l, p);
        }
    }
    f12_conj(f);
}

__device__ __forceinline__ void load_f12(const uint64_t* p, Fq12& f) {
    f.c0 = {load_fq2(p), load_fq2(p + 12), load_fq2(p + 24)};
    f.c1 = {load_fq2(p + 36), load_fq2(p + 48), load_fq2(p + 60)};
}
__device__ __forceinline__ void store_f12(uint64_t* p, const Fq12& f) {
    store_fq2(p, f.c0.c0); store_fq2(p + 12, f.c0.c1); store_fq2(p + 24, f.c0.c2);
    store_fq2(p + 36, f.c1.c0); store_fq2(p + 48, f.c1.c1); store_fq2(p + 60, f.c1.c2);
}

}  // namespace zk
