// plonk_verify_kernels.hpp -- the device side of zkhip_plonk_verify_batch (plonk/src/protocol/verifier.rs:62-172) for gfx950.
//
//   plonk_points_check_kernel  curve and subgroup membership of the key's commitments, once per key
//   plonk_pi_kernel            PI(zeta_b) of every proof from its evaluation-form column, barycentric:
//                              PI(zeta) = (zeta^n - 1) / n * sum_i pi_i w^i / (zeta - w^i); grid (row blocks) x batch, PV_PI_E = 8 consecutive
//                              rows per lane whose denominators share one inversion (Montgomery's trick), one partial per workgroup
//   plonk_pi_finish_kernel     adds a proof's partials, applies the factor and adds PI(zeta_b) to the generator's scalar (the host wrote
//                              that scalar without it)
//   plonk_terms_kernel         one lane per (proof, term): validate the point, multiply by the canonical scalar, store XYZZ
//   plonk_combine_kernel       one lane per proof: the two sums, affine; `right` against prepared entry 0 and -`left` against entry 1
//
// The terms of one proof, in the order of the scalar table the host writes (verifier.rs:101-169):
//   0..7   q_m, q_l, q_r, q_o, q_c, sigma_1, sigma_2, sigma_3 (the key's commitments) with a b, a, b, c, 1, nu^4, nu^5, -k_s3
//   8..10  a, b, c with nu, nu^2, nu^3            11  the accumulator with k_acc
//   12..14 t_low, t_mid, t_high with -z_H, -z_H zeta^n, -z_H zeta^2n
//   15, 16 W_zeta, W_zeta_omega with zeta, mu zeta w                17  G with -es                    (0..17: `right`)
//   18, 19 W_zeta, W_zeta_omega with 1, mu                                                             (`left`)
// Terms 4 and 18 have the scalar one by construction: an addition, no ladder.
//
// Registers: the ladders are those of pairing.hpp (g1_mul<8> around the out-of-line Fq product), so the term kernel's budget is
// kzg_terms_kernel's.  The per-proof kernels run 64 lanes per workgroup, as the pairing's do.
#pragma once
#include "pairing.hpp"
#include "plonk_kernels.hpp"
#include "srs_kernels.hpp"

namespace zk {

constexpr int PV_BLOCK = 64;              // lanes per workgroup of the per-proof and per-term kernels
constexpr int PV_TERMS = 20;              // terms per proof
constexpr int PV_RIGHT = 18;              // terms 0 .. PV_RIGHT - 1 sum to `right`, the rest to `left`
constexpr int PV_TERM_QC = 4, PV_TERM_G = 17, PV_TERM_LEFT_WZ = 18;
constexpr int PV_VK_POINTS = 8, PV_PROOF_POINTS = 9;
constexpr int PV_PI_T = 128;              // lanes per workgroup of the PI pass
constexpr int PV_PI_E = 8;                // consecutive rows per lane: one inversion (~380 products) for the eight denominators
constexpr int PV_PI_ROWS = PV_PI_T * PV_PI_E;

// bad[i] = 1: point i is finite and not a valid G1 element
static __global__ __launch_bounds__(PV_BLOCK) void plonk_points_check_kernel(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n,
                                                                            uint8_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (i >= n) return;
    bad[i] = inf[i] || g1_point_valid(load_affine(xy, i)) ? 0 : 1;
}

// partial[b * gridDim.x + block] = sum over the block's rows of pi_i w^i / (zeta_b - w^i).  A row with zeta_b = w^i takes one for its
// denominator, adds nothing and leaves i + 1 in hit[b] (zeroed by the caller; the w^i are distinct, so at most one row writes).
static __global__ __launch_bounds__(PV_PI_T) void plonk_pi_kernel(const uint64_t* const* __restrict__ cols, const uint64_t* __restrict__ omega_pow,
                                                                 const uint64_t* __restrict__ zetas, size_t n, uint64_t* __restrict__ partial,
                                                                 unsigned long long* __restrict__ hit) {
    __shared__ Fr smem[PV_PI_T / 64];
    const size_t b = blockIdx.y;
    const uint64_t* __restrict__ col = cols[b];
    const Fr zeta = load_fr(zetas, b);
    const size_t base = ((size_t)blockIdx.x * PV_PI_T + threadIdx.x) * PV_PI_E;
    // forward: pre[j] = den_0 .. den_{j-1}.  Only the prefix products are kept: the way back reads w^i again, which costs a load and a
    // subtraction where keeping den_j and pi_j w^i would cost sixteen registers a row.
    Fr pre[PV_PI_E];
    Fr run = Fr::one();
#pragma unroll
    for (int j = 0; j < PV_PI_E; ++j) {
        const size_t i = base + j;
        pre[j] = run;
        if (i < n) {
            const Fr d = zeta - load_fr(omega_pow, i);
            if (d.is_zero()) hit[b] = (unsigned long long)i + 1;
            else run = run * d;
        }
    }
    Fr sum = Fr::zero();
    if (base < n) {
        Fr inv = fr_inverse(run);                      // 1 / (den_0 .. den_{E-1})
#pragma unroll
        for (int j = PV_PI_E - 1; j >= 0; --j) {
            const size_t i = base + j;
            if (i < n) {
                const Fr w = load_fr(omega_pow, i);
                const Fr d = zeta - w;
                if (!d.is_zero()) {                    // else its denominator was one: nothing to add, nothing to unwind
                    sum = sum + load_fr(col, i) * w * (inv * pre[j]);
                    inv = inv * d;
                }
            }
        }
    }
    sum = block_reduce_fr(sum, smem);
    if (threadIdx.x == 0) store_fr(partial, b * gridDim.x + blockIdx.x, sum);
}

// One lane per proof: PI(zeta_b) = factor_b * (sum of its partials), or pi_i itself where zeta_b = w^i (what the coefficient form
// evaluates to there).  g_scalars (stride g_stride elements; may be null) += PI(zeta_b); pi_out (may be null) receives PI(zeta_b).
static __global__ __launch_bounds__(PV_BLOCK) void plonk_pi_finish_kernel(const uint64_t* const* __restrict__ cols, const uint64_t* __restrict__ partial,
                                                                        const unsigned long long* __restrict__ hit,
                                                                        const uint64_t* __restrict__ factors, size_t batch, size_t n_blocks,
                                                                        uint64_t* __restrict__ g_scalars, size_t g_stride,
                                                                        uint64_t* __restrict__ pi_out) {
    const size_t b = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (b >= batch) return;
    Fr v;
    if (hit[b]) {
        v = load_fr(cols[b], (size_t)(hit[b] - 1));
    } else {
        Fr s = Fr::zero();
        for (size_t k = 0; k < n_blocks; ++k) s = s + load_fr(partial, b * n_blocks + k);
        v = s * load_fr(factors, b);
    }
    if (g_scalars) store_fr(g_scalars, b * g_stride, load_fr(g_scalars, b * g_stride) + v);
    if (pi_out) store_fr(pi_out, b, v);
}

// Lane t = b * PV_TERMS + j: term j of proof b (table above).  vk: the key's eight commitments, validated with the key; points: nine per
// proof, validated here (bad[t] = 1: finite and off the curve, outside the subgroup or with an unreduced coordinate); scalars:
// Montgomery form, PV_TERMS per proof.  A point at infinity is the identity.
static __global__ __launch_bounds__(PV_BLOCK) void plonk_terms_kernel(const uint64_t* __restrict__ vk_xy, const uint8_t* __restrict__ vk_inf,
                                                                    const uint64_t* __restrict__ points, const uint8_t* __restrict__ points_inf,
                                                                    const uint64_t* __restrict__ scalars, size_t batch,
                                                                    uint64_t* __restrict__ terms, uint8_t* __restrict__ bad) {
    const size_t t = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (t >= batch * PV_TERMS) return;
    const size_t b = t / PV_TERMS;
    const int j = (int)(t % PV_TERMS);
    // proof point of term j >= 8: as, bs, cs, accumulator, t_low, t_mid, t_high, w_zeta, w_zeta_omega, (G), w_zeta, w_zeta_omega
    const int src = j < PV_VK_POINTS ? j : j < PV_TERM_G ? j - PV_VK_POINTS : j - PV_VK_POINTS - 3;
    G1Affine pt = g1_generator();
    bool at_inf = false, ok = true;
    if (j < PV_VK_POINTS) {
        pt = load_affine(vk_xy, src);
        at_inf = vk_inf[src] != 0;
    } else if (j != PV_TERM_G) {
        pt = load_affine(points, b * PV_PROOF_POINTS + src);
        at_inf = points_inf[b * PV_PROOF_POINTS + src] != 0;
        ok = at_inf || g1_point_valid(pt);
    }
    bad[t] = ok ? 0 : 1;
    G1Xyzz acc = G1Xyzz::identity();
    if (!at_inf) {
        if (j == PV_TERM_QC || j == PV_TERM_LEFT_WZ) {
            g1_madd(acc, pt, false);
        } else {
            const Fr k = load_fr(scalars, t).from_mont();
            acc = g1_mul<8>(pt, k.l, false);
        }
    }
    store_xyzz(terms, t, acc);
}

__device__ __forceinline__ bool pv_store_affine(const G1Xyzz& acc, bool negate, uint64_t* __restrict__ xy, uint64_t* __restrict__ xy_plain) {
    if (acc.is_identity()) {
        store_fq(xy, Fq::zero()); store_fq(xy + 6, Fq::zero());
        if (xy_plain) { store_fq(xy_plain, Fq::zero()); store_fq(xy_plain + 6, Fq::zero()); }
        return false;
    }
    const Fq inv = pair_fq_inverse(fq_mul(acc.zz, acc.zzz));
    const Fq x = fq_mul(acc.x, fq_mul(inv, acc.zzz)), y = fq_mul(acc.y, fq_mul(inv, acc.zz));
    store_fq(xy, x); store_fq(xy + 6, negate ? y.neg() : y);
    if (xy_plain) { store_fq(xy_plain, x); store_fq(xy_plain + 6, y); }
    return true;
}

// One lane per proof.  pair_xy / pair_inf[2 b], [2 b + 1]: `right` and -`left`, the pairing's G1 arguments against prepared entries 0
// and 1; out_xy / out_inf: `right` and `left` as the reference names them.  A sum that is the identity has its flag set and zero
// coordinates.  A proof with a bad term gives two identities: its verdict is the caller's to overwrite.
static __global__ __launch_bounds__(PV_BLOCK) void plonk_combine_kernel(const uint64_t* __restrict__ terms, const uint8_t* __restrict__ bad, size_t batch,
                                                                      uint64_t* __restrict__ pair_xy, uint8_t* __restrict__ pair_inf,
                                                                      uint64_t* __restrict__ out_xy, uint8_t* __restrict__ out_inf) {
    const size_t b = (size_t)blockIdx.x * PV_BLOCK + threadIdx.x;
    if (b >= batch) return;
    bool any_bad = false;
    for (int j = 0; j < PV_TERMS; ++j) any_bad = any_bad || bad[b * PV_TERMS + j] != 0;
    G1Xyzz right = G1Xyzz::identity(), left = G1Xyzz::identity();
    if (!any_bad) {
        right = load_xyzz(terms, b * PV_TERMS);
        for (int j = 1; j < PV_RIGHT; ++j) g1_add(right, load_xyzz(terms, b * PV_TERMS + j));
        left = load_xyzz(terms, b * PV_TERMS + PV_RIGHT);
        for (int j = PV_RIGHT + 1; j < PV_TERMS; ++j) g1_add(left, load_xyzz(terms, b * PV_TERMS + j));
    }
    const bool rf = pv_store_affine(right, false, pair_xy + 24 * b, out_xy + 24 * b);
    const bool lf = pv_store_affine(left, true, pair_xy + 24 * b + 12, out_xy + 24 * b + 12);
    pair_inf[2 * b] = out_inf[2 * b] = rf ? 0 : 1;
    pair_inf[2 * b + 1] = out_inf[2 * b + 1] = lf ? 0 : 1;
}

}  // namespace zk
