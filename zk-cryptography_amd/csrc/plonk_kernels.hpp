// plonk_kernels.hpp -- the univariate passes of the PLONK prover (plonk/src/protocol/prover.rs) for gfx950.
//
// Everything here is a streaming pass over coefficient or evaluation vectors of Fr, 32-byte elements moved with 16-byte accesses:
//   plonk_powers_kernel      tables c * b^i (coset shift g^i, g^-i, the domain's w^i, constant columns)
//   plonk_blind_kernel       p += (b_0 + b_1 X + ..) (X^n - 1)                                          prover.rs:104-111, 163-165
//   plonk_gp_*               the permutation accumulator (prover.rs:133-155) as ratio -> three-pass exclusive prefix PRODUCT;
//                            the denominators are inverted with Montgomery's trick per workgroup (one Fermat inversion each);
//                            the same pass checks the gate identity on every row.  No workgroup waits on another.
//   plonk_quotient_kernel    t(x) = numerator(x) / Z_H(x) on the coset g <w_D>                            prover.rs:191-226
//   plonk_split_kernel       t's coefficients off the coset (* g^-i), split in three and blinded             :228-247
//   plonk_linearise_kernel   r(X) plus the nu-combination of round 5, one pass over coefficient vectors      :324-359
#pragma once
#include "fp.hpp"
#include "mle_kernels.hpp"

namespace zk {

constexpr int GP_T = 256;                 // lanes per workgroup of the grand-product passes
constexpr int GP_E = 4;                   // rows per lane
constexpr int GP_ROWS = GP_T * GP_E;
// status words the prover reads back (zeroed per proof)
enum : int { PLONK_FLAG_GATE = 0, PLONK_FLAG_DENOM = 1, PLONK_FLAG_CLOSE = 2, PLONK_FLAG_QUOTIENT = 3, PLONK_FLAGS = 4 };

// a^(r - 2): one inversion per workgroup (255 squarings)
__device__ __noinline__ Fr fr_inverse(const Fr& a) {
    Fr acc = Fr::one();
    for (int i = 254; i >= 0; --i) {
        acc = acc * acc;
        uint32_t w = FrParams::p(i >> 5);
        if ((i >> 5) == 0) w = 0xffffffffu;               // r = .. fffffffe ffffffff 00000001: r - 2 borrows from the second word
        if ((i >> 5) == 1) w -= 1;
        if ((w >> (i & 31)) & 1) acc = acc * a;
    }
    return acc;
}

// out[i] = scale * base^i, i < count
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_powers_kernel(FrArg base_v, FrArg scale_v, size_t count, uint64_t* __restrict__ out) {
    const Fr base = fr_from_arg(base_v), scale = fr_from_arg(scale_v);
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t i = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; i < count; i += stride) {
        Fr acc = scale, sq = base;
        for (size_t e = i; e; e >>= 1) {
            if (e & 1) acc = acc * sq;
            sq = sq * sq;
        }
        store_fr(out, i, acc);
    }
}

// out[i] = a[i] * b[i] for i < n_src, zero for n_src <= i < n (the coset scaling in front of a transform of fewer than 2^12 points)
__device__ __forceinline__ void plonk_scale_pad_body(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t n_src, size_t n,
                                                     uint64_t* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t i = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; i < n; i += stride)
        store_fr(out, i, i < n_src ? load_fr(a, i) * load_fr(b, i) : Fr::zero());
}
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_scale_pad_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t n_src,
                                                                          size_t n, uint64_t* __restrict__ out) {
    plonk_scale_pad_body(a, b, n_src, n, out);
}

// p (n coefficients, room for n + k) += (b_0 + b_1 X + .. + b_{k-1} X^(k-1)) (X^n - 1), k <= 3 < n
// lane j < k adds its term b_j X^j (X^n - 1)
__device__ __forceinline__ void plonk_blind_body(uint64_t* __restrict__ p, size_t n, uint32_t j, const Fr& bj) {
    store_fr(p, j, load_fr(p, j) - bj);
    store_fr(p, n + j, bj);
}
struct PlonkBlindArg { uint64_t v[12]; };
static __global__ __launch_bounds__(64) void plonk_blind_kernel(uint64_t* __restrict__ p, size_t n, uint32_t k, PlonkBlindArg b) {
    const uint32_t j = threadIdx.x;
    if (j >= k) return;
    Fr bj;
#pragma unroll
    for (int i = 0; i < 4; ++i) { bj.l[2 * i] = (uint32_t)b.v[4 * j + i]; bj.l[2 * i + 1] = (uint32_t)(b.v[4 * j + i] >> 32); }
    plonk_blind_body(p, n, j, bj);
}

// ---- grand product ------------------------------------------------------------------------------------------------------------
// inclusive prefix products (pre) and inclusive suffix products (suf) of the GP_T values v_t, both left in LDS
__device__ __forceinline__ void gp_scan_both(const Fr& v, Fr* pre, Fr* suf) {
    const uint32_t t = threadIdx.x;
    Fr p = v, s = v;
    pre[t] = p; suf[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)GP_T; d <<= 1) {
        Fr pv = Fr::one(), sv = Fr::one();
        if (t >= d) pv = pre[t - d];
        if (t + d < (uint32_t)GP_T) sv = suf[t + d];
        __syncthreads();
        p = p * pv; s = s * sv;
        pre[t] = p; suf[t] = s;
        __syncthreads();
    }
}

struct PlonkCols { const uint64_t* q[8]; };     // q_m, q_l, q_r, q_o, q_c, sigma_1, sigma_2, sigma_3 (the order of VerifierPreprocessedInput::vpi)

// Pass 1: per row the gate check and f_i = num_i / den_i (prover.rs:136-152); per workgroup the product of its f_i.
__device__ __forceinline__ void plonk_gp_ratio_body(const uint64_t* __restrict__ wa, const uint64_t* __restrict__ wb, const uint64_t* __restrict__ wc,
                                                    const uint64_t* __restrict__ pub, const PlonkCols& cols, const uint64_t* __restrict__ omega_pow,
                                                    size_t n, const Fr& beta, const Fr& gamma, uint64_t* __restrict__ f_out,
                                                    uint64_t* __restrict__ block_prod, int* __restrict__ flags) {
    __shared__ Fr pre[GP_T], suf[GP_T];
    __shared__ Fr inv_total;
    const uint32_t t = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * GP_T + t) * GP_E;
    Fr num[GP_E], den[GP_E];
#pragma unroll
    for (int j = 0; j < GP_E; ++j) {
        const size_t i = base + j;
        num[j] = Fr::one(); den[j] = Fr::one();
        if (i >= n) continue;
        const Fr a = load_fr(wa, i), b = load_fr(wb, i), c = load_fr(wc, i);
        const Fr gate = a * b * load_fr(cols.q[0], i) + a * load_fr(cols.q[1], i) + b * load_fr(cols.q[2], i) + c * load_fr(cols.q[3], i) +
                        load_fr(pub, i) + load_fr(cols.q[4], i);
        if (!gate.is_zero()) flags[PLONK_FLAG_GATE] = 1;
        const Fr bw = beta * load_fr(omega_pow, i);
        const Fr ag = a + gamma, bg = b + gamma, cg = c + gamma;
        num[j] = (ag + bw) * (bg + bw + bw) * (cg + bw + bw + bw);
        Fr d = (ag + beta * load_fr(cols.q[5], i)) * (bg + beta * load_fr(cols.q[6], i)) * (cg + beta * load_fr(cols.q[7], i));
        if (d.is_zero()) { flags[PLONK_FLAG_DENOM] = 1; d = Fr::one(); }
        den[j] = d;
    }
    Fr part[GP_E];                                   // part[j] = den_0 .. den_{j-1}
    Fr p = Fr::one();
#pragma unroll
    for (int j = 0; j < GP_E; ++j) { part[j] = p; p = p * den[j]; }
    gp_scan_both(p, pre, suf);
    if (t == 0) inv_total = fr_inverse(pre[GP_T - 1]);
    __syncthreads();
    Fr run = inv_total;                              // 1 / (this lane's product): the total's inverse times everybody else's
    if (t > 0) run = run * pre[t - 1];
    if (t + 1 < (uint32_t)GP_T) run = run * suf[t + 1];
    Fr f[GP_E];
#pragma unroll
    for (int j = GP_E - 1; j >= 0; --j) {
        f[j] = num[j] * (run * part[j]);
        run = run * den[j];
    }
    Fr q = Fr::one();
#pragma unroll
    for (int j = 0; j < GP_E; ++j) {
        if (base + j < n) store_fr(f_out, base + j, f[j]);
        q = q * f[j];
    }
    __syncthreads();
    pre[t] = q;
    __syncthreads();
    for (uint32_t d = GP_T / 2; d >= 1; d >>= 1) {
        if (t < d) pre[t] = pre[t] * pre[t + d];
        __syncthreads();
    }
    if (t == 0) store_fr(block_prod, blockIdx.x, pre[0]);
}
static __global__ __launch_bounds__(GP_T) void plonk_gp_ratio_kernel(const uint64_t* __restrict__ wa, const uint64_t* __restrict__ wb,
                                                                   const uint64_t* __restrict__ wc, const uint64_t* __restrict__ pub,
                                                                   PlonkCols cols, const uint64_t* __restrict__ omega_pow, size_t n,
                                                                   FrArg beta_v, FrArg gamma_v, uint64_t* __restrict__ f_out,
                                                                   uint64_t* __restrict__ block_prod, int* __restrict__ flags) {
    plonk_gp_ratio_body(wa, wb, wc, pub, cols, omega_pow, n, fr_from_arg(beta_v), fr_from_arg(gamma_v), f_out, block_prod, flags);
}

// Pass 2, one workgroup: block_excl[b] = product of block_prod[b'] over b' < b
__device__ __forceinline__ void plonk_gp_top_body(const uint64_t* __restrict__ block_prod, uint32_t n_blocks, uint64_t* __restrict__ block_excl) {
    __shared__ Fr lds[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + 1023) / 1024;
    const uint32_t lo = min(t * per, n_blocks), hi = min(lo + per, n_blocks);
    Fr g = Fr::one();
    for (uint32_t b = lo; b < hi; ++b) g = g * load_fr(block_prod, b);
    Fr p = g;
    lds[t] = p;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        Fr v = Fr::one();
        if (t >= d) v = lds[t - d];
        __syncthreads();
        p = p * v;
        lds[t] = p;
        __syncthreads();
    }
    Fr y = t ? lds[t - 1] : Fr::one();
    for (uint32_t b = lo; b < hi; ++b) {
        store_fr(block_excl, b, y);
        y = y * load_fr(block_prod, b);
    }
}
static __global__ __launch_bounds__(1024) void plonk_gp_top_kernel(const uint64_t* __restrict__ block_prod, uint32_t n_blocks,
                                                                  uint64_t* __restrict__ block_excl) {
    plonk_gp_top_body(block_prod, n_blocks, block_excl);
}

// Pass 3: acc_i = product of f_k over k < i (acc_0 = 1); the last row checks that the accumulator closes: acc_{n-1} f_{n-1} = 1
__device__ __forceinline__ void plonk_gp_apply_body(const uint64_t* __restrict__ f_in, const uint64_t* __restrict__ block_excl, size_t n,
                                                    uint64_t* __restrict__ acc, int* __restrict__ flags) {
    __shared__ Fr pre[GP_T];
    const uint32_t t = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * GP_T + t) * GP_E;
    Fr f[GP_E];
    Fr q = Fr::one();
#pragma unroll
    for (int j = 0; j < GP_E; ++j) {
        f[j] = base + j < n ? load_fr(f_in, base + j) : Fr::one();
        q = q * f[j];
    }
    Fr p = q;
    pre[t] = p;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)GP_T; d <<= 1) {
        Fr v = Fr::one();
        if (t >= d) v = pre[t - d];
        __syncthreads();
        p = p * v;
        pre[t] = p;
        __syncthreads();
    }
    Fr y = load_fr(block_excl, blockIdx.x);
    if (t) y = y * pre[t - 1];
#pragma unroll
    for (int j = 0; j < GP_E; ++j) {
        const size_t i = base + j;
        if (i < n) store_fr(acc, i, y);
        y = y * f[j];
        if (i == n - 1 && !(y == Fr::one())) flags[PLONK_FLAG_CLOSE] = 1;
    }
}
static __global__ __launch_bounds__(GP_T) void plonk_gp_apply_kernel(const uint64_t* __restrict__ f_in, const uint64_t* __restrict__ block_excl,
                                                                   size_t n, uint64_t* __restrict__ acc, int* __restrict__ flags) {
    plonk_gp_apply_body(f_in, block_excl, n, acc, flags);
}

// ---- quotient -----------------------------------------------------------------------------------------------------------------
// One pass over the D points x_j = g w_D^j.  ev: a_s, b_s, c_s, z, PI (D each); pre: q_m, q_l, q_r, q_o, q_c, sigma_1..3, L_1, x (D each).
// z(w x_j) is z's own evaluation `rot` = D / n places on.  Z_H takes D / n values on the coset: zh_inv[j mod (D / n)].
__device__ __forceinline__ void plonk_quotient_body(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ pre, size_t D, const Fr& beta,
                                                    const Fr& gamma, const Fr& alpha, const Fr& alpha2, const FrArg (&zh_inv)[8], uint32_t rot,
                                                    uint64_t* __restrict__ t_out) {
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t j = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; j < D; j += stride) {
        const Fr a = load_fr(ev, j), b = load_fr(ev + 4 * D, j), c = load_fr(ev + 8 * D, j);
        const Fr z = load_fr(ev + 12 * D, j), zw = load_fr(ev + 12 * D, (j + rot) & (D - 1));
        Fr gate = a * b * load_fr(pre, j) + a * load_fr(pre + 4 * D, j) + b * load_fr(pre + 8 * D, j) + c * load_fr(pre + 12 * D, j) +
                  load_fr(ev + 16 * D, j) + load_fr(pre + 16 * D, j);
        const Fr ag = a + gamma, bg = b + gamma, cg = c + gamma;
        const Fr bx = beta * load_fr(pre + 36 * D, j);
        const Fr p1 = (ag + bx) * (bg + bx + bx) * (cg + bx + bx + bx) * z;
        const Fr p2 = (ag + beta * load_fr(pre + 20 * D, j)) * (bg + beta * load_fr(pre + 24 * D, j)) * (cg + beta * load_fr(pre + 28 * D, j)) * zw;
        const Fr l = (z - Fr::one()) * load_fr(pre + 32 * D, j);
        const Fr num = gate + alpha * (p1 - p2) + alpha2 * l;
        store_fr(t_out, j, num * fr_from_arg(zh_inv[j & (rot - 1)]));
    }
}
struct PlonkQuotArg { FrArg beta, gamma, alpha, alpha2, zh_inv[8]; uint32_t rot; };
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_quotient_kernel(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ pre, size_t D,
                                                                        PlonkQuotArg k, uint64_t* __restrict__ t_out) {
    plonk_quotient_body(ev, pre, D, fr_from_arg(k.beta), fr_from_arg(k.gamma), fr_from_arg(k.alpha), fr_from_arg(k.alpha2), k.zh_inv, k.rot, t_out);
}

// t's coefficients as the inverse transform left them (scaled by g^i): unscale, split at n and 2n, blind (prover.rs:228-247).
// tl, tm: n + 1 coefficients; th: n + 6.  A coefficient at or beyond 3n + 6 that is not zero means Z_H did not divide the numerator.
__device__ __forceinline__ void plonk_split_body(const uint64_t* __restrict__ t, const uint64_t* __restrict__ ginv_pow, size_t n, size_t D, const Fr& b10,
                                                 const Fr& b11, uint64_t* __restrict__ tl, uint64_t* __restrict__ tm, uint64_t* __restrict__ th,
                                                 int* __restrict__ flags) {
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t i = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; i < D; i += stride) {
        Fr v = load_fr(t, i);
        if (i >= 3 * n + 6) {
            if (!v.is_zero()) flags[PLONK_FLAG_QUOTIENT] = 1;
            continue;
        }
        v = v * load_fr(ginv_pow, i);
        if (i < n) {
            store_fr(tl, i, v);
            if (i == 0) { store_fr(tl, n, b10); store_fr(tm, n, b11); }
        } else if (i < 2 * n) {
            store_fr(tm, i - n, i == n ? v - b10 : v);
        } else {
            store_fr(th, i - 2 * n, i == 2 * n ? v - b11 : v);
        }
    }
}
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_split_kernel(const uint64_t* __restrict__ t, const uint64_t* __restrict__ ginv_pow, size_t n,
                                                                     size_t D, FrArg b10_v, FrArg b11_v, uint64_t* __restrict__ tl,
                                                                     uint64_t* __restrict__ tm, uint64_t* __restrict__ th, int* __restrict__ flags) {
    plonk_split_body(t, ginv_pow, n, D, fr_from_arg(b10_v), fr_from_arg(b11_v), tl, tm, th, flags);
}

// ---- linearisation --------------------------------------------------------------------------------------------------------------
// out[i] = sum_k s_k p_k[i] (+ c0 at i = 0), i < len: the numerator of W_zeta (prover.rs:324-359) with every scalar of round 5 folded
// into the 15 weights on the host.  Every vector is zero-padded to len.
// The scalars are read inside the loop, so the body takes their source: c0(), weight(q) and poly(q), the vector of term q.
constexpr int PLONK_LIN_TERMS = 15;
template <class Src>
__device__ __forceinline__ void plonk_linearise_body(const Src& src, size_t len, uint64_t* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t i = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; i < len; i += stride) {
        Fr acc = i == 0 ? src.c0() : Fr::zero();
#pragma unroll
        for (int q = 0; q < PLONK_LIN_TERMS; ++q) acc = acc + src.weight(q) * load_fr(src.poly(q), i);
        store_fr(out, i, acc);
    }
}
struct PlonkLinArg { const uint64_t* p[PLONK_LIN_TERMS]; FrArg s[PLONK_LIN_TERMS]; FrArg c0; };
// The single kernel converts its fifteen weights ONCE, in front of the loop, and the source hands out those copies: the weights then
// stay in registers across the loop (137 VGPRs), as they did before the body was shared.  Reading k.s[q] inside weight() compiles to
// 76 VGPRs and a reload of the weights per element, which measured 6 us slower per launch at n = 2^12 (profiles/plonk_bodies/NOTES.md).
struct PlonkLinArgSrc {
    const PlonkLinArg& k;
    const Fr* w;
    __device__ __forceinline__ Fr c0() const { return fr_from_arg(k.c0); }
    __device__ __forceinline__ Fr weight(int q) const { return w[q]; }
    __device__ __forceinline__ const uint64_t* poly(int q) const { return k.p[q]; }
};
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_linearise_kernel(PlonkLinArg k, size_t len, uint64_t* __restrict__ out) {
    Fr w[PLONK_LIN_TERMS];
#pragma unroll
    for (int q = 0; q < PLONK_LIN_TERMS; ++q) w[q] = fr_from_arg(k.s[q]);
    plonk_linearise_body(PlonkLinArgSrc{k, w}, len, out);
}

}  // namespace zk
