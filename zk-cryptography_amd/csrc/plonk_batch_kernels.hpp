// plonk_batch_kernels.hpp -- the passes of plonk_kernels.hpp (and the Horner scan of mle_kernels.hpp) for a CHUNK of proofs of one
// circuit (zkhip_plonk_prove_batch), for gfx950.
//
// Every proof of a chunk owns one work area of the same layout; the areas lie `ws` ELEMENTS (32 bytes each) apart, so a kernel takes
// the address a buffer has in proof 0's area and the proof index -- the grid's LAST used dimension -- moves it by b * ws.  What differs
// from proof to proof and is a kernel argument in the single prover -- beta, gamma, alpha, alpha^2, the eleven blinding scalars, zeta,
// w zeta, the fifteen linearisation weights and c0 -- is a row of PB_SLOTS field elements per proof in device memory (`par`), uploaded
// once per round; the flags are PLONK_FLAGS ints per proof, `fs` INTS apart.  The bodies are those of the single kernels, written
// beside them and not shared with them: the single prover's kernels compile to what they did (profiles/plonk_batch/NOTES.md).
// No workgroup waits on another; a launch's size depends on the proofs of a chunk, the number of launches does not.
#pragma once
#include "plonk_kernels.hpp"

namespace zk {

// a proof's row of `par`
enum : uint32_t { PB_BETA = 0, PB_GAMMA = 1, PB_ALPHA = 2, PB_ALPHA2 = 3, PB_BLIND = 4 /* 11 */, PB_ZETA = 15, PB_ZETA_W = 16,
                  PB_LIN = 17 /* PLONK_LIN_TERMS */, PB_C0 = 32, PB_SLOTS = 40 };
static_assert(PB_LIN + PLONK_LIN_TERMS == PB_C0, "the weights end where c0 begins");

__device__ __forceinline__ Fr pb_par(const uint64_t* __restrict__ par, uint32_t b, uint32_t slot) { return load_fr(par, (size_t)b * PB_SLOTS + slot); }

// The wire and public columns arrive as separate device pointers, four per proof (a, b, c, public): column j of proof b goes to
// dst + 4 (b ws + j n).  grid (x, 4, proofs)
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_gather_kernel(const uint64_t* const* __restrict__ cols, size_t n, uint64_t* __restrict__ dst,
                                                                            size_t ws) {
    const uint32_t j = blockIdx.y, b = blockIdx.z;
    const uint64_t* __restrict__ src = cols[4 * (size_t)b + j];
    uint64_t* __restrict__ out = dst + 4 * ((size_t)b * ws + (size_t)j * n);
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t i = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; i < n; i += stride) store_fr(out, i, load_fr(src, i));
}

// plonk_blind_kernel for m <= 3 polynomials of every proof: coefficient j of polynomial q is the blinding scalar slot[q][j].
// grid (m, proofs)
struct PlonkBlindBatchArg { uint64_t* p[3]; uint8_t slot[3][3]; };
static __global__ __launch_bounds__(64) void plonk_batch_blind_kernel(PlonkBlindBatchArg a, size_t n, uint32_t k, const uint64_t* __restrict__ par, size_t ws) {
    const uint32_t j = threadIdx.x, q = blockIdx.x, b = blockIdx.y;
    if (j >= k) return;
    uint64_t* __restrict__ p = a.p[q] + 4 * (size_t)b * ws;
    const Fr bj = pb_par(par, b, PB_BLIND + a.slot[q][j]);
    store_fr(p, j, load_fr(p, j) - bj);
    store_fr(p, n + j, bj);
}

// ---- grand product: plonk_gp_ratio / _top / _apply with the proof as grid.y ---------------------------------------------------------
static __global__ __launch_bounds__(GP_T) void plonk_batch_gp_ratio_kernel(const uint64_t* __restrict__ wa, const uint64_t* __restrict__ wb,
                                                                         const uint64_t* __restrict__ wc, const uint64_t* __restrict__ pub,
                                                                         PlonkCols cols, const uint64_t* __restrict__ omega_pow, size_t n,
                                                                         const uint64_t* __restrict__ par, uint64_t* __restrict__ f_out,
                                                                         uint64_t* __restrict__ block_prod, int* __restrict__ flags, size_t ws, size_t fs) {
    __shared__ Fr pre[GP_T], suf[GP_T];
    __shared__ Fr inv_total;
    const uint32_t pb = blockIdx.y;
    const size_t shift = 4 * (size_t)pb * ws;
    wa += shift; wb += shift; wc += shift; pub += shift; f_out += shift; block_prod += shift; flags += (size_t)pb * fs;
    const Fr beta = pb_par(par, pb, PB_BETA), gamma = pb_par(par, pb, PB_GAMMA);
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
    Fr part[GP_E];
    Fr p = Fr::one();
#pragma unroll
    for (int j = 0; j < GP_E; ++j) { part[j] = p; p = p * den[j]; }
    gp_scan_both(p, pre, suf);
    if (t == 0) inv_total = fr_inverse(pre[GP_T - 1]);
    __syncthreads();
    Fr run = inv_total;
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

// grid (proofs)
static __global__ __launch_bounds__(1024) void plonk_batch_gp_top_kernel(const uint64_t* __restrict__ block_prod, uint32_t n_blocks,
                                                                        uint64_t* __restrict__ block_excl, size_t ws) {
    __shared__ Fr lds[1024];
    block_prod += 4 * (size_t)blockIdx.x * ws; block_excl += 4 * (size_t)blockIdx.x * ws;
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

// grid (workgroups of a proof, proofs)
static __global__ __launch_bounds__(GP_T) void plonk_batch_gp_apply_kernel(const uint64_t* __restrict__ f_in, const uint64_t* __restrict__ block_excl,
                                                                         size_t n, uint64_t* __restrict__ acc, int* __restrict__ flags, size_t ws, size_t fs) {
    __shared__ Fr pre[GP_T];
    const size_t shift = 4 * (size_t)blockIdx.y * ws;
    f_in += shift; block_excl += shift; acc += shift; flags += (size_t)blockIdx.y * fs;
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

// ---- quotient -----------------------------------------------------------------------------------------------------------------------
// plonk_scale_pad_kernel for the five coset inputs of every proof: row j of proof b, D elements at dst + 4 (b ws + j D), is
// src[j][i] * mul[i] for i < len[j] and zero beyond.  grid (x, 5, proofs)
constexpr int PB_COSET_ROWS = 5;
struct PlonkPadBatchArg { const uint64_t* src[PB_COSET_ROWS]; uint32_t len[PB_COSET_ROWS]; };
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_scale_pad_kernel(PlonkPadBatchArg a, const uint64_t* __restrict__ mul, size_t D,
                                                                               uint64_t* __restrict__ dst, size_t ws) {
    const uint32_t j = blockIdx.y, b = blockIdx.z;
    const uint64_t* __restrict__ src = a.src[j] + 4 * (size_t)b * ws;
    uint64_t* __restrict__ out = dst + 4 * ((size_t)b * ws + (size_t)j * D);
    const size_t n_src = a.len[j];
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t i = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; i < D; i += stride)
        store_fr(out, i, i < n_src ? load_fr(src, i) * load_fr(mul, i) : Fr::zero());
}

// plonk_quotient_kernel; the ten coset columns `pre` are the key's, the same for every proof.  grid (x, proofs)
struct PlonkQuotBatchArg { FrArg zh_inv[8]; uint32_t rot; };
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_quotient_kernel(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ pre, size_t D,
                                                                              PlonkQuotBatchArg k, const uint64_t* __restrict__ par,
                                                                              uint64_t* __restrict__ t_out, size_t ws) {
    const uint32_t pb = blockIdx.y;
    ev += 4 * (size_t)pb * ws; t_out += 4 * (size_t)pb * ws;
    const Fr beta = pb_par(par, pb, PB_BETA), gamma = pb_par(par, pb, PB_GAMMA), alpha = pb_par(par, pb, PB_ALPHA), alpha2 = pb_par(par, pb, PB_ALPHA2);
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t j = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; j < D; j += stride) {
        const Fr a = load_fr(ev, j), b = load_fr(ev + 4 * D, j), c = load_fr(ev + 8 * D, j);
        const Fr z = load_fr(ev + 12 * D, j), zw = load_fr(ev + 12 * D, (j + k.rot) & (D - 1));
        Fr gate = a * b * load_fr(pre, j) + a * load_fr(pre + 4 * D, j) + b * load_fr(pre + 8 * D, j) + c * load_fr(pre + 12 * D, j) +
                  load_fr(ev + 16 * D, j) + load_fr(pre + 16 * D, j);
        const Fr ag = a + gamma, bg = b + gamma, cg = c + gamma;
        const Fr bx = beta * load_fr(pre + 36 * D, j);
        const Fr p1 = (ag + bx) * (bg + bx + bx) * (cg + bx + bx + bx) * z;
        const Fr p2 = (ag + beta * load_fr(pre + 20 * D, j)) * (bg + beta * load_fr(pre + 24 * D, j)) * (cg + beta * load_fr(pre + 28 * D, j)) * zw;
        const Fr l = (z - Fr::one()) * load_fr(pre + 32 * D, j);
        const Fr num = gate + alpha * (p1 - p2) + alpha2 * l;
        store_fr(t_out, j, num * fr_from_arg(k.zh_inv[j & (k.rot - 1)]));
    }
}

// plonk_split_kernel.  grid (x, proofs)
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_split_kernel(const uint64_t* __restrict__ t, const uint64_t* __restrict__ ginv_pow, size_t n,
                                                                           size_t D, const uint64_t* __restrict__ par, uint64_t* __restrict__ tl,
                                                                           uint64_t* __restrict__ tm, uint64_t* __restrict__ th, int* __restrict__ flags,
                                                                           size_t ws, size_t fs) {
    const uint32_t pb = blockIdx.y;
    const size_t shift = 4 * (size_t)pb * ws;
    t += shift; tl += shift; tm += shift; th += shift; flags += (size_t)pb * fs;
    const Fr b10 = pb_par(par, pb, PB_BLIND + 9), b11 = pb_par(par, pb, PB_BLIND + 10);
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

// ---- linearisation ------------------------------------------------------------------------------------------------------------------
// plonk_linearise_kernel: term q reads p[q], moved by the proof's offset when bit q of `own` is set (the proof's own polynomials; the
// others are the key's), with the weight par[PB_LIN + q]; c0 = par[PB_C0].  grid (x, proofs)
struct PlonkLinBatchArg { const uint64_t* p[PLONK_LIN_TERMS]; uint32_t own; };
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_linearise_kernel(PlonkLinBatchArg k, size_t len, const uint64_t* __restrict__ par,
                                                                               uint64_t* __restrict__ out, size_t ws) {
    const uint32_t pb = blockIdx.y;
    const size_t shift = 4 * (size_t)pb * ws;
    out += shift;
    const size_t stride = (size_t)gridDim.x * MLE_BLOCK;
    for (size_t i = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x; i < len; i += stride) {
        Fr acc = i == 0 ? pb_par(par, pb, PB_C0) : Fr::zero();
#pragma unroll
        for (int q = 0; q < PLONK_LIN_TERMS; ++q) acc = acc + pb_par(par, pb, PB_LIN + q) * load_fr(k.p[q] + (((k.own >> q) & 1u) ? shift : 0), i);
        store_fr(out, i, acc);
    }
}

// ---- Horner: evaluations and divisions by a linear factor --------------------------------------------------------------------------
// horner_scan_kernel / horner_top_kernel of mle_kernels.hpp over a list of up to PB_JOBS (polynomial, length, point) jobs per proof:
// all seven evaluations of round 4 in one scan and one top launch, both divisions of round 5 in scan, top, apply.  Job j reads
// coeffs[j] (moved by the proof's offset when bit j of `own` is set) at the point par[zslot[j]]; its workgroup values and carries are
// vals / carries + 4 (b ws + j vstride + workgroup); the value p(z) goes to evals + 4 (b ws + j), the quotient (APPLY) to quotient[j]
// of the proof's area.  A job's workgroups beyond ceil(len / (HS_T HS_L)) leave at once.  grid (workgroups of the longest job, jobs, proofs)
constexpr int PB_JOBS = 7;
struct HornerBatchArg {
    const uint64_t* coeffs[PB_JOBS];
    uint64_t* quotient[PB_JOBS];
    uint32_t len[PB_JOBS];
    uint8_t zslot[PB_JOBS];
    uint32_t own, vstride;
};
template <bool APPLY>
static __global__ __launch_bounds__(HS_T) void horner_batch_scan_kernel(HornerBatchArg a, const uint64_t* __restrict__ par, uint64_t* __restrict__ vals,
                                                                      const uint64_t* __restrict__ carries, uint64_t* __restrict__ evals, size_t ws) {
    __shared__ Fr a_lds[HS_T];
    const uint32_t job = blockIdx.y, pb = blockIdx.z;
    const size_t n = a.len[job];
    if ((size_t)blockIdx.x * HS_T * HS_L >= n) return;                  // the whole workgroup: nobody is left at a barrier
    const size_t shift = 4 * (size_t)pb * ws;
    const uint64_t* __restrict__ coeffs = a.coeffs[job] + (((a.own >> job) & 1u) ? shift : 0);
    const size_t v_at = (size_t)pb * ws + (size_t)job * a.vstride + blockIdx.x;
    const Fr z = pb_par(par, pb, a.zslot[job]);
    const uint32_t t = threadIdx.x;
    const size_t s = ((size_t)blockIdx.x * HS_T + t) * HS_L;
    Fr c[HS_L];
#pragma unroll
    for (int j = 0; j < HS_L; ++j) c[j] = (s + j < n) ? load_fr(coeffs, s + j) : Fr::zero();
    Fr h = c[HS_L - 1];
#pragma unroll
    for (int j = HS_L - 2; j >= 0; --j) h = c[j] + z * h;
    Fr rp = z;
#pragma unroll
    for (int q = 1; q < HS_L; q <<= 1) rp = rp * rp;
    Fr carry_in = Fr::zero();
    if (APPLY) {
        carry_in = load_fr(carries, v_at);
        if (t == HS_T - 1) h = h + rp * carry_in;
    }
    a_lds[t] = h;
    __syncthreads();
    for (uint32_t d = 1; d < (uint32_t)HS_T; d <<= 1) {
        Fr v = Fr::zero();
        const bool has = t + d < (uint32_t)HS_T;
        if (has) v = a_lds[t + d];
        __syncthreads();
        if (has) { h = h + rp * v; a_lds[t] = h; }
        __syncthreads();
        rp = rp * rp;
    }
    if (!APPLY) {
        if (t == 0) store_fr(vals, v_at, h);
        return;
    }
    uint64_t* __restrict__ quotient = a.quotient[job] + shift;
    Fr v = (t == HS_T - 1) ? carry_in : a_lds[t + 1];
#pragma unroll
    for (int j = HS_L - 1; j >= 0; --j) {
        v = c[j] + z * v;
        const size_t i = s + j;
        if (i == 0) store_fr(evals, (size_t)pb * ws + job, v);
        else if (i < n) store_fr(quotient, i - 1, v);
    }
}
// grid (jobs, proofs); evals == nullptr: the carries alone
static __global__ __launch_bounds__(1024) void horner_batch_top_kernel(HornerBatchArg a, const uint64_t* __restrict__ par, const uint64_t* __restrict__ vals,
                                                                     uint64_t* __restrict__ carries, uint64_t* __restrict__ evals, size_t ws) {
    __shared__ Fr a_lds[1024];
    const uint32_t job = blockIdx.x, pb = blockIdx.y;
    const uint32_t n_blocks = (uint32_t)(((size_t)a.len[job] + (size_t)HS_T * HS_L - 1) / ((size_t)HS_T * HS_L));
    const size_t v_at = (size_t)pb * ws + (size_t)job * a.vstride;
    const uint64_t* __restrict__ block_vals = vals + 4 * v_at;
    uint64_t* __restrict__ out = carries + 4 * v_at;
    const uint32_t t = threadIdx.x;
    Fr R = pb_par(par, pb, a.zslot[job]);
    for (int q = 1; q < HS_T * HS_L; q <<= 1) R = R * R;
    const uint32_t per = (n_blocks + 1023) / 1024;
    const uint32_t lo = min(t * per, n_blocks), hi = min(lo + per, n_blocks);
    Fr g = Fr::zero();
    for (uint32_t b = hi; b-- > lo;) g = load_fr(block_vals, b) + R * g;
    Fr rp = Fr::one();
    for (uint32_t q = 0; q < per; ++q) rp = rp * R;
    a_lds[t] = g;
    __syncthreads();
    Fr h = g;
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        Fr v = Fr::zero();
        const bool has = t + d < 1024;
        if (has) v = a_lds[t + d];
        __syncthreads();
        if (has) { h = h + rp * v; a_lds[t] = h; }
        __syncthreads();
        rp = rp * rp;
    }
    Fr y = (t == 1023) ? Fr::zero() : a_lds[t + 1];
    for (uint32_t b = hi; b-- > lo;) {
        store_fr(out, b, y);
        y = load_fr(block_vals, b) + R * y;
    }
    if (t == 0 && evals) store_fr(evals, (size_t)pb * ws + job, y);
}

}  // namespace zk
