// plonk_batch_kernels.hpp -- the passes of plonk_kernels.hpp (and the Horner scan of mle_kernels.hpp) for a CHUNK of proofs of one
// circuit (zkhip_plonk_prove_batch), for gfx950.
//
// Every proof of a chunk owns one work area of the same layout; the areas lie `ws` ELEMENTS (32 bytes each) apart, so a kernel takes
// the address a buffer has in proof 0's area and the proof index -- the grid's LAST used dimension -- moves it by b * ws.  What differs
// from proof to proof and is a kernel argument in the single prover -- beta, gamma, alpha, alpha^2, the eleven blinding scalars, zeta,
// w zeta, the fifteen linearisation weights and c0 -- is a row of PB_SLOTS field elements per proof in device memory (`par`), uploaded
// once per round; the flags are PLONK_FLAGS ints per proof, `fs` INTS apart.
//
// No field arithmetic is written here.  Every kernel but the gather is a wrapper: it moves the pointers to its proof's area, reads the
// proof's scalars from `par` and calls the `.._body` that the single prover's kernel of the same pass calls (plonk_kernels.hpp,
// mle_kernels.hpp), so a formula exists once.  The bodies index rows by blockIdx.x alone, which is why the proof (and the job, and the
// coset row) sit on the grid's other dimensions.
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
    plonk_blind_body(a.p[q] + 4 * (size_t)b * ws, n, j, pb_par(par, b, PB_BLIND + a.slot[q][j]));
}

// ---- grand product: plonk_gp_ratio / _top / _apply with the proof as grid.y ---------------------------------------------------------
static __global__ __launch_bounds__(GP_T) void plonk_batch_gp_ratio_kernel(const uint64_t* __restrict__ wa, const uint64_t* __restrict__ wb,
                                                                         const uint64_t* __restrict__ wc, const uint64_t* __restrict__ pub,
                                                                         PlonkCols cols, const uint64_t* __restrict__ omega_pow, size_t n,
                                                                         const uint64_t* __restrict__ par, uint64_t* __restrict__ f_out,
                                                                         uint64_t* __restrict__ block_prod, int* __restrict__ flags, size_t ws, size_t fs) {
    const uint32_t pb = blockIdx.y;
    const size_t shift = 4 * (size_t)pb * ws;
    plonk_gp_ratio_body(wa + shift, wb + shift, wc + shift, pub + shift, cols, omega_pow, n, pb_par(par, pb, PB_BETA), pb_par(par, pb, PB_GAMMA),
                        f_out + shift, block_prod + shift, flags + (size_t)pb * fs);
}

// grid (proofs)
static __global__ __launch_bounds__(1024) void plonk_batch_gp_top_kernel(const uint64_t* __restrict__ block_prod, uint32_t n_blocks,
                                                                        uint64_t* __restrict__ block_excl, size_t ws) {
    const size_t shift = 4 * (size_t)blockIdx.x * ws;
    plonk_gp_top_body(block_prod + shift, n_blocks, block_excl + shift);
}

// grid (workgroups of a proof, proofs)
static __global__ __launch_bounds__(GP_T) void plonk_batch_gp_apply_kernel(const uint64_t* __restrict__ f_in, const uint64_t* __restrict__ block_excl,
                                                                         size_t n, uint64_t* __restrict__ acc, int* __restrict__ flags, size_t ws, size_t fs) {
    const size_t shift = 4 * (size_t)blockIdx.y * ws;
    plonk_gp_apply_body(f_in + shift, block_excl + shift, n, acc + shift, flags + (size_t)blockIdx.y * fs);
}

// ---- quotient -----------------------------------------------------------------------------------------------------------------------
// plonk_scale_pad_kernel for the five coset inputs of every proof: row j of proof b, D elements at dst + 4 (b ws + j D), is
// src[j][i] * mul[i] for i < len[j] and zero beyond.  grid (x, 5, proofs)
constexpr int PB_COSET_ROWS = 5;
struct PlonkPadBatchArg { const uint64_t* src[PB_COSET_ROWS]; uint32_t len[PB_COSET_ROWS]; };
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_scale_pad_kernel(PlonkPadBatchArg a, const uint64_t* __restrict__ mul, size_t D,
                                                                               uint64_t* __restrict__ dst, size_t ws) {
    const uint32_t j = blockIdx.y, b = blockIdx.z;
    plonk_scale_pad_body(a.src[j] + 4 * (size_t)b * ws, mul, a.len[j], D, dst + 4 * ((size_t)b * ws + (size_t)j * D));
}

// plonk_quotient_kernel; the ten coset columns `pre` are the key's, the same for every proof.  grid (x, proofs)
struct PlonkQuotBatchArg { FrArg zh_inv[8]; uint32_t rot; };
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_quotient_kernel(const uint64_t* __restrict__ ev, const uint64_t* __restrict__ pre, size_t D,
                                                                              PlonkQuotBatchArg k, const uint64_t* __restrict__ par,
                                                                              uint64_t* __restrict__ t_out, size_t ws) {
    const uint32_t pb = blockIdx.y;
    const size_t shift = 4 * (size_t)pb * ws;
    plonk_quotient_body(ev + shift, pre, D, pb_par(par, pb, PB_BETA), pb_par(par, pb, PB_GAMMA), pb_par(par, pb, PB_ALPHA), pb_par(par, pb, PB_ALPHA2),
                        k.zh_inv, k.rot, t_out + shift);
}

// plonk_split_kernel.  grid (x, proofs)
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_split_kernel(const uint64_t* __restrict__ t, const uint64_t* __restrict__ ginv_pow, size_t n,
                                                                           size_t D, const uint64_t* __restrict__ par, uint64_t* __restrict__ tl,
                                                                           uint64_t* __restrict__ tm, uint64_t* __restrict__ th, int* __restrict__ flags,
                                                                           size_t ws, size_t fs) {
    const uint32_t pb = blockIdx.y;
    const size_t shift = 4 * (size_t)pb * ws;
    plonk_split_body(t + shift, ginv_pow, n, D, pb_par(par, pb, PB_BLIND + 9), pb_par(par, pb, PB_BLIND + 10), tl + shift, tm + shift, th + shift,
                     flags + (size_t)pb * fs);
}

// ---- linearisation ------------------------------------------------------------------------------------------------------------------
// plonk_linearise_kernel: term q reads p[q], moved by the proof's offset when bit q of `own` is set (the proof's own polynomials; the
// others are the key's), with the weight par[PB_LIN + q]; c0 = par[PB_C0].  grid (x, proofs)
struct PlonkLinBatchArg { const uint64_t* p[PLONK_LIN_TERMS]; uint32_t own; };
struct PlonkLinBatchSrc {
    const PlonkLinBatchArg& k;
    const uint64_t* __restrict__ par;
    uint32_t pb;
    size_t shift;
    __device__ __forceinline__ Fr c0() const { return pb_par(par, pb, PB_C0); }
    __device__ __forceinline__ Fr weight(int q) const { return pb_par(par, pb, PB_LIN + q); }
    __device__ __forceinline__ const uint64_t* poly(int q) const { return k.p[q] + (((k.own >> q) & 1u) ? shift : 0); }
};
static __global__ __launch_bounds__(MLE_BLOCK) void plonk_batch_linearise_kernel(PlonkLinBatchArg k, size_t len, const uint64_t* __restrict__ par,
                                                                               uint64_t* __restrict__ out, size_t ws) {
    const uint32_t pb = blockIdx.y;
    const size_t shift = 4 * (size_t)pb * ws;
    plonk_linearise_body(PlonkLinBatchSrc{k, par, pb, shift}, len, out + shift);
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
    const uint32_t job = blockIdx.y, pb = blockIdx.z;
    const size_t n = a.len[job];
    if ((size_t)blockIdx.x * HS_T * HS_L >= n) return;                  // the whole workgroup: nobody is left at a barrier
    const size_t shift = 4 * (size_t)pb * ws;
    const size_t v_at = 4 * ((size_t)pb * ws + (size_t)job * a.vstride);   // the job's row of workgroup values and of carries
    horner_scan_body<APPLY>(a.coeffs[job] + (((a.own >> job) & 1u) ? shift : 0), n, pb_par(par, pb, a.zslot[job]), APPLY ? nullptr : vals + v_at,
                            APPLY ? carries + v_at : nullptr, APPLY ? a.quotient[job] + shift : nullptr, APPLY ? evals + shift + 4 * job : nullptr);
}
// grid (jobs, proofs); evals == nullptr: the carries alone
static __global__ __launch_bounds__(1024) void horner_batch_top_kernel(HornerBatchArg a, const uint64_t* __restrict__ par, const uint64_t* __restrict__ vals,
                                                                     uint64_t* __restrict__ carries, uint64_t* __restrict__ evals, size_t ws) {
    const uint32_t job = blockIdx.x, pb = blockIdx.y;
    const uint32_t n_blocks = (uint32_t)(((size_t)a.len[job] + (size_t)HS_T * HS_L - 1) / ((size_t)HS_T * HS_L));
    const size_t v_at = 4 * ((size_t)pb * ws + (size_t)job * a.vstride);
    horner_top_body(vals + v_at, n_blocks, pb_par(par, pb, a.zslot[job]), carries + v_at, evals ? evals + 4 * ((size_t)pb * ws + job) : nullptr);
}

}  // namespace zk
