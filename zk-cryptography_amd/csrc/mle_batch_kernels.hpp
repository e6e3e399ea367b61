// mle_batch_kernels.hpp -- MultilinearTrait::evaluation (evaluation_form.rs:162-175) of a BATCH of tables and points
// (zkhip_mle_evaluation_batch; the regimes, the chunks and the workspace layout: mle_batch_plan.hpp).
//
// Job b evaluates the table tables[b] (n entries; a pointer may repeat, tables are only read) at its own points
// pts[b * n_pts .. (b + 1) * n_pts) from device memory.  A workgroup stages at most 2^12 entries in LDS -- exactly 32 bytes of dynamic
// LDS per entry, so that small tables share a CU -- and folds them with fold_tail_kernel's body.  No workgroup waits for another:
// a table of 2^h blocks leaves 2^h records and a second launch adds them up.  Field arithmetic is exact and every value is kept
// reduced, so the sum over blocks has the limbs the single call's chain of folds has.
#pragma once
#include "mle_batch_plan.hpp"
#include "mle_kernels.hpp"

namespace zk {

static_assert(MEB_TAIL_LOG == (uint32_t)TAIL_LOG && MEB_BLOCK == (uint32_t)MLE_BLOCK, "mle_batch_plan.hpp restates mle_kernels.hpp");

// n <= 2^12: grid (jobs), 32 n bytes of dynamic LDS; LANES = meb_lanes(log2 n).  n == 1: the entry itself.
template <int LANES>
static __global__ __launch_bounds__(LANES) void mle_eval_batch_resident_kernel(const uint64_t* const* __restrict__ tables, uint32_t n,
                                                                                   const uint64_t* __restrict__ pts, uint32_t n_pts,
                                                                                   uint64_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];
    Fr* tab = reinterpret_cast<Fr*>(zk_dyn_lds);
    const uint32_t b = blockIdx.x;
    const uint64_t* job_pts = pts + 4 * (size_t)b * n_pts;
    fold_tail_body<LANES>(tab, tables[b], n, n_pts, [&](uint32_t p) { return load_fr(job_pts, p); });
    if (threadIdx.x == 0) store_fr(out, b, tab[0]);
}

// 2^13 <= n: grid (2^h, jobs), h = n_pts - 12.  Workgroup (q, b) folds block q of table b with the job's points h .. n_pts - 1 and
// stores value * eq_q(points 0 .. h - 1) at records[b * 2^h + q].  MEB_WIDE_BLOCK lanes: a block is 2^12 entries.
static __global__ __launch_bounds__(MEB_WIDE_BLOCK) void mle_eval_batch_blocks_kernel(const uint64_t* const* __restrict__ tables, uint32_t h,
                                                                                 const uint64_t* __restrict__ pts, uint32_t n_pts,
                                                                                 uint64_t* __restrict__ records) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];
    Fr* tab = reinterpret_cast<Fr*>(zk_dyn_lds);
    const uint32_t q = blockIdx.x, b = blockIdx.y;
    const uint64_t* job_pts = pts + 4 * (size_t)b * n_pts;
    fold_tail_body<(int)MEB_WIDE_BLOCK>(tab, tables[b] + 4 * ((size_t)q << TAIL_LOG), (uint32_t)TAIL_N, n_pts - h, [&](uint32_t p) { return load_fr(job_pts, h + p); });
    if (threadIdx.x == 0) {
        Fr v = tab[0];
        const Fr one = Fr::one();
        for (uint32_t i = 0; i < h; ++i) {
            const Fr r = load_fr(job_pts, i);
            v = v * (meb_weight_bit(q, h, i) ? r : one - r);
        }
        store_fr(records, ((size_t)b << h) + q, v);
    }
}

// out[b] = sum of records[b * per_job .. (b + 1) * per_job), one lane per job (per_job <= 16)
static __global__ __launch_bounds__(MLE_BLOCK) void mle_eval_batch_sum_kernel(const uint64_t* __restrict__ records, uint32_t per_job, uint32_t jobs,
                                                                              uint64_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * MLE_BLOCK + threadIdx.x;
    if (b >= jobs) return;
    Fr s = load_fr(records, (size_t)b * per_job);
    for (uint32_t q = 1; q < per_job; ++q) s = s + load_fr(records, (size_t)b * per_job + q);
    store_fr(out, b, s);
}

}  // namespace zk
