// horner_jobs_kernels.hpp -- the Horner suffix scan of mle_kernels.hpp over a LIST OF JOBS, each a polynomial and a point of its own:
// zkhip_univariate_kzg_open_batch's chunk (univariate_open_plan.hpp).  The arithmetic is horner_scan_body / horner_top_body, unchanged;
// these kernels resolve a job's pointers and call them.
//
// The list is a table in device memory, written by one copy per chunk (HornerBatchArg of plonk_batch_kernels.hpp is a by-value struct of a
// proof's few jobs; a chunk here holds up to 1024):
//     [ HornerJobsHead: one zero field element ][ HornerJob x count ][ uint32 order[count] ]
// order lists the SHORT jobs (at most HS_T * HS_L coefficients) first, then the LONG ones; a launch takes its job from order[first + blockIdx.y].
//
// SHORT: one workgroup is the whole scan, and its carry-in is zero: the APPLY body with the head's zero as its carry already leaves the
// quotient and V_0.  One launch, grid (1, short jobs) -- no pass 1, no top.
// LONG: scan over grid (workgroups of the longest job, long jobs), top over grid (long jobs), apply as the scan.  A workgroup beyond its
// own job's count leaves before the body's first barrier -- the whole workgroup, the condition is uniform.  The top pass shares out the
// JOB's workgroups among its lanes (n_blocks is the job's own), so a job of more than 1024 workgroups gives a lane several.
// Bounds: a job writes n - 1 quotient elements at q_off, n_blocks values and n_blocks carries at row_off, one evaluation at its index of
// `evals`: the planner lays these out without overlap inside the chunk's scratch.
#pragma once
#include "mle_kernels.hpp"

namespace zk {

struct HornerJob {                      // 64 bytes; z at a 16-byte offset (load_fr reads it as two uint4)
    const uint64_t* coeffs;
    uint64_t n;
    uint64_t z[4];
    uint64_t q_off;                     // quotient, in field elements from `scratch`
    uint64_t row_off;                   // LONG: values, then carries, in field elements from `scratch`
};
struct HornerJobsHead { uint64_t zero[4]; uint64_t pad[4]; };
static_assert(sizeof(HornerJob) == 64 && sizeof(HornerJobsHead) == 64, "the job table's layout");

__device__ __forceinline__ uint32_t horner_job_blocks(uint64_t n) { return (uint32_t)((n + (uint64_t)(HS_T * HS_L) - 1) / (uint64_t)(HS_T * HS_L)); }

static __global__ __launch_bounds__(HS_T) void horner_jobs_short_kernel(const HornerJobsHead* __restrict__ head, const HornerJob* __restrict__ jobs,
                                                                        const uint32_t* __restrict__ order, uint64_t* __restrict__ scratch,
                                                                        uint64_t* __restrict__ evals) {
    const uint32_t k = order[blockIdx.y];
    const HornerJob& j = jobs[k];
    // blockIdx.x == 0: the body's carry is head->zero
    horner_scan_body<true>(j.coeffs, (size_t)j.n, load_fr(j.z, 0), nullptr, head->zero, scratch + 4 * j.q_off, evals + 4 * (size_t)k);
}
template <bool APPLY>
static __global__ __launch_bounds__(HS_T) void horner_jobs_scan_kernel(const HornerJob* __restrict__ jobs, const uint32_t* __restrict__ order,
                                                                       uint32_t first, uint64_t* __restrict__ scratch, uint64_t* __restrict__ evals) {
    const uint32_t k = order[first + blockIdx.y];
    const HornerJob& j = jobs[k];
    const uint32_t n_blocks = horner_job_blocks(j.n);
    if (blockIdx.x >= n_blocks) return;                                 // the whole workgroup: nobody is left at a barrier
    uint64_t* const vals = scratch + 4 * j.row_off;
    horner_scan_body<APPLY>(j.coeffs, (size_t)j.n, load_fr(j.z, 0), APPLY ? nullptr : vals, APPLY ? vals + 4 * (size_t)n_blocks : nullptr,
                            APPLY ? scratch + 4 * j.q_off : nullptr, APPLY ? evals + 4 * (size_t)k : nullptr);
}
static __global__ __launch_bounds__(1024) void horner_jobs_top_kernel(const HornerJob* __restrict__ jobs, const uint32_t* __restrict__ order,
                                                                      uint32_t first, uint64_t* __restrict__ scratch) {
    const HornerJob& j = jobs[order[first + blockIdx.x]];
    const uint32_t n_blocks = horner_job_blocks(j.n);
    uint64_t* const vals = scratch + 4 * j.row_off;
    horner_top_body(vals, n_blocks, load_fr(j.z, 0), vals + 4 * (size_t)n_blocks, nullptr);
}

}  // namespace zk
