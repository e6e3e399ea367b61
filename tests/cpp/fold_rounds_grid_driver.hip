// fold_rounds_grid_driver.hip -- test-only launchers for fold_rounds_kernel of csrc/fold_rounds.hpp at a grid the caller chooses
// (tests/test_gpu_fold_rounds_grid.py).
//
// fold_rounds_driver.hip's comparison with the number of fold workgroups F as an argument: the schedule of the fold workgroups
// (csrc/fold_schedule.hpp) is a function of the grid, and the kernel must leave the same bits at every grid of two or more workgroups.
//   separate (fused = 0): blockfold_kernel, then sumcheck_small_kernel, then multifold_mfma_kernel<4, 4>; `wgs` is not read;
//   fused    (fused = 1): blockfold_kernel, then fold_rounds_kernel at grid 1 + wgs.
// Buffers, shapes and return values are fold_rounds_driver.hip's.  Nothing of libzkhip is linked: the headers alone.
#include <hip/hip_runtime.h>

#include "../../zk-cryptography_amd/csrc/fold_rounds.hpp"

using namespace zk;

extern "C" {

// info[2] = bytes of the transcript state, fold workgroups of the one-tile-per-wave grid for m outputs
int fold_rounds_grid_driver_info(unsigned long long m, unsigned* info) {
    if (!info) return hipErrorInvalidValue;
    info[0] = (unsigned)sizeof(SumcheckDev); info[1] = fold_rounds_workgroups((size_t)m);
    return hipSuccess;
}
unsigned fold_rounds_grid_driver_slices(unsigned k1, unsigned k2) {
    BlockfoldShape sh = {};
    return k2 <= (unsigned)TREE_MAX_LOG && blockfold_shape(1u << k2, k1, &sh) ? sh.ny : 0u;
}
// what the schedule says of T tiles on wgs workgroups: sched[4] = waves, q, rem, leftovers of workgroup 0
int fold_rounds_grid_driver_schedule(unsigned long long tiles, unsigned wgs, unsigned long long* sched) {
    if (!sched || wgs == 0) return hipErrorInvalidValue;
    const FoldSchedule s = fold_schedule((size_t)tiles, wgs);
    sched[0] = s.waves; sched[1] = s.q; sched[2] = s.rem; sched[3] = fold_wg_leftovers(s, 0);
    return hipSuccess;
}

int fold_rounds_grid_driver_run(int fused, unsigned wgs, const uint64_t* table, unsigned long long m, unsigned k, unsigned k2,
                                const uint64_t* w, const uint64_t* fine, uint64_t* p1, uint64_t* w2, void* st, uint64_t* rp, uint64_t* ch,
                                unsigned round0, uint64_t* out, uint64_t* partials, unsigned rot, void* stream) {
    BlockfoldShape sh = {};
    if (!table || !w || !fine || !p1 || !w2 || !st || !rp || !ch || !out || !partials) return hipErrorInvalidValue;
    if (m < 8192 || m % 256 != 0 || k < 4 || k > (unsigned)MF_CAP_LOGK || k2 < 3 || k2 > (unsigned)TREE_MAX_LOG) return hipErrorInvalidValue;
    if (fused && (wgs == 0 || wgs > fold_rounds_workgroups((size_t)m))) return hipErrorInvalidValue;   // (more would only add idle workgroups)
    if (!blockfold_shape(1u << k2, k, &sh)) return hipErrorInvalidValue;
    const size_t small_lds = small_lds_bytes(k2, (int)k2, false);
    const size_t q_bytes = mfm_lds_bytes((1u << k) < (uint32_t)MFM_CHUNK ? (1u << k) : (uint32_t)MFM_CHUNK);
    if (small_lds > FOLD_ROUNDS_LDS || q_bytes + FOLD_ROUNDS_XCH > FOLD_ROUNDS_LDS) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(blockfold_kernel, dim3((1u << k2) >> sh.log_ow, sh.ny), dim3(BF_BLOCK), 0, s, fine, 1u << k2, sh.sl, sh.per, w, p1);
    SmallArgs a = {};
    a.src = p1; a.group = sh.ny; a.stride = 1u << k2; a.canon = 1; a.log_n = k2; a.n_rounds = k2; a.round0 = round0; a.weights_out = w2;
    hipError_t e;
    if (fused) {
        e = hipFuncSetAttribute((const void*)fold_rounds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 158 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(fold_rounds_kernel, dim3(1 + wgs), dim3(64 * FOLD_ROUNDS_WAVES), FOLD_ROUNDS_LDS, s, a, (SumcheckDev*)st, rp, ch,
                           table, (size_t)m, k, w, out, rot);
    } else {
        e = hipFuncSetAttribute((const void*)sumcheck_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(sumcheck_small_kernel, dim3(1), dim3(SMALL_BLOCK), FOLD_ROUNDS_LDS, s, a, (SumcheckDev*)st, rp, ch);
        hipLaunchKernelGGL((multifold_mfma_kernel<4, 4>), dim3((unsigned)(m / 256)), dim3(256), q_bytes, s, table, (size_t)m, k, w, out, partials, rot);
    }
    return hipGetLastError();
}

}  // extern "C"
