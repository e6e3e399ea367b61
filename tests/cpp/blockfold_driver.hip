// blockfold_driver.hip -- test-only launchers for blockfold_kernel and blockfold_shape of csrc/multifold_kernels.hpp
// (tests/test_gpu_blockfold.py, tests/test_blockfold_driver_cpu.py).
//
// The kernel gets the grid, the block and the split of the terms that blockfold_shape gives it -- the rule csrc/zkhip.hip launches it
// with.  Pointers are device pointers; a launcher returns hipGetLastError(), or hipErrorInvalidValue WITHOUT touching a device for a
// null pointer or an (m, k) the shape function refuses: m no power of two, fewer outputs than one workgroup takes (log_ow > log2 m),
// k = 0, more than 2^10 terms.  Nothing of libzkhip is linked: the header alone.
#include <hip/hip_runtime.h>

#include "../../zk-cryptography_amd/csrc/multifold_kernels.hpp"

using namespace zk;

extern "C" {

int blockfold_driver_block() { return BF_BLOCK; }

// shape[5] = log_ow, slices, per, ny, workgroups
int blockfold_driver_shape(unsigned m, unsigned k, unsigned* shape) {
    BlockfoldShape sh = {};
    if (!shape || !blockfold_shape(m, k, &sh)) return hipErrorInvalidValue;
    shape[0] = sh.log_ow; shape[1] = sh.sl; shape[2] = sh.per; shape[3] = sh.ny; shape[4] = (m >> sh.log_ow) * sh.ny;
    return hipSuccess;
}

// in: 2^k x m elements (Montgomery form); weights: 2^k (Montgomery form, with the factor 2^32); partial: ny x m canonical integers
int blockfold_driver_run(const uint64_t* in, unsigned m, unsigned k, const uint64_t* weights, uint64_t* partial, void* stream) {
    BlockfoldShape sh = {};
    if (!in || !weights || !partial || !blockfold_shape(m, k, &sh)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blockfold_kernel, dim3(m >> sh.log_ow, sh.ny), dim3(BF_BLOCK), 0, (hipStream_t)stream, in, (uint32_t)m, sh.sl, sh.per,
                       weights, partial);
    return hipGetLastError();
}

}  // extern "C"
