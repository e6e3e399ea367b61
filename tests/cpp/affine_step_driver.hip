// Test-only launcher for csrc/affine_step.hpp (tests/test_gpu_affine_step.py): the header alone, nothing of libzkhip linked.
// One triple (t, D, d) per row of 16 lanes, as the serial prover kernel uses the routine: lanes 0 .. 9 of the row build the table
// T_k = D * 2^(28 k) mod r in LDS, a barrier hands it over, then the row takes the digest-dependent step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../zk-cryptography_amd/csrc/affine_step.hpp"

using namespace zk;

constexpr int DRV_BLOCK = 256, DRV_ROWS = DRV_BLOCK / 16;

// t, D: canonical limbs; d: the raw 256 bits, little-endian limbs; 8 words per triple each.  n is padded by the host to whole blocks.
static __global__ __launch_bounds__(DRV_BLOCK) void affine_step_kernel(const uint32_t* __restrict__ t, const uint32_t* __restrict__ D,
                                                                       const uint32_t* __restrict__ d, uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t tbl[DRV_ROWS * AFF_TABLE_WORDS];
    const uint32_t lane = threadIdx.x & 15, row = threadIdx.x >> 4;
    const size_t triple = (size_t)blockIdx.x * DRV_ROWS + row;
    uint32_t* mine = tbl + row * AFF_TABLE_WORDS;
    if (lane < (uint32_t)AFF_DIGITS) {
        Fr dv;
#pragma unroll
        for (int i = 0; i < 8; ++i) dv.l[i] = D[8 * triple + i];
        affine_table_store(mine, lane, dv * affine_pow_mont(lane));
    }
    __syncthreads();
    uint32_t dl[8], dg[AFF_DIGITS];
#pragma unroll
    for (int i = 0; i < 8; ++i) dl[i] = d[8 * triple + i];
    affine_digits(dl, dg);
    AffineLane c;
    c.init();
    const uint32_t r = affine_step_rows(c, t[8 * triple + (lane & 7)], mine, dg);
    if (lane < 8) out[8 * triple + lane] = r;
}

// device pointers; n_triples a multiple of 16.  Returns the HIP error of the launch and the wait for it.
extern "C" int affine_step_driver(const void* t, const void* D, const void* d, size_t n_triples, void* out) {
    if (n_triples == 0 || n_triples % DRV_ROWS) return -1;
    hipLaunchKernelGGL(affine_step_kernel, dim3((unsigned)(n_triples / DRV_ROWS)), dim3(DRV_BLOCK), 0, 0, (const uint32_t*)t,
                       (const uint32_t*)D, (const uint32_t*)d, (uint32_t*)out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}
