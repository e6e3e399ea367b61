// circuit_eval_batch_kernels.hpp -- Circuit::evaluation (circuit/src/circuit.rs:31-57) of a batch of inputs on the resident circuit,
// for gfx950.  Gate g of layer k holds below[in0] + below[in1] or below[in0] * below[in1], `below` being layer k + 1 or the input.
//
// Gate indices and types are the resident circuit's arrays (gkr.hip: LayerDev::in0 / in1 / type); where an input's tables are comes
// from the device pointer table of the call, entry b * stride + k = layer k of input b, k = stride - 1 the input (stride = n_layers + 1:
// the array zkhip_gkr_prove_batch takes).  Two kernels (which layer gets which: circuit_eval_plan.hpp):
//   circuit_eval_wide_kernel   one layer of every input of a chunk, one gate per lane: grid (gate tiles, inputs)
//   circuit_eval_tail_kernel   layers `top` .. 0 of one input per workgroup.  Every layer is written to its table in global memory and
//                              the next one reads it from there behind a workgroup barrier: a workgroup's waves share their CU's
//                              vector cache, so what the barrier orders within the workgroup is all the hand-off needs.
// No workgroup waits for another, in either kernel: a layer that other workgroups wrote is read by the NEXT launch.
// The arithmetic is circuit_layer_kernel's (mle_kernels.hpp): the same operators on the same operands, so the same limbs.
#pragma once
#include "circuit_eval_plan.hpp"
#include "fp.hpp"

namespace zk {

struct CebLayer {                    // one layer of the resident circuit as the kernels read it (uploaded with the circuit)
    const uint32_t *in0, *in1;
    const uint8_t* type;
    uint32_t n_gates, pad_;
};

// the value tables are plain pointers (no __restrict__ on them): the tail reads what it has just written
__device__ __forceinline__ void ceb_gate(const CebLayer& L, const uint64_t* below, uint64_t* out, uint32_t g) {
    const Fr x = load_fr(below, L.in0[g]), y = load_fr(below, L.in1[g]);
    store_fr(out, g, L.type[g] ? x * y : x + y);
}

static __global__ __launch_bounds__(CEB_TILE) void circuit_eval_wide_kernel(CebLayer L, const uint64_t* const* __restrict__ ptrs, uint32_t stride,
                                                                           uint32_t k) {
    const uint32_t g = blockIdx.x * CEB_TILE + threadIdx.x;
    if (g >= L.n_gates) return;
    const uint64_t* const* row = ptrs + (size_t)blockIdx.y * stride + k;
    ceb_gate(L, row[1], const_cast<uint64_t*>(row[0]), g);
}

static __global__ __launch_bounds__(CEB_TAIL_BLOCK) void circuit_eval_tail_kernel(const CebLayer* __restrict__ layers,
                                                                                 const uint64_t* const* __restrict__ ptrs, uint32_t stride, uint32_t top) {
    const uint64_t* const* row = ptrs + (size_t)blockIdx.x * stride;
    for (uint32_t k = top + 1; k-- > 0;) {
        const CebLayer L = layers[k];
        const uint64_t* below = row[k + 1];
        uint64_t* out = const_cast<uint64_t*>(row[k]);
        for (uint32_t g = threadIdx.x; g < L.n_gates; g += CEB_TAIL_BLOCK) ceb_gate(L, below, out, g);
        __syncthreads();             // layer k is in its table before any lane reads it as `below`
    }
}

}  // namespace zk
