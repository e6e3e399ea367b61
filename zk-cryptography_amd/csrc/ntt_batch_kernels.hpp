// ntt_batch_kernels.hpp -- a batch of transforms of one size per launch (zkhip_domain_transform_batch, zkhip_univariate_multiply_batch).
//
// Row b of a batch is the transform of in + 4 b in_stride (n_src values, zero beyond; times in2's row b element-wise when in2 is
// given) into out + 4 b out_stride; strides count field elements.  Every row uses the one twiddle table / pass plan of its size, and
// the butterflies are the single transform's own (ntt_kernels.hpp: ntt_lds_stages, ntt_first8_body, ntt_pass_body) -- field
// arithmetic is exact, so a row equals the single call limb for limb.
//   n <= 2^11: ntt_batch_small_kernel<TILE_LOG>, all log_n stages in one LDS tile; a tile of 2^TILE_LOG elements holds
//              2^(TILE_LOG - log_n) whole rows.  TILE_LOG = 10 (256 threads) up to 2^10, TILE_LOG = 11 (512 threads, the tile of the
//              >= 2^12-point passes) for 2^11 -- one workgroup and one launch per row instead of two workgroups and three launches.
//   n >= 2^12: ntt_batch_first8_kernel and ntt_batch_pass_kernel<>, the single transform's workgroups with the row on blockIdx.y.
#pragma once
#include "ntt_kernels.hpp"

namespace zk {

// in / out may be the same rows (in place, in_stride == out_stride): a workgroup reads all of its rows before it writes any, and no
// other workgroup touches them.  Lanes of the last workgroup whose row is >= batch neither load nor store.  scaled: the outputs are
// multiplied by `scale` (the inverse transform's 1/n) on their way out.  Only the first n_dst outputs of a row are stored.
// log_n == 0 is the padded copy (tw is not read).
template <int TILE_LOG>
static __global__ __launch_bounds__(1 << (TILE_LOG - 2)) void ntt_batch_small_kernel(
    const uint64_t* in, size_t in_stride, size_t n_src, const uint64_t* in2, size_t in2_stride, uint64_t* out, size_t out_stride,
    size_t n_dst, uint32_t batch, uint32_t log_n, const uint64_t* __restrict__ tw, FrArg scale, uint32_t scaled) {
    constexpr uint32_t TILE = 1u << TILE_LOG, BLOCK = TILE / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];
    Fr* tab = reinterpret_cast<Fr*>(zk_dyn_lds);
    const uint32_t n = 1u << log_n;
    const uint32_t first = blockIdx.x << (TILE_LOG - log_n);                    // this workgroup's first row
    const uint32_t rows = min(TILE >> log_n, batch - first);                    // >= 1: the grid is ceil(batch / rows per tile)
    const uint32_t live = rows << log_n;                                        // elements of the tile that belong to a row
    for (uint32_t q = threadIdx.x; q < live; q += BLOCK) {
        const size_t row = first + (q >> log_n);
        const uint32_t src = log_n ? bitrev(q & (n - 1), log_n) : 0u;
        Fr v = src < n_src ? load_fr(in + 4 * row * in_stride, src) : Fr::zero();
        if (in2 && src < n_src) v = v * load_fr(in2 + 4 * row * in2_stride, src);
        tab[q] = v;
    }
    __syncthreads();
    ntt_lds_stages<(int)BLOCK>(tab, live / 2, log_n, log_n, tw);
    const Fr sc = fr_from_arg(scale);
    for (uint32_t q = threadIdx.x; q < live; q += BLOCK) {
        const size_t row = first + (q >> log_n);
        const uint32_t i = q & (n - 1);
        if (i < n_dst) store_fr(out + 4 * row * out_stride, i, scaled ? tab[q] * sc : tab[q]);
    }
}

// grid (n >> 11, batch); the arguments of ntt_first8_kernel with a stride per operand
static __global__ __launch_bounds__(NTT_BIG_BLOCK) void ntt_batch_first8_kernel(const uint64_t* __restrict__ in, size_t in_stride, size_t n_src,
                                                                                const uint64_t* __restrict__ in2, size_t in2_stride,
                                                                                uint64_t* __restrict__ out, size_t out_stride, uint32_t log_n,
                                                                                const uint64_t* __restrict__ tw1) {
    const size_t row = blockIdx.y;
    ntt_first8_body(blockIdx.x, in + 4 * row * in_stride, n_src, in2 ? in2 + 4 * row * in2_stride : nullptr, out + 4 * row * out_stride,
                    log_n, tw1);
}

// grid (n >> 11, batch); src and dst may be the same rows (a workgroup writes the tile it read)
template <bool LAST_SCALED>
static __global__ __launch_bounds__(NTT_BIG_BLOCK) void ntt_batch_pass_kernel(const uint64_t* src, size_t src_stride, uint64_t* dst, size_t dst_stride,
                                                                              uint32_t s0, uint32_t T, const uint64_t* __restrict__ tw,
                                                                              FrArg scale, size_t n_dst) {
    const size_t row = blockIdx.y;
    ntt_pass_body<LAST_SCALED>(blockIdx.x, src + 4 * row * src_stride, dst + 4 * row * dst_stride, s0, T, tw, scale, n_dst);
}

}  // namespace zk
