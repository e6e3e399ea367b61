// plonk_kernels_driver.hip -- test-only launchers for the kernels of csrc/plonk_kernels.hpp (tests/test_gpu_plonk_kernels.py).
//
// One extern "C" launcher per kernel.  Pointers are device pointers unless named h_*; a field scalar is four uint64 Montgomery limbs on
// the host.  The five streaming kernels take their grid from the caller, so that a test reaches the second and later iterations of a
// lane's loop at a few thousand items; the grand-product passes use the prover's grid.  A launcher returns hipGetLastError(), or
// hipErrorInvalidValue WITHOUT launching for an argument with which a kernel would index outside what the caller declared.
// Nothing of libzkhip is linked: the header alone.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../zk-cryptography_amd/csrc/plonk_kernels.hpp"

using namespace zk;

namespace {

constexpr unsigned MAX_GRID = 1u << 16;            // far above any grid a test asks for; keeps a wrong argument from a huge launch
inline FrArg arg(const uint64_t* h) { FrArg r; std::memcpy(r.v, h, 32); return r; }
inline bool bad_grid(unsigned grid) { return grid == 0 || grid > MAX_GRID; }
inline bool pow2(size_t v) { return v && !(v & (v - 1)); }
inline hipStream_t st(void* s) { return (hipStream_t)s; }

}  // namespace

extern "C" {

// the grid the prover gives a streaming kernel over n_items, and the rows of one grand-product workgroup
int plonk_driver_stream_grid(size_t n_items) { return mle_grid_stream(n_items); }
int plonk_driver_gp_rows() { return GP_ROWS; }
int plonk_driver_flag_count() { return PLONK_FLAGS; }

int plonk_driver_powers(const uint64_t* h_base, const uint64_t* h_scale, size_t count, uint64_t* out, unsigned grid, void* stream) {
    if (!h_base || !h_scale || !out || count == 0 || bad_grid(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plonk_powers_kernel, dim3(grid), dim3(MLE_BLOCK), 0, st(stream), arg(h_base), arg(h_scale), count, out);
    return hipGetLastError();
}

int plonk_driver_scale_pad(const uint64_t* a, const uint64_t* b, size_t n_src, size_t n, uint64_t* out, unsigned grid, void* stream) {
    if (!a || !b || !out || n == 0 || n_src > n || bad_grid(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plonk_scale_pad_kernel, dim3(grid), dim3(MLE_BLOCK), 0, st(stream), a, b, n_src, n, out);
    return hipGetLastError();
}

// p: n + k elements; h_b: k scalars
int plonk_driver_blind(uint64_t* p, size_t n, unsigned k, const uint64_t* h_b, void* stream) {
    if (!p || !h_b || n == 0 || k == 0 || k > 3 || k >= n) return hipErrorInvalidValue;
    PlonkBlindArg b = {};
    std::memcpy(b.v, h_b, 32 * k);
    hipLaunchKernelGGL(plonk_blind_kernel, dim3(1), dim3(64), 0, st(stream), p, n, (uint32_t)k, b);
    return hipGetLastError();
}

// cols: 8 device pointers (q_m, q_l, q_r, q_o, q_c, sigma_1, sigma_2, sigma_3) in a host array; every vector n elements, f_out n,
// block_prod ceil(n / GP_ROWS), flags PLONK_FLAGS ints
int plonk_driver_gp_ratio(const uint64_t* wa, const uint64_t* wb, const uint64_t* wc, const uint64_t* pub, const uint64_t* const* h_cols,
                          const uint64_t* omega_pow, size_t n, const uint64_t* h_beta, const uint64_t* h_gamma, uint64_t* f_out,
                          uint64_t* block_prod, int* flags, void* stream) {
    if (!wa || !wb || !wc || !pub || !h_cols || !omega_pow || !h_beta || !h_gamma || !f_out || !block_prod || !flags || n == 0)
        return hipErrorInvalidValue;
    PlonkCols cols;
    for (int j = 0; j < 8; ++j) {
        if (!h_cols[j]) return hipErrorInvalidValue;
        cols.q[j] = h_cols[j];
    }
    const size_t nb = (n + GP_ROWS - 1) / GP_ROWS;
    if (nb > MAX_GRID) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plonk_gp_ratio_kernel, dim3((unsigned)nb), dim3(GP_T), 0, st(stream), wa, wb, wc, pub, cols, omega_pow, n, arg(h_beta),
                       arg(h_gamma), f_out, block_prod, flags);
    return hipGetLastError();
}

int plonk_driver_gp_top(const uint64_t* block_prod, unsigned n_blocks, uint64_t* block_excl, void* stream) {
    if (!block_prod || !block_excl || n_blocks == 0 || n_blocks > (1u << 24)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plonk_gp_top_kernel, dim3(1), dim3(1024), 0, st(stream), block_prod, (uint32_t)n_blocks, block_excl);
    return hipGetLastError();
}

int plonk_driver_gp_apply(const uint64_t* f_in, const uint64_t* block_excl, size_t n, uint64_t* acc, int* flags, void* stream) {
    if (!f_in || !block_excl || !acc || !flags || n == 0) return hipErrorInvalidValue;
    const size_t nb = (n + GP_ROWS - 1) / GP_ROWS;
    if (nb > MAX_GRID) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plonk_gp_apply_kernel, dim3((unsigned)nb), dim3(GP_T), 0, st(stream), f_in, block_excl, n, acc, flags);
    return hipGetLastError();
}

// ev: 5 D elements, pre: 10 D, t_out: D; h_scalars: beta, gamma, alpha, alpha2; h_zh_inv: 8 scalars
int plonk_driver_quotient(const uint64_t* ev, const uint64_t* pre, size_t D, unsigned rot, const uint64_t* h_scalars, const uint64_t* h_zh_inv,
                          uint64_t* t_out, unsigned grid, void* stream) {
    if (!ev || !pre || !h_scalars || !h_zh_inv || !t_out || bad_grid(grid)) return hipErrorInvalidValue;
    if (!pow2(D) || (rot != 4 && rot != 8) || D < rot) return hipErrorInvalidValue;
    PlonkQuotArg q = {};
    q.beta = arg(h_scalars); q.gamma = arg(h_scalars + 4); q.alpha = arg(h_scalars + 8); q.alpha2 = arg(h_scalars + 12);
    for (int j = 0; j < 8; ++j) q.zh_inv[j] = arg(h_zh_inv + 4 * j);
    q.rot = rot;
    hipLaunchKernelGGL(plonk_quotient_kernel, dim3(grid), dim3(MLE_BLOCK), 0, st(stream), ev, pre, D, q, t_out);
    return hipGetLastError();
}

// t: D elements, ginv_pow: 3 n + 6, tl and tm: n + 1, th: n + 6
int plonk_driver_split(const uint64_t* t, const uint64_t* ginv_pow, size_t n, size_t D, const uint64_t* h_b10, const uint64_t* h_b11, uint64_t* tl,
                       uint64_t* tm, uint64_t* th, int* flags, unsigned grid, void* stream) {
    if (!t || !ginv_pow || !h_b10 || !h_b11 || !tl || !tm || !th || !flags || bad_grid(grid)) return hipErrorInvalidValue;
    if (n == 0 || !pow2(D) || D < 3 * n + 6) return hipErrorInvalidValue;
    hipLaunchKernelGGL(plonk_split_kernel, dim3(grid), dim3(MLE_BLOCK), 0, st(stream), t, ginv_pow, n, D, arg(h_b10), arg(h_b11), tl, tm, th, flags);
    return hipGetLastError();
}

// h_ptrs: PLONK_LIN_TERMS device pointers (len elements each; they may coincide); h_weights: PLONK_LIN_TERMS scalars; out: len
int plonk_driver_linearise(const uint64_t* const* h_ptrs, const uint64_t* h_weights, const uint64_t* h_c0, size_t len, uint64_t* out, unsigned grid,
                           void* stream) {
    if (!h_ptrs || !h_weights || !h_c0 || !out || len == 0 || bad_grid(grid)) return hipErrorInvalidValue;
    PlonkLinArg L = {};
    for (int j = 0; j < PLONK_LIN_TERMS; ++j) {
        if (!h_ptrs[j]) return hipErrorInvalidValue;
        L.p[j] = h_ptrs[j];
        L.s[j] = arg(h_weights + 4 * j);
    }
    L.c0 = arg(h_c0);
    hipLaunchKernelGGL(plonk_linearise_kernel, dim3(grid), dim3(MLE_BLOCK), 0, st(stream), L, len, out);
    return hipGetLastError();
}

}  // extern "C"
