// mle_kernels_driver.hip -- test-only launchers for the kernels of csrc/mle_kernels.hpp and the three helpers of `evaluation` in
// csrc/multifold_kernels.hpp (tests/test_gpu_mle_kernels.py, tests/test_mle_model_cpu.py).
//
// Every grid-stride kernel takes its GRID as an argument, so that its loop can be stepped at small n; mle_driver_grid gives the grid
// the library would launch.  Pointers are device pointers unless a name starts with h_ (host: a field element of 4 words, or a list of
// points, passed to the kernel by value as the library does).  A launcher returns hipGetLastError(), or hipErrorInvalidValue WITHOUT
// touching a device for a null pointer, a grid of 0 or above 2^20 workgroups, or a shape the kernel cannot take.  Nothing of libzkhip
// is linked: the headers alone.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../zk-cryptography_amd/csrc/multifold_kernels.hpp"

using namespace zk;

namespace {

constexpr unsigned MAX_POINTS = 48;   // PtsArg
inline bool grid_ok(unsigned g) { return g >= 1 && g <= (1u << 20); }
inline bool pow2(size_t n) { return n && !(n & (n - 1)); }
inline unsigned log2u(size_t n) { unsigned l = 0; while (((size_t)1 << l) < n) ++l; return l; }
inline FrArg fr_arg(const uint64_t* h) { FrArg a = {}; if (h) std::memcpy(a.v, h, 32); return a; }
inline PtsArg pts_arg(const uint64_t* h, unsigned n) { PtsArg a = {}; if (h && n) std::memcpy(a.v, h, 32 * (size_t)n); return a; }
inline unsigned horner_blocks(size_t n) { return (unsigned)((n + (size_t)HS_T * HS_L - 1) / ((size_t)HS_T * HS_L)); }
inline hipStream_t S(void* s) { return (hipStream_t)s; }

}  // namespace

extern "C" {

int mle_driver_block() { return MLE_BLOCK; }
int mle_driver_horner_block() { return HS_T * HS_L; }
int mle_driver_tail_n() { return TAIL_N; }
// the grid the library launches a kernel over n_items with: mle_grid_stream (stream != 0) or mle_grid
int mle_driver_grid(size_t n_items, int stream) { return stream ? mle_grid_stream(n_items) : mle_grid(n_items); }

// fold_kernel: in 2 n_out entries, out n_out; the point from h_r (by value) or d_r; partials (2 per workgroup) selects WITH_SUMS
int mle_driver_fold(const uint64_t* in, uint64_t* out, size_t n_out, unsigned log_half, const uint64_t* h_r, const uint64_t* d_r,
                    uint64_t* partials, unsigned grid, void* stream) {
    if (!in || !out || (!h_r == !d_r) || !grid_ok(grid) || !pow2(n_out) || log_half > log2u(n_out)) return hipErrorInvalidValue;
    if (partials)
        hipLaunchKernelGGL(fold_kernel<true>, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), in, out, n_out, log_half, d_r, fr_arg(h_r), partials);
    else
        hipLaunchKernelGGL(fold_kernel<false>, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), in, out, n_out, log_half, d_r, fr_arg(h_r), partials);
    return hipGetLastError();
}

// half_sums_kernel: partials 2 per workgroup
int mle_driver_half_sums(const uint64_t* in, size_t n, uint64_t* partials, unsigned grid, void* stream) {
    if (!in || !partials || !n || !grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(half_sums_kernel, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), in, n, partials);
    return hipGetLastError();
}
// finish_sums_kernel: out 3 entries (lower, upper, total)
int mle_driver_finish_sums(const uint64_t* partials, unsigned n_partials, uint64_t* out, void* stream) {
    if (!partials || !out || !n_partials) return hipErrorInvalidValue;
    hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(MLE_BLOCK), 0, S(stream), partials, n_partials, out);
    return hipGetLastError();
}

// fold_tail_kernel: n <= TAIL_N entries folded with h_pts[first_pt .. first_pt + n_pts); out n >> n_pts entries
int mle_driver_fold_tail(const uint64_t* in, unsigned n, const uint64_t* h_pts, unsigned first_pt, unsigned n_pts, uint64_t* out, void* stream) {
    if (!in || !out || (n_pts && !h_pts) || !pow2(n) || n > (unsigned)TAIL_N || n_pts > log2u(n) || first_pt + n_pts > MAX_POINTS)
        return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute((const void*)fold_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TAIL_LDS_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fold_tail_kernel, dim3(1), dim3(MLE_BLOCK), TAIL_LDS_BYTES, S(stream), in, n, pts_arg(h_pts, first_pt + n_pts), first_pt, n_pts, out);
    return hipGetLastError();
}

// distinct_kernel: out[i * nb + j] = a[i] (+|*) b[j]
int mle_driver_distinct(int mul, const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, unsigned grid, void* stream) {
    if (!a || !b || !out || !na || !nb || !grid_ok(grid)) return hipErrorInvalidValue;
    if (mul)
        hipLaunchKernelGGL(distinct_kernel<true>, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), a, b, nb, na * nb, out);
    else
        hipLaunchKernelGGL(distinct_kernel<false>, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), a, b, nb, na * nb, out);
    return hipGetLastError();
}

// elementwise_kernel: op 0 a + b, 1 a - b, 2 a * h_scalar
int mle_driver_elementwise(int op, const uint64_t* a, const uint64_t* b, const uint64_t* h_scalar, size_t n, uint64_t* out, unsigned grid,
                           void* stream) {
    if (!a || !out || op < 0 || op > 2 || (op == 2 ? !h_scalar : !b) || !n || !grid_ok(grid)) return hipErrorInvalidValue;
    const FrArg sc = fr_arg(op == 2 ? h_scalar : nullptr);
    if (op == 0)
        hipLaunchKernelGGL(elementwise_kernel<0>, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), a, b, sc, n, out);
    else if (op == 1)
        hipLaunchKernelGGL(elementwise_kernel<1>, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), a, b, sc, n, out);
    else
        hipLaunchKernelGGL(elementwise_kernel<2>, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), a, (const uint64_t*)nullptr, sc, n, out);
    return hipGetLastError();
}

// to_bytes_kernel: out 32 n bytes
int mle_driver_to_bytes(const uint64_t* in, size_t n, void* out_bytes, unsigned grid, void* stream) {
    if (!in || !out_bytes || !n || !grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(to_bytes_kernel, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), in, n, (uint32_t*)out_bytes);
    return hipGetLastError();
}

// repeat_kernel: out[i] = in[i mod n_in] (shift 0) or in[i >> shift]; n_in a power of two, n_out within what the form reads
int mle_driver_repeat(const uint64_t* in, size_t n_in, unsigned shift, size_t n_out, uint64_t* out, unsigned grid, void* stream) {
    if (!in || !out || !pow2(n_in) || !n_out || shift > 40 || !grid_ok(grid) || (shift && n_out > (n_in << shift))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(repeat_kernel, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), in, n_in, shift, n_out, out);
    return hipGetLastError();
}

// open_step_kernel: quotient and remainder n / 2 entries each
int mle_driver_open_step(const uint64_t* in, size_t n, const uint64_t* h_z, uint64_t* quotient, uint64_t* remainder, unsigned grid, void* stream) {
    if (!in || !h_z || !quotient || !remainder || !pow2(n) || n < 2 || !grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(open_step_kernel, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), in, n, fr_arg(h_z), quotient, remainder);
    return hipGetLastError();
}
// open_steps_small_kernel: quotients n - (n >> n_rounds) entries in level order; ping n / 2, pong n / 4 entries
int mle_driver_open_steps_small(const uint64_t* in, unsigned n, const uint64_t* h_pts, unsigned n_rounds, uint64_t* quotients, uint64_t* ping,
                                uint64_t* pong, void* stream) {
    if (!in || !h_pts || !quotients || !ping || !pong || !pow2(n) || n < 2 || n > (unsigned)TAIL_N || !n_rounds || n_rounds > log2u(n))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(open_steps_small_kernel, dim3(1), dim3(MLE_BLOCK), 0, S(stream), in, n, pts_arg(h_pts, n_rounds), n_rounds, quotients, ping, pong);
    return hipGetLastError();
}
// open_steps_small_batch_kernel: tables and points on the device, one workgroup per opening; the strides count entries
int mle_driver_open_steps_small_batch(const uint64_t* const* d_tables, unsigned batch, unsigned n, const uint64_t* d_pts, unsigned n_rounds,
                                      uint64_t* quotients, size_t q_stride, uint64_t* ping, size_t ping_stride, uint64_t* pong, size_t pong_stride,
                                      uint64_t* evals, void* stream) {
    if (!d_tables || !d_pts || !quotients || !ping || !pong || !evals || !grid_ok(batch) || !pow2(n) || n < 2 || n > (unsigned)TAIL_N ||
        !n_rounds || n_rounds > log2u(n) || q_stride < n - (n >> n_rounds) || ping_stride < n / 2 || pong_stride < n / 4)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(open_steps_small_batch_kernel, dim3(batch), dim3(MLE_BLOCK), 0, S(stream), d_tables, n, d_pts, n_rounds, quotients, q_stride, ping,
                       ping_stride, pong, pong_stride, evals);
    return hipGetLastError();
}

// DenseUnivariatePolynomial::evaluate as the library launches it: scan<false>, top with v0_out.  block_vals and carries hold one
// entry per block of mle_driver_horner_block() coefficients.
int mle_driver_horner_eval(const uint64_t* coeffs, size_t n, const uint64_t* h_z, uint64_t* block_vals, uint64_t* carries, uint64_t* v0_out,
                           void* stream) {
    if (!coeffs || !h_z || !block_vals || !carries || !v0_out || !n || n >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    const unsigned nb = horner_blocks(n);
    const FrArg z = fr_arg(h_z);
    hipLaunchKernelGGL(horner_scan_kernel<false>, dim3(nb), dim3(HS_T), 0, S(stream), coeffs, n, z, block_vals, (const uint64_t*)nullptr,
                       (uint64_t*)nullptr, (uint64_t*)nullptr);
    hipLaunchKernelGGL(horner_top_kernel, dim3(1), dim3(1024), 0, S(stream), (const uint64_t*)block_vals, nb, z, carries, v0_out);
    return hipGetLastError();
}
// UnivariateKZG::open's scan: scan<false>, top, scan<true>; quotient n - 1 entries (V_1 .. V_{n-1}), evaluation 1 (V_0)
int mle_driver_horner_divide(const uint64_t* coeffs, size_t n, const uint64_t* h_z, uint64_t* block_vals, uint64_t* carries, uint64_t* quotient,
                             uint64_t* evaluation, void* stream) {
    if (!coeffs || !h_z || !block_vals || !carries || !quotient || !evaluation || !n || n >= ((size_t)1 << 31)) return hipErrorInvalidValue;
    const unsigned nb = horner_blocks(n);
    const FrArg z = fr_arg(h_z);
    hipLaunchKernelGGL(horner_scan_kernel<false>, dim3(nb), dim3(HS_T), 0, S(stream), coeffs, n, z, block_vals, (const uint64_t*)nullptr,
                       (uint64_t*)nullptr, (uint64_t*)nullptr);
    hipLaunchKernelGGL(horner_top_kernel, dim3(1), dim3(1024), 0, S(stream), (const uint64_t*)block_vals, nb, z, carries, (uint64_t*)nullptr);
    hipLaunchKernelGGL(horner_scan_kernel<true>, dim3(nb), dim3(HS_T), 0, S(stream), coeffs, n, z, (uint64_t*)nullptr, (const uint64_t*)carries,
                       quotient, evaluation);
    return hipGetLastError();
}

// dense_degree_kernel: the output word is zeroed in front of the launch, as zkhip_dense_degree does
int mle_driver_dense_degree(const uint64_t* coeffs, size_t n, unsigned long long* out, unsigned grid, void* stream) {
    if (!coeffs || !out || !n || !grid_ok(grid)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(out, 0, 8, S(stream));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dense_degree_kernel, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), coeffs, n, out);
    return hipGetLastError();
}

// circuit_layer_kernel: gates 3 words each (type, in0, in1); the CALLER keeps in0, in1 inside `in`
int mle_driver_circuit_layer(const uint64_t* in, const uint32_t* gates, size_t n_gates, uint64_t* out, unsigned grid, void* stream) {
    if (!in || !gates || !out || !n_gates || !grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(circuit_layer_kernel, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), in, gates, n_gates, out);
    return hipGetLastError();
}
// wiring_ones_kernel: add and mul hold n_gates << (2 shift) entries at least and are zeroed by the caller; in0, in1 < 2^shift
int mle_driver_wiring_ones(const uint32_t* gates, size_t n_gates, unsigned shift, uint64_t* add, uint64_t* mul, unsigned grid, void* stream) {
    if (!gates || !add || !mul || !n_gates || shift > 13 || !grid_ok(grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wiring_ones_kernel, dim3(grid), dim3(MLE_BLOCK), 0, S(stream), gates, n_gates, shift, add, mul);
    return hipGetLastError();
}

// eq_weights_kernel: out 2^k weights of h_pts[first .. first + k) (with the factor 2^32)
int mle_driver_eq_weights(const uint64_t* h_pts, unsigned first, unsigned k, uint64_t* out, void* stream) {
    if (!h_pts || !out || !k || k > (unsigned)MF_CAP_LOGK || first + k > MAX_POINTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(eq_weights_kernel, dim3(((1u << k) + MLE_BLOCK - 1) / MLE_BLOCK), dim3(MLE_BLOCK), 0, S(stream), pts_arg(h_pts, first + k), first, k, out);
    return hipGetLastError();
}
// eval_weights_kernel with the grid of zkhip_mle_evaluation: w1 2^k1, wa 2^(k2 - s), wb 2^s entries of h_pts[0 .. k1 + k2)
int mle_driver_eval_weights(const uint64_t* h_pts, unsigned k1, unsigned k2, unsigned s, uint64_t* w1, uint64_t* wa, uint64_t* wb, void* stream) {
    if (!h_pts || !w1 || !wa || !wb || !k1 || k1 > (unsigned)MF_CAP_LOGK || s > k2 || k1 + k2 > MAX_POINTS || k2 - s > 24 || s > 24)
        return hipErrorInvalidValue;
    const size_t lanes = ((size_t)1 << k1) + ((size_t)1 << (k2 - s)) + ((size_t)1 << s);
    hipLaunchKernelGGL(eval_weights_kernel, dim3((unsigned)((lanes + MLE_BLOCK - 1) / MLE_BLOCK)), dim3(MLE_BLOCK), 0, S(stream), pts_arg(h_pts, k1 + k2),
                       k1, k2, s, w1, wa, wb);
    return hipGetLastError();
}
// sum_records_kernel: out[0] = the sum of n records
int mle_driver_sum_records(const uint64_t* records, unsigned n, uint64_t* out, void* stream) {
    if (!records || !out || !n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sum_records_kernel, dim3(1), dim3(MLE_BLOCK), 0, S(stream), records, n, out);
    return hipGetLastError();
}

}  // extern "C"
