// arith_driver.hip -- test-only launchers for the arithmetic layer under every kernel (tests/test_gpu_arith.py): the saturated fields
// of csrc/fp.hpp, the unsaturated FqU of fqu.hpp, the XYZZ group law of g1u.hpp, the unreduced accumulator of wide_acc.hpp, the DPP
// reductions of fp.hpp and the matrix-core fold of mfma_fold.hpp.
//
// One kernel per primitive, one work item per lane: raw limbs in, raw limbs out, and no conversion that the primitive under test would
// also perform.  Layouts are those of the headers: Fr 8 x u32, Fq 12 x u32, FqU 16 x u32 (14 limbs + 2 pad), affine 2 FqU, XYZZ 4 FqU.
// A launcher returns hipGetLastError(), or hipErrorInvalidValue WITHOUT launching for a null pointer, a zero count, an unknown
// operation or a size beyond what a test asks for.  Nothing of libzkhip is linked: the headers alone.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../zk-cryptography_amd/csrc/g1u.hpp"
#include "../../zk-cryptography_amd/csrc/mfma_fold.hpp"

using namespace zk;

namespace {

constexpr size_t MAX_ITEMS = (size_t)1 << 20;      // far above any count a test asks for; keeps a wrong argument from a huge launch
constexpr unsigned BLOCK = 256;
inline hipStream_t st(void* s) { return (hipStream_t)s; }
inline bool bad_count(size_t n) { return n == 0 || n > MAX_ITEMS; }
inline unsigned grid_of(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

enum FpOp { FP_ADD, FP_SUB, FP_MUL, FP_SQR, FP_NEG, FP_DBL, FP_TO_MONT, FP_FROM_MONT, FP_OPS };
enum FquOp { FQU_FROM_ARK, FQU_TO_ARK, FQU_MUL, FQU_WEAK_NORM, FQU_STRONG_NORM, FQU_SUB4, FQU_SUB8, FQU_SUB16, FQU_SUB8_DBL, FQU_IS_ZERO, FQU_OPS };
enum G1uOp { G1U_DOUBLE_AFFINE, G1U_DOUBLE, G1U_MADD, G1U_MADD_NEG, G1U_ADD, G1U_ADD_QUAD, G1U_OPS };
enum RedOp { RED_WAVE, RED_WAVE2, RED_BLOCK, RED_BLOCK2, RED_OPS };

template <class F>
__device__ __forceinline__ F load_fp(const uint32_t* p, size_t i) {
    F r;
#pragma unroll
    for (int j = 0; j < F::N; ++j) r.l[j] = p[F::N * i + j];
    return r;
}
template <class F>
__device__ __forceinline__ void store_fp(uint32_t* p, size_t i, const F& v) {
#pragma unroll
    for (int j = 0; j < F::N; ++j) p[F::N * i + j] = v.l[j];
}

template <class F, int OP>
__global__ __launch_bounds__(BLOCK) void fp_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const F x = load_fp<F>(a, i);
    F r;
    if constexpr (OP == FP_ADD) r = x + load_fp<F>(b, i);
    else if constexpr (OP == FP_SUB) r = x - load_fp<F>(b, i);
    else if constexpr (OP == FP_MUL) r = x * load_fp<F>(b, i);
    else if constexpr (OP == FP_SQR) r = x.sqr();
    else if constexpr (OP == FP_NEG) r = x.neg();
    else if constexpr (OP == FP_DBL) r = x.dbl();
    else if constexpr (OP == FP_TO_MONT) r = x.to_mont();
    else r = x.from_mont();
    store_fp<F>(out, i, r);
}

template <class F, int OP>
int launch_fp(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL((fp_kernel<F, OP>), dim3(grid_of(n)), dim3(BLOCK), 0, s, a, b, out, n);
    return hipGetLastError();
}
template <class F>
int dispatch_fp(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    switch (op) {
        case FP_ADD: return launch_fp<F, FP_ADD>(a, b, out, n, s);
        case FP_SUB: return launch_fp<F, FP_SUB>(a, b, out, n, s);
        case FP_MUL: return launch_fp<F, FP_MUL>(a, b, out, n, s);
        case FP_SQR: return launch_fp<F, FP_SQR>(a, b, out, n, s);
        case FP_NEG: return launch_fp<F, FP_NEG>(a, b, out, n, s);
        case FP_DBL: return launch_fp<F, FP_DBL>(a, b, out, n, s);
        case FP_TO_MONT: return launch_fp<F, FP_TO_MONT>(a, b, out, n, s);
        default: return launch_fp<F, FP_FROM_MONT>(a, b, out, n, s);
    }
}

// out: 16 u32 per item, but 12 for FQU_TO_ARK and 1 (0 / 1) for FQU_IS_ZERO; a: 12 u32 per item for FQU_FROM_ARK
template <int OP>
__global__ __launch_bounds__(BLOCK) void fqu_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if constexpr (OP == FQU_FROM_ARK) {
        store_fqu(out + 16 * i, fqu_from_ark(load_fp<Fq>(a, i)));
    } else if constexpr (OP == FQU_TO_ARK) {
        store_fp<Fq>(out, i, fqu_to_ark(load_fqu(a + 16 * i)));
    } else if constexpr (OP == FQU_IS_ZERO) {
        out[i] = fqu_is_zero_mod_p(load_fqu(a + 16 * i)) ? 1u : 0u;
    } else {
        const FqU x = load_fqu(a + 16 * i);
        FqU r;
        if constexpr (OP == FQU_MUL) r = fqu_mul(x, load_fqu(b + 16 * i));
        else if constexpr (OP == FQU_WEAK_NORM) r = fqu_weak_norm(x);
        else if constexpr (OP == FQU_STRONG_NORM) r = fqu_strong_norm(x);
        else if constexpr (OP == FQU_SUB4) r = fqu_sub<4>(x, load_fqu(b + 16 * i));
        else if constexpr (OP == FQU_SUB8) r = fqu_sub<8>(x, load_fqu(b + 16 * i));
        else if constexpr (OP == FQU_SUB16) r = fqu_sub<16>(x, load_fqu(b + 16 * i));
        else r = fqu_sub<8>(x, fqu_dbl(load_fqu(b + 16 * i)));       // the shape g1u_double / g1u_madd / g1u_add pass
        store_fqu(out + 16 * i, r);
    }
}
template <int OP>
int launch_fqu(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL((fqu_kernel<OP>), dim3(grid_of(n)), dim3(BLOCK), 0, s, a, b, out, n);
    return hipGetLastError();
}

// a: XYZZ (affine for G1U_DOUBLE_AFFINE), b: XYZZ (affine for the madd forms), out: XYZZ.  G1U_ADD_QUAD: n is a multiple of 64 and
// every lane of a wave calls; the caller gives the four lanes of a quad the same pair.
template <int OP>
__global__ __launch_bounds__(64) void g1u_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    G1XyzzU r;
    if constexpr (OP == G1U_DOUBLE_AFFINE) r = g1u_double_affine(load_affine_u(a, i));
    else if constexpr (OP == G1U_DOUBLE) r = g1u_double(load_xyzz_u(a, i));
    else if constexpr (OP == G1U_MADD || OP == G1U_MADD_NEG) { r = load_xyzz_u(a, i); g1u_madd(r, load_affine_u(b, i), OP == G1U_MADD_NEG); }
    else if constexpr (OP == G1U_ADD) { r = load_xyzz_u(a, i); g1u_add(r, load_xyzz_u(b, i)); }
    else r = g1u_add_quad(load_xyzz_u(a, i), load_xyzz_u(b, i));
    store_xyzz_u(out, i, r);
}
template <int OP>
int launch_g1u(const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL((g1u_kernel<OP>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, a, b, out, n);
    return hipGetLastError();
}

// lane i: sum over j < terms of w[j * lanes + i] * t[j * lanes + i], unreduced, then wide_reduce
__global__ __launch_bounds__(64) void wide_mac_kernel(const uint64_t* __restrict__ w, const uint64_t* __restrict__ t, size_t lanes, uint32_t terms,
                                                      uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= lanes) return;
    WideAcc acc;
    acc.clear();
    for (uint32_t j = 0; j < terms; ++j) acc.mac(load_fr(w, (size_t)j * lanes + i), load_fr(t, (size_t)j * lanes + i));
    store_fr(out, i, wide_reduce(acc.lo, acc.hi));
}
// x: 17 u32 per item
__global__ __launch_bounds__(64) void wide_redc_kernel(const uint32_t* __restrict__ x_in, size_t n, uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    uint32_t x[18];
#pragma unroll
    for (int j = 0; j < 17; ++j) x[j] = x_in[17 * i + j];
    x[17] = 0;
    store_fr(out, i, wide_redc(x));
}

// every thread writes what the reduction returned to it: item blockIdx.x * blockDim.x + threadIdx.x of out_a (and out_b)
template <int OP>
__global__ __launch_bounds__(1024) void reduce_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint64_t* __restrict__ out_a,
                                                      uint64_t* __restrict__ out_b) {
    __shared__ Fr smem[2 * 16];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    Fr x = load_fr(a, i);
    if constexpr (OP == RED_WAVE) {
        store_fr(out_a, i, wave_reduce_fr(x));
    } else if constexpr (OP == RED_BLOCK) {
        store_fr(out_a, i, block_reduce_fr(x, smem));
    } else {
        Fr y = load_fr(b, i);
        if constexpr (OP == RED_WAVE2) wave_reduce_fr2(x, y);
        else block_reduce_fr2(x, y, smem);
        store_fr(out_a, i, x);
        store_fr(out_b, i, y);
    }
}
template <int OP>
int launch_reduce(const uint64_t* a, const uint64_t* b, uint64_t* out_a, uint64_t* out_b, unsigned block, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL((reduce_kernel<OP>), dim3(grid), dim3(block), 0, s, a, b, out_a, out_b);
    return hipGetLastError();
}

inline bool bad_fold(size_t m, unsigned k, unsigned rot) { return m == 0 || m % 256 != 0 || m > 65536 || k < 3 || k > 8 || rot > 15; }

}  // namespace

extern "C" {

int arith_driver_op_count(int family) { return family == 0 ? FP_OPS : family == 1 ? FQU_OPS : family == 2 ? G1U_OPS : family == 3 ? RED_OPS : -1; }

// field: 0 = Fr (8 u32 per element), 1 = Fq (12); b may be null for the unary operations
int arith_driver_fp(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, void* stream) {
    if (!a || !out || bad_count(n) || op < 0 || op >= FP_OPS || (field != 0 && field != 1)) return hipErrorInvalidValue;
    if (op <= FP_MUL && !b) return hipErrorInvalidValue;
    return field == 0 ? dispatch_fp<Fr>(op, a, b, out, n, st(stream)) : dispatch_fp<Fq>(op, a, b, out, n, st(stream));
}

int arith_driver_fqu(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, void* stream) {
    if (!a || !out || bad_count(n) || op < 0 || op >= FQU_OPS) return hipErrorInvalidValue;
    const bool binary = op == FQU_MUL || op == FQU_SUB4 || op == FQU_SUB8 || op == FQU_SUB16 || op == FQU_SUB8_DBL;
    if (binary && !b) return hipErrorInvalidValue;
    switch (op) {
        case FQU_FROM_ARK: return launch_fqu<FQU_FROM_ARK>(a, b, out, n, st(stream));
        case FQU_TO_ARK: return launch_fqu<FQU_TO_ARK>(a, b, out, n, st(stream));
        case FQU_MUL: return launch_fqu<FQU_MUL>(a, b, out, n, st(stream));
        case FQU_WEAK_NORM: return launch_fqu<FQU_WEAK_NORM>(a, b, out, n, st(stream));
        case FQU_STRONG_NORM: return launch_fqu<FQU_STRONG_NORM>(a, b, out, n, st(stream));
        case FQU_SUB4: return launch_fqu<FQU_SUB4>(a, b, out, n, st(stream));
        case FQU_SUB8: return launch_fqu<FQU_SUB8>(a, b, out, n, st(stream));
        case FQU_SUB16: return launch_fqu<FQU_SUB16>(a, b, out, n, st(stream));
        case FQU_SUB8_DBL: return launch_fqu<FQU_SUB8_DBL>(a, b, out, n, st(stream));
        default: return launch_fqu<FQU_IS_ZERO>(a, b, out, n, st(stream));
    }
}

int arith_driver_g1u(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n, void* stream) {
    if (!a || !out || bad_count(n) || op < 0 || op >= G1U_OPS) return hipErrorInvalidValue;
    if (op >= G1U_MADD && !b) return hipErrorInvalidValue;
    if (op == G1U_ADD_QUAD && n % 64 != 0) return hipErrorInvalidValue;
    switch (op) {
        case G1U_DOUBLE_AFFINE: return launch_g1u<G1U_DOUBLE_AFFINE>(a, b, out, n, st(stream));
        case G1U_DOUBLE: return launch_g1u<G1U_DOUBLE>(a, b, out, n, st(stream));
        case G1U_MADD: return launch_g1u<G1U_MADD>(a, b, out, n, st(stream));
        case G1U_MADD_NEG: return launch_g1u<G1U_MADD_NEG>(a, b, out, n, st(stream));
        case G1U_ADD: return launch_g1u<G1U_ADD>(a, b, out, n, st(stream));
        default: return launch_g1u<G1U_ADD_QUAD>(a, b, out, n, st(stream));
    }
}

// w, t: terms * lanes elements (term-major); out: lanes.  terms <= 1024: the accumulator's bound, x < 2^520
int arith_driver_wide_mac(const uint64_t* w, const uint64_t* t, size_t lanes, unsigned terms, uint64_t* out, void* stream) {
    if (!w || !t || !out || bad_count(lanes) || terms == 0 || terms > 1024 || lanes * terms > MAX_ITEMS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_mac_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st(stream), w, t, lanes, (uint32_t)terms, out);
    return hipGetLastError();
}
int arith_driver_wide_redc(const uint32_t* x, size_t n, uint64_t* out, void* stream) {
    if (!x || !out || bad_count(n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_redc_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st(stream), x, n, out);
    return hipGetLastError();
}

// a, b, out_a, out_b: grid * block elements (b and out_b for the two-sum forms only); block a multiple of 64, at most 1024
int arith_driver_reduce(int op, const uint64_t* a, const uint64_t* b, uint64_t* out_a, uint64_t* out_b, unsigned block, unsigned grid, void* stream) {
    if (!a || !out_a || op < 0 || op >= RED_OPS || block == 0 || block % 64 != 0 || block > 1024 || grid == 0 || grid > 4096) return hipErrorInvalidValue;
    const bool two = op == RED_WAVE2 || op == RED_BLOCK2;
    if (two && (!b || !out_b)) return hipErrorInvalidValue;
    switch (op) {
        case RED_WAVE: return launch_reduce<RED_WAVE>(a, b, out_a, out_b, block, grid, st(stream));
        case RED_WAVE2: return launch_reduce<RED_WAVE2>(a, b, out_a, out_b, block, grid, st(stream));
        case RED_BLOCK: return launch_reduce<RED_BLOCK>(a, b, out_a, out_b, block, grid, st(stream));
        default: return launch_reduce<RED_BLOCK2>(a, b, out_a, out_b, block, grid, st(stream));
    }
}

// multifold_mfma_kernel<4, 4>: in 2^k * m elements, weights 2^k, out m, partials m / 64; m a multiple of 256 (one workgroup = four tiles)
int arith_driver_mfma_fold(const uint64_t* in, size_t m, unsigned k, const uint64_t* weights, uint64_t* out, uint64_t* partials, unsigned rot,
                           void* stream) {
    if (!in || !weights || !out || !partials || bad_fold(m, k, rot)) return hipErrorInvalidValue;
    const size_t q_bytes = mfm_lds_bytes(std::min<uint32_t>(1u << k, (uint32_t)MFM_CHUNK));
    hipLaunchKernelGGL((multifold_mfma_kernel<4, 4>), dim3((unsigned)(m / 256)), dim3(256), q_bytes, st(stream), in, m, (uint32_t)k, weights, out,
                       partials, (uint32_t)rot);
    return hipGetLastError();
}
// multifold_mfma_kernel<4, 4, true>: records m / 64; wa: m >> out_s elements, wb: 2^out_s
int arith_driver_mfma_fold_wsum(const uint64_t* in, size_t m, unsigned k, const uint64_t* weights, uint64_t* records, unsigned rot,
                                const uint64_t* wa, const uint64_t* wb, unsigned out_s, void* stream) {
    if (!in || !weights || !records || !wa || !wb || bad_fold(m, k, rot) || out_s > 16 || ((size_t)1 << out_s) > m) return hipErrorInvalidValue;
    const size_t q_bytes = mfm_lds_bytes(std::min<uint32_t>(1u << k, (uint32_t)MFM_CHUNK));
    hipLaunchKernelGGL((multifold_mfma_kernel<4, 4, true>), dim3((unsigned)(m / 256)), dim3(256), q_bytes, st(stream), in, m, (uint32_t)k, weights,
                       (uint64_t*)nullptr, records, (uint32_t)rot, wa, wb, (uint32_t)out_s);
    return hipGetLastError();
}

}  // extern "C"
