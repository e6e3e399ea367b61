// dense_points_kernels.hpp -- the kernels of zkhip_dense_points (ntt.hip) for gfx950: a polynomial at many points, and the polynomial
// through many points.  The plan -- segments, chunks of jobs, scratch layout -- is dense_points_plan.hpp; the algorithm is described there.
//
// Every O(inner x points) loop is private to a lane: a workgroup of DP_LANES lanes owns DP_LANES points, stages DP_CHUNK inner
// elements in LDS at a time, and all lanes of a wave read the same LDS address in the same step (a broadcast, no bank conflict).
// The loops issue one to three Montgomery products per (inner element, point) and nothing else of weight.  No lane reads what another
// lane of the same launch wrote to global memory: records cross launches only.
//
//   dp_eval_kernel<RECORD>       Horner over a segment of the coefficients, top down; RECORD: times x^(first coefficient), to a record
//   dp_eval_sum_kernel           adds a point's S records
//   dp_weights_kernel<RECORD>    D_i = prod_{j != i} (x_i - x_j) over a segment of the nodes; !RECORD: the flag and 1 / D_i
//   dp_weights_fold_kernel       multiplies a node's S partial products; the flag and 1 / D_i
//   dp_domain_kernel<RECORD>     (Num, Den) over a segment of the nodes at z = w^t; !RECORD: Num = P(w^t)
//   dp_domain_fold_kernel        combines a domain point's S (Num, Den) records
// Grids are (min(point blocks, DP_MAX_GRID_X), segments, jobs); a workgroup strides over the point blocks beyond its grid.
#pragma once
#include "dense_points_plan.hpp"
#include "fp.hpp"
#include "mle_kernels.hpp"
#include "plonk_kernels.hpp"      // fr_inverse

namespace zk {

// x^e by squaring; e is the same in every lane of a workgroup
__device__ __forceinline__ Fr dp_pow(const Fr& x, size_t e) {
    Fr acc = Fr::one(), sq = x;
    for (; e; e >>= 1) {
        if (e & 1) acc = acc * sq;
        sq = sq * sq;
    }
    return acc;
}

// 1 / d, and the call's flag when d == 0: a plain store of 1 from the lane that met it (the Fermat inverse of zero is zero)
__device__ __forceinline__ Fr dp_invert(const Fr& d, uint32_t* __restrict__ flag) {
    if (d.is_zero()) *flag = 1u;
    return fr_inverse(d);
}

// coefficients [lo, hi) of job blockIdx.z at the job's points; records[(job * S + seg) * n_x + p] with RECORD, out + 4 job out_stride else
template <bool RECORD>
static __global__ __launch_bounds__(DP_LANES) void dp_eval_kernel(const uint64_t* __restrict__ coeffs, size_t in_stride, size_t n_in,
                                                                 const uint64_t* __restrict__ xs, size_t x_stride, size_t n_x,
                                                                 uint64_t* __restrict__ out, size_t out_stride, size_t seg_len) {
    __shared__ __attribute__((aligned(16))) Fr sh[DP_CHUNK];
    const size_t job = blockIdx.z, seg = blockIdx.y;
    const uint64_t* c = coeffs + 4 * job * in_stride;
    const uint64_t* x = xs + 4 * job * x_stride;
    const size_t lo = min(seg * seg_len, n_in), hi = min(lo + seg_len, n_in);
    uint64_t* dst = RECORD ? out + 4 * (job * gridDim.y + seg) * n_x : out + 4 * job * out_stride;
    const size_t blocks = (n_x + DP_LANES - 1) / DP_LANES;
    for (size_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const size_t p = blk * DP_LANES + threadIdx.x;
        const Fr X = p < n_x ? load_fr(x, p) : Fr::zero();
        Fr acc = Fr::zero();
        for (size_t top = hi; top > lo;) {
            const uint32_t cnt = (uint32_t)min((size_t)DP_CHUNK, top - lo);
            const size_t base = top - cnt;
            __syncthreads();                                      // the chunk before has been read
            if (threadIdx.x < cnt) sh[threadIdx.x] = load_fr(c, base + threadIdx.x);
            __syncthreads();
            for (uint32_t k = cnt; k-- > 0;) acc = acc * X + sh[k];
            top = base;
        }
        if (RECORD) acc = acc * dp_pow(X, lo);
        if (p < n_x) store_fr(dst, p, acc);
    }
}

// out[job][p] = sum over s of records[(job * S + s) * n_x + p]
static __global__ __launch_bounds__(DP_LANES) void dp_eval_sum_kernel(const uint64_t* __restrict__ records, uint32_t segs, size_t n_x,
                                                                     uint64_t* __restrict__ out, size_t out_stride) {
    const size_t job = blockIdx.z;
    const size_t blocks = (n_x + DP_LANES - 1) / DP_LANES;
    for (size_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
        const size_t p = blk * DP_LANES + threadIdx.x;
        if (p >= n_x) continue;
        Fr acc = load_fr(records, job * segs * n_x + p);
        for (uint32_t s = 1; s < segs; ++s) acc = acc + load_fr(records, (job * segs + s) * n_x + p);
        store_fr(out + 4 * job * out_stride, p, acc);
    }
}

// row blockIdx.z of the node sets (x_stride == 0: the one shared set).  RECORD: out = records[(row * S + seg) * n + i]; else out =
// winv[row * n + i] = 1 / D_i.  n <= 2^14: one point block per blockIdx.x.
template <bool RECORD>
static __global__ __launch_bounds__(DP_LANES) void dp_weights_kernel(const uint64_t* __restrict__ xs, size_t x_stride, uint32_t n, uint32_t seg_len,
                                                                    uint64_t* __restrict__ out, uint32_t* __restrict__ flag) {
    __shared__ __attribute__((aligned(16))) Fr sh[DP_CHUNK];
    const size_t row = blockIdx.z;
    const uint32_t seg = blockIdx.y;
    const uint64_t* x = xs + 4 * row * x_stride;
    const uint32_t lo = min(seg * seg_len, n), hi = min(lo + seg_len, n);
    const uint32_t i = blockIdx.x * DP_LANES + threadIdx.x;
    const Fr X = i < n ? load_fr(x, i) : Fr::zero();
    Fr acc = Fr::one();
    for (uint32_t base = lo; base < hi; base += DP_CHUNK) {
        const uint32_t cnt = min((uint32_t)DP_CHUNK, hi - base);
        __syncthreads();
        if (threadIdx.x < cnt) sh[threadIdx.x] = load_fr(x, base + threadIdx.x);
        __syncthreads();
        for (uint32_t k = 0; k < cnt; ++k) {
            const Fr d = X - sh[k];
            acc = acc * (base + k == i ? Fr::one() : d);
        }
    }
    if (i >= n) return;
    if (RECORD) store_fr(out, ((size_t)row * gridDim.y + seg) * n + i, acc);
    else store_fr(out, (size_t)row * n + i, dp_invert(acc, flag));
}

static __global__ __launch_bounds__(DP_LANES) void dp_weights_fold_kernel(const uint64_t* __restrict__ records, uint32_t segs, uint32_t n,
                                                                         uint64_t* __restrict__ winv, uint32_t* __restrict__ flag) {
    const size_t row = blockIdx.z;
    const uint32_t i = blockIdx.x * DP_LANES + threadIdx.x;
    if (i >= n) return;
    Fr acc = load_fr(records, row * segs * n + i);
    for (uint32_t s = 1; s < segs; ++s) acc = acc * load_fr(records, (row * segs + s) * n + i);
    store_fr(winv, row * n + i, dp_invert(acc, flag));
}

// job blockIdx.z at z = w^t, t = blockIdx.x * DP_LANES + lane < N, over the nodes [lo, hi) of segment blockIdx.y.  The workgroup stages
// x_i and s_i = y_i / D_i.  RECORD: out = records, (Num, Den) at 2 * ((job * S + seg) * N + t); else out = vals[job * N + t] = Num.
template <bool RECORD>
static __global__ __launch_bounds__(DP_LANES) void dp_domain_kernel(const uint64_t* __restrict__ ys, size_t y_stride, const uint64_t* __restrict__ xs,
                                                                   size_t x_stride, const uint64_t* __restrict__ winv, size_t w_stride, uint32_t n,
                                                                   uint32_t N, uint32_t seg_len, FrArg omega, uint64_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) Fr sh_x[DP_CHUNK];
    __shared__ __attribute__((aligned(16))) Fr sh_s[DP_CHUNK];
    const size_t job = blockIdx.z;
    const uint32_t seg = blockIdx.y;
    const uint64_t* y = ys + 4 * job * y_stride;
    const uint64_t* x = xs + 4 * job * x_stride;
    const uint64_t* w = winv + 4 * job * w_stride;
    const uint32_t lo = min(seg * seg_len, n), hi = min(lo + seg_len, n);
    const uint32_t t = blockIdx.x * DP_LANES + threadIdx.x;
    const Fr z = dp_pow(fr_from_arg(omega), t < N ? t : 0);
    Fr num = Fr::zero(), den = Fr::one();
    for (uint32_t base = lo; base < hi; base += DP_CHUNK) {
        const uint32_t cnt = min((uint32_t)DP_CHUNK, hi - base);
        __syncthreads();
        if (threadIdx.x < cnt) {
            sh_x[threadIdx.x] = load_fr(x, base + threadIdx.x);
            sh_s[threadIdx.x] = load_fr(y, base + threadIdx.x) * load_fr(w, base + threadIdx.x);
        }
        __syncthreads();
        for (uint32_t k = 0; k < cnt; ++k) {
            const Fr d = z - sh_x[k];
            num = num * d + sh_s[k] * den;
            den = den * d;
        }
    }
    if (t >= N) return;
    if (RECORD) {
        const size_t at = 2 * (((size_t)job * gridDim.y + seg) * N + t);
        store_fr(out, at, num);
        store_fr(out, at + 1, den);
    } else {
        store_fr(out, (size_t)job * N + t, num);
    }
}

// segments A then B: (Num_A Den_B + Num_B Den_A, Den_A Den_B); the last segment's product of denominators is not needed
static __global__ __launch_bounds__(DP_LANES) void dp_domain_fold_kernel(const uint64_t* __restrict__ records, uint32_t segs, uint32_t N,
                                                                        uint64_t* __restrict__ vals) {
    const size_t job = blockIdx.z;
    const uint32_t t = blockIdx.x * DP_LANES + threadIdx.x;
    if (t >= N) return;
    Fr num = load_fr(records, 2 * (job * segs * N + t)), den = load_fr(records, 2 * (job * segs * N + t) + 1);
    for (uint32_t s = 1; s < segs; ++s) {
        const size_t at = 2 * ((job * segs + s) * N + t);
        const Fr nb = load_fr(records, at), db = load_fr(records, at + 1);
        num = num * db + nb * den;
        if (s + 1 < segs) den = den * db;
    }
    store_fr(vals, job * N + t, num);
}

}  // namespace zk
