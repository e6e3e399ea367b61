// ntt.hip -- C-ABI entry points of the NTT / Domain / polynomial product path.
// gfx950 only.  No CPU fallback: every entry point launches HIP kernels or fails.
#include "../../include/zkhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <new>
#include <vector>

#include "ctx.hpp"
#include "dense_points_kernels.hpp"
#include "host_fr.hpp"
#include "host_util.hpp"
#include "ntt_batch_kernels.hpp"
#include "ntt_kernels.hpp"

using namespace zk;

// F::get_root_of_unity(2^log_n) (domain.rs:38): the 2^32-th root 7^((r-1)/2^32), squared (32 - log_n) times
static zkhost::Fr root_of_unity(uint32_t log_n) {
    zkhost::Fr g = zkhost::fr_from_u64(7);
    uint64_t e[4];
    uint64_t rm1[4] = {zkhost::FR_P[0] - 1, zkhost::FR_P[1], zkhost::FR_P[2], zkhost::FR_P[3]};
    for (int i = 0; i < 4; ++i) e[i] = (rm1[i] >> 32) | (i < 3 ? (rm1[i + 1] << 32) : 0);
    zkhost::Fr w = zkhost::fr_one();
    for (int i = 255; i >= 0; --i) {
        w = zkhost::fr_mul(w, w);
        if ((e[i / 64] >> (i % 64)) & 1) w = zkhost::fr_mul(w, g);
    }
    for (uint32_t i = log_n; i < 32; ++i) w = zkhost::fr_mul(w, w);
    return w;
}

extern "C" int zkhip_domain_params(uint64_t size, uint64_t* h_generator, uint64_t* h_generator_inv, uint64_t* h_size_inv) {
    if (!is_pow2((size_t)size) || !h_generator || !h_generator_inv || !h_size_inv) return ZKHIP_ERR_ARG;
    const uint32_t log_n = log2_exact((size_t)size);
    if (log_n > 32) return ZKHIP_ERR_SHAPE;   // get_root_of_unity(..).unwrap() panics beyond the 2-adicity
    zkhost::Fr w = root_of_unity(log_n);
    zkhost::Fr wi = zkhost::fr_inv(w);
    zkhost::Fr ni = zkhost::fr_inv(zkhost::fr_from_u64(size));
    std::memcpy(h_generator, w.l, 32);
    std::memcpy(h_generator_inv, wi.l, 32);
    std::memcpy(h_size_inv, ni.l, 32);
    return ZKHIP_OK;
}

// Twiddle tables and pass plans live in the CONTEXT that built them (zkhip_ctx::ntt_state): contexts on different host threads share
// nothing, and zkhip_ctx_destroy returns their device memory (they used to be process-wide maps keyed by the context's address).
struct TwiddleKey {
    uint32_t log_n; int inverse;
    bool operator<(const TwiddleKey& o) const {
        if (log_n != o.log_n) return log_n < o.log_n;
        return inverse < o.inverse;
    }
};
struct NttPass { uint32_t s0, T; DevMem table; };
struct NttPlan { DevMem tw1; std::vector<NttPass> passes; zkhost::Fr n_inv; };
struct NttCache {
    std::map<TwiddleKey, DevMem> twiddles;
    std::map<TwiddleKey, NttPlan> plans;
};
void NttCacheDelete::operator()(NttCache* nc) const { delete nc; }
static NttCache* ntt_cache(zkhip_ctx* c) {
    if (!c->ntt_state) c->ntt_state.reset(new (std::nothrow) NttCache());
    return c->ntt_state.get();
}

static int get_twiddles(zkhip_ctx* c, uint32_t log_n, int inverse, uint64_t** out) {
    NttCache* nc = ntt_cache(c);
    if (!nc) return ZKHIP_ERR_NOMEM;
    TwiddleKey key{log_n, inverse};
    auto it = nc->twiddles.find(key);
    if (it != nc->twiddles.end()) { *out = (uint64_t*)it->second.get(); return ZKHIP_OK; }
    const uint32_t log_half = log_n ? log_n - 1 : 0;
    const size_t half = (size_t)1 << log_half;
    zkhost::Fr w = root_of_unity(log_n);
    if (inverse) w = zkhost::fr_inv(w);
    std::vector<zkhost::Fr> pw(log_half ? log_half : 1);
    for (uint32_t k = 0; k < log_half; ++k) { pw[k] = w; w = zkhost::fr_mul(w, w); }
    DevMem tab, powers;                             // built here, kept only when everything below went through
    ZK_HIP(c, dev_alloc(tab, half * 32));
    ZK_HIP(c, dev_alloc(powers, pw.size() * 32));
    uint64_t *d_tab = (uint64_t*)tab.get(), *d_pw = (uint64_t*)powers.get();
    ZK_HIP(c, hipMemcpyAsync(d_pw, pw.data(), pw.size() * 32, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(ntt_twiddle_kernel, dim3(mle_grid(half)), dim3(MLE_BLOCK), 0, c->stream, d_pw, log_half, d_tab);
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    nc->twiddles[key] = std::move(tab);
    *out = d_tab;
    return ZKHIP_OK;
}

// ---- transforms of >= 2^12 points (ntt_kernels.hpp, second half) ------------------------------------------------------------
static int get_plan(zkhip_ctx* c, uint32_t log_n, int inverse, NttPlan** out) {
    NttCache* nc = ntt_cache(c);
    if (!nc) return ZKHIP_ERR_NOMEM;
    TwiddleKey key{log_n, inverse};
    auto it = nc->plans.find(key);
    if (it != nc->plans.end()) { *out = &it->second; return ZKHIP_OK; }
    uint64_t* W = nullptr;
    ZK_TRY(get_twiddles(c, log_n, inverse, &W));
    NttPlan plan;
    plan.n_inv = zkhost::fr_inv(zkhost::fr_from_u64((uint64_t)1 << log_n));
    ZK_HIP(c, dev_alloc(plan.tw1, 256 * 32));
    hipLaunchKernelGGL(ntt_first_table_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, W, log_n, (uint64_t*)plan.tw1.get());
    // the stages after the first eight, in passes of <= 7 spread evenly
    const uint32_t rest = log_n - NTT_FIRST_STAGES;
    const uint32_t n_pass = (rest + 6) / 7;
    uint32_t s0 = NTT_FIRST_STAGES;
    for (uint32_t p = 0; p < n_pass; ++p) {
        const uint32_t T = (rest - (s0 - NTT_FIRST_STAGES) + (n_pass - p) - 1) / (n_pass - p);
        NttPass ps{s0, T, nullptr};
        const size_t entries = (((size_t)1 << T) - 1) << s0;
        ZK_HIP(c, dev_alloc(ps.table, entries * 32));
        FrArg sc = {};
        const bool scaled = inverse && p + 1 == n_pass;
        if (scaled) std::memcpy(sc.v, plan.n_inv.l, 32);
        hipLaunchKernelGGL(ntt_pass_table_kernel, dim3(mle_grid_stream(entries)), dim3(MLE_BLOCK), 0, c->stream, W, log_n, s0, T, sc,
                           scaled ? 1u : 0u, (uint64_t*)ps.table.get());
        plan.passes.push_back(std::move(ps));
        s0 += T;
    }
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    *out = &(nc->plans[key] = std::move(plan));
    return ZKHIP_OK;
}

// src (n_src <= n elements, zero-padded; times src2 element-wise when given) -> dst (the first n_dst <= n outputs), which may
// be src itself; d_scratch: n elements.  The last pass writes dst, every earlier one d_scratch.
static int ntt_big(zkhip_ctx* c, const uint64_t* d_src, size_t n_src, const uint64_t* d_src2, uint64_t* d_dst, size_t n_dst,
                   uint32_t log_n, int inverse, uint64_t* d_scratch) {
    const size_t n = (size_t)1 << log_n;
    NttPlan* plan = nullptr;
    ZK_TRY(get_plan(c, log_n, inverse, &plan));
    const size_t lds = (size_t)NTT_BIG_TILE * 32;
    const unsigned grid = (unsigned)(n >> NTT_BIG_TILE_LOG);
    {
        ProfScope ps(c, "ntt_first8", 32.0 * (double)(n_src + n) + (d_src2 ? 32.0 * (double)n : 0.0));
        hipLaunchKernelGGL(ntt_first8_kernel, dim3(grid), dim3(NTT_BIG_BLOCK), lds, c->stream, d_src, n_src, d_src2, d_scratch, log_n, (const uint64_t*)plan->tw1.get());
    }
    FrArg sc = {};
    std::memcpy(sc.v, plan->n_inv.l, 32);
    for (size_t p = 0; p < plan->passes.size(); ++p) {
        const NttPass& ps = plan->passes[p];
        const bool last = p + 1 == plan->passes.size();
        ProfScope pr(c, "ntt_pass", 32.0 * (double)(n + (last ? n_dst : n)) + 32.0 * (double)((((size_t)1 << ps.T) - 1) << ps.s0));
        if (last && inverse)
            hipLaunchKernelGGL(ntt_pass_kernel<true>, dim3(grid), dim3(NTT_BIG_BLOCK), lds, c->stream, d_scratch, d_dst, ps.s0, ps.T, (const uint64_t*)ps.table.get(), sc, n_dst);
        else
            hipLaunchKernelGGL(ntt_pass_kernel<false>, dim3(grid), dim3(NTT_BIG_BLOCK), lds, c->stream, d_scratch, last ? d_dst : d_scratch, ps.s0, ps.T,
                               (const uint64_t*)ps.table.get(), sc, last ? n_dst : n);
    }
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// d_data (n = 2^log_n, in place).  Forward: serial_fft with omega; inverse: omega^-1 then scale by n^-1.
static int ntt_inplace(zkhip_ctx* c, uint64_t* d_data, uint32_t log_n, int inverse, uint64_t* d_scratch) {
    const size_t n = (size_t)1 << log_n;
    if (log_n == 0) return ZKHIP_OK;
    if (log_n >= 12) return ntt_big(c, d_data, n, nullptr, d_data, n, log_n, inverse, d_scratch);
    uint64_t* tw = nullptr;
    ZK_TRY(get_twiddles(c, log_n, inverse, &tw));
    const uint32_t tile = (uint32_t)std::min<size_t>(NTT_TILE, n);
    {
        ProfScope ps(c, "ntt_first_stages", 64.0 * (double)n);
        hipLaunchKernelGGL(ntt_first_stages_kernel, dim3((unsigned)(n / tile)), dim3(MLE_BLOCK), 0, c->stream, d_data, d_scratch,
                           log_n, tw);
    }
    for (uint32_t s = NTT_TILE_LOG; s < log_n;) {
        uint32_t T = std::min<uint32_t>(NTT_MID_MAX, log_n - s);
        if (log_n - s > NTT_MID_MAX && log_n - s < 2 * NTT_MID_MAX) T = (log_n - s + 1) / 2;   // balance the last two passes
        ProfScope ps(c, "ntt_mid_stages", 64.0 * (double)n);
        hipLaunchKernelGGL(ntt_mid_stages_kernel, dim3((unsigned)(n >> NTT_MID_TILE_LOG)), dim3(MLE_BLOCK), 0, c->stream,
                           d_scratch, log_n, s, T, tw);
        s += T;
    }
    if (inverse) {
        zkhost::Fr ni = zkhost::fr_inv(zkhost::fr_from_u64((uint64_t)n));
        FrArg sc;
        std::memcpy(sc.v, ni.l, 32);
        hipLaunchKernelGGL(elementwise_kernel<2>, dim3(mle_grid_stream(n)), dim3(MLE_BLOCK), 0, c->stream, d_scratch,
                           (const uint64_t*)nullptr, sc, n, d_data);
    } else {
        ZK_HIP(c, hipMemcpyAsync(d_data, d_scratch, n * 32, hipMemcpyDeviceToDevice, c->stream));
    }
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

extern "C" int zkhip_ntt(zkhip_ctx* c, uint64_t* d_data, uint32_t log_n, int inverse) {
    if (!c || !d_data) return ZKHIP_ERR_ARG;
    if (log_n > 30) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    const size_t n = (size_t)1 << log_n;
    ZK_TRY(c->reserve_ws(n * 32));
    return ntt_inplace(c, d_data, log_n, inverse, (uint64_t*)c->ws.ptr);
}

// Domain::fft / ifft as the reference calls them (domain.rs:108-118: clone, resize to the domain size with zeros, transform):
// d_src holds n_src <= 2^log_n values, d_dst receives the 2^log_n results; d_src is not modified.  The one aliasing rule, at every
// size: d_dst == d_src transforms in place and needs n_src == 2^log_n, anything shorter is ZKHIP_ERR_ARG (a buffer of n_src < n elements
// cannot take n results); buffers that overlap in any other way are not supported.
extern "C" int zkhip_domain_transform(zkhip_ctx* c, const uint64_t* d_src, size_t n_src, uint64_t* d_dst, uint32_t log_n, int inverse) {
    if (!c || !d_dst || (n_src && !d_src)) return ZKHIP_ERR_ARG;
    if (log_n > 30) return ZKHIP_ERR_SHAPE;
    const size_t n = (size_t)1 << log_n;
    if (n_src > n) return ZKHIP_ERR_SHAPE;
    if (d_dst == d_src && n_src != n) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    ZK_TRY(c->reserve_ws(n * 32));
    if (log_n >= 12) return ntt_big(c, d_src, n_src, nullptr, d_dst, n, log_n, inverse, (uint64_t*)c->ws.ptr);
    if (d_dst != d_src) {
        if (n_src < n) ZK_HIP(c, hipMemsetAsync(d_dst + 4 * n_src, 0, (n - n_src) * 32, c->stream));
        if (n_src) ZK_HIP(c, hipMemcpyAsync(d_dst, d_src, n_src * 32, hipMemcpyDeviceToDevice, c->stream));
    }
    return ntt_inplace(c, d_dst, log_n, inverse, (uint64_t*)c->ws.ptr);
}

// Coset hook of the PLONK prover (plonk.hip), transforms of >= 2^12 points: the forward transform of d_src[i] * d_mul[i], i < n_src,
// zero beyond -- the coset scaling c_i g^i and the zero padding both happen in the first pass's gather.  d_mul holds n_src entries.
int zk_ntt_scaled_transform(zkhip_ctx* c, const uint64_t* d_src, size_t n_src, const uint64_t* d_mul, uint64_t* d_dst, uint32_t log_n) {
    if (!c || !d_src || !d_mul || !d_dst) return ZKHIP_ERR_ARG;
    if (log_n < 12 || log_n > 30 || n_src > ((size_t)1 << log_n)) return ZKHIP_ERR_SHAPE;
    const size_t n = (size_t)1 << log_n;
    ZK_TRY(c->activate());
    ZK_TRY(c->reserve_ws(n * 32));
    return ntt_big(c, d_src, n_src, d_mul, d_dst, n, log_n, 0, (uint64_t*)c->ws.ptr);
}

extern "C" int zkhip_pointwise_mul(zkhip_ctx* c, const uint64_t* d_a, const uint64_t* d_b, size_t n, uint64_t* d_out) {
    if (!c || !d_a || !d_b || !d_out) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    hipLaunchKernelGGL(pointwise_mul_kernel, dim3(mle_grid_stream(n)), dim3(MLE_BLOCK), 0, c->stream, d_a, d_b, n, d_out);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

extern "C" int zkhip_univariate_multiply(zkhip_ctx* c, const uint64_t* d_a, size_t na, const uint64_t* d_b, size_t nb,
                                         uint64_t* d_out) {
    if (!c || !d_a || !d_b || !d_out) return ZKHIP_ERR_ARG;
    if (na == 0 || nb == 0) return ZKHIP_ERR_SHAPE;   // len_a + len_b - 1 underflows in the reference (evaluation.rs:66)
    ZK_TRY(c->activate());
    const size_t unscaled = na + nb - 1;
    uint32_t log_n = 0;
    while (((size_t)1 << log_n) < unscaled) ++log_n;
    if (log_n > 30) return ZKHIP_ERR_SHAPE;
    const size_t n = (size_t)1 << log_n;
    ZK_TRY(c->reserve_ws(3 * n * 32));
    uint64_t* scratch = (uint64_t*)c->ws.ptr;
    uint64_t* ea = scratch + 4 * n;
    uint64_t* eb = ea + 4 * n;
    if (log_n >= 12) {
        // three transforms and nothing else: the zero padding (resize, :73-74) happens in the forward transforms' gather, the
        // evaluation-form product (:79-82) in the inverse transform's gather, the truncation (:85) in its last pass
        ZK_TRY(ntt_big(c, d_a, na, nullptr, ea, n, log_n, 0, scratch));                              // domain.fft :76-77
        ZK_TRY(ntt_big(c, d_b, nb, nullptr, eb, n, log_n, 0, scratch));
        return ntt_big(c, ea, n, eb, d_out, unscaled, log_n, 1, scratch);                            // domain.ifft :84
    }
    ZK_HIP(c, hipMemsetAsync(ea, 0, 2 * n * 32, c->stream));                                        // resize(.., F::ZERO) :73-74
    ZK_HIP(c, hipMemcpyAsync(ea, d_a, na * 32, hipMemcpyDeviceToDevice, c->stream));
    ZK_HIP(c, hipMemcpyAsync(eb, d_b, nb * 32, hipMemcpyDeviceToDevice, c->stream));
    ZK_TRY(ntt_inplace(c, ea, log_n, 0, scratch));                                                   // domain.fft :76-77
    ZK_TRY(ntt_inplace(c, eb, log_n, 0, scratch));
    hipLaunchKernelGGL(pointwise_mul_kernel, dim3(mle_grid_stream(n)), dim3(MLE_BLOCK), 0, c->stream, ea, eb, n, ea);   // :79-82
    ZK_TRY(ntt_inplace(c, ea, log_n, 1, scratch));                                                   // domain.ifft :84
    ZK_HIP(c, hipMemcpyAsync(d_out, ea, unscaled * 32, hipMemcpyDeviceToDevice, c->stream));         // truncate :85
    return ZKHIP_OK;
}

// ---- a batch of transforms of one size (ntt_batch_kernels.hpp) ---------------------------------------------------------------
// Scratch a batch call may hold beyond the caller's buffers: this much, or what ONE row needs if that is more.  A batch that
// needs more runs as consecutive chunks of rows, each chunk one launch chain.  A constant, not a switch.
constexpr size_t NTT_BATCH_SCRATCH_BYTES = (size_t)256 << 20;

// Shapes that run as the loop of single calls: those at which the batched kernels were not measured ahead of the loop beyond the
// repeat-to-repeat spread (profiles/ntt_batch/NOTES.md).  That is a batch of ONE transform of >= 2^12 points -- the same workgroups
// as the single chain, 44.20 against 44.11 us at 2^12 and 50.88 against 50.75 us at 2^14; up to 2^11 points one transform is one
// launch instead of three and 1.1 to 1.5 times faster, and every batch of four or more is ahead at every size measured.
static bool ntt_batch_as_loop(uint32_t log_n, uint32_t batch) { return batch == 1 && log_n >= 12; }

// rows of n <= 2^11 points: one launch, no scratch; in / out may be the same rows
static int ntt_small_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* d_src, size_t src_stride, size_t n_src, const uint64_t* d_src2,
                           size_t src2_stride, uint64_t* d_dst, size_t dst_stride, size_t n_dst, uint32_t log_n, int inverse) {
    const size_t n = (size_t)1 << log_n;
    uint64_t* tw = nullptr;
    if (log_n) ZK_TRY(get_twiddles(c, log_n, inverse, &tw));
    FrArg sc = {};
    if (inverse) {
        const zkhost::Fr ni = zkhost::fr_inv(zkhost::fr_from_u64((uint64_t)n));
        std::memcpy(sc.v, ni.l, 32);
    }
    const uint32_t scaled = inverse && log_n ? 1u : 0u;
    const double bytes = (double)batch * (32.0 * (double)(n_src + n_dst) + (d_src2 ? 32.0 * (double)n_src : 0.0));
    if (log_n <= (uint32_t)NTT_TILE_LOG) {
        const uint32_t per = (uint32_t)NTT_TILE >> log_n;
        ProfScope ps(c, "ntt_batch_small", bytes);
        hipLaunchKernelGGL(ntt_batch_small_kernel<NTT_TILE_LOG>, dim3((batch + per - 1) / per), dim3(NTT_TILE / 4), (size_t)NTT_TILE * 32, c->stream,
                           d_src, src_stride, n_src, d_src2, src2_stride, d_dst, dst_stride, n_dst, batch, log_n, (const uint64_t*)tw, sc, scaled);
    } else {
        ProfScope ps(c, "ntt_batch_tile11", bytes);
        hipLaunchKernelGGL(ntt_batch_small_kernel<NTT_BIG_TILE_LOG>, dim3(batch), dim3(NTT_BIG_TILE / 4), (size_t)NTT_BIG_TILE * 32, c->stream,
                           d_src, src_stride, n_src, d_src2, src2_stride, d_dst, dst_stride, n_dst, batch, log_n, (const uint64_t*)tw, sc, scaled);
    }
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// rows of n >= 2^12 points, ntt_big with the row as the grid's second dimension: the first pass gathers src -> work, the passes run
// in place in work, the last one writes dst.  work == dst (n_dst == n, dst distinct from src) needs no scratch at all.
static int ntt_big_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* d_src, size_t src_stride, size_t n_src, const uint64_t* d_src2,
                         size_t src2_stride, uint64_t* d_dst, size_t dst_stride, size_t n_dst, uint32_t log_n, int inverse,
                         uint64_t* d_work, size_t work_stride) {
    const size_t n = (size_t)1 << log_n;
    NttPlan* plan = nullptr;
    ZK_TRY(get_plan(c, log_n, inverse, &plan));
    const size_t lds = (size_t)NTT_BIG_TILE * 32;
    const dim3 grid((unsigned)(n >> NTT_BIG_TILE_LOG), batch);
    {
        ProfScope ps(c, "ntt_batch_first8", (double)batch * (32.0 * (double)(n_src + n) + (d_src2 ? 32.0 * (double)n : 0.0)));
        hipLaunchKernelGGL(ntt_batch_first8_kernel, grid, dim3(NTT_BIG_BLOCK), lds, c->stream, d_src, src_stride, n_src, d_src2, src2_stride,
                           d_work, work_stride, log_n, (const uint64_t*)plan->tw1.get());
    }
    FrArg sc = {};
    std::memcpy(sc.v, plan->n_inv.l, 32);
    for (size_t p = 0; p < plan->passes.size(); ++p) {
        const NttPass& ps = plan->passes[p];
        const bool last = p + 1 == plan->passes.size();
        ProfScope pr(c, "ntt_batch_pass", (double)batch * 32.0 * (double)(n + (last ? n_dst : n)) + 32.0 * (double)((((size_t)1 << ps.T) - 1) << ps.s0));
        if (last && inverse)
            hipLaunchKernelGGL(ntt_batch_pass_kernel<true>, grid, dim3(NTT_BIG_BLOCK), lds, c->stream, (const uint64_t*)d_work, work_stride, d_dst, dst_stride,
                               ps.s0, ps.T, (const uint64_t*)ps.table.get(), sc, n_dst);
        else
            hipLaunchKernelGGL(ntt_batch_pass_kernel<false>, grid, dim3(NTT_BIG_BLOCK), lds, c->stream, (const uint64_t*)d_work, work_stride,
                               last ? d_dst : d_work, last ? dst_stride : work_stride, ps.s0, ps.T, (const uint64_t*)ps.table.get(), sc, last ? n_dst : n);
    }
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// rows per chunk when every row needs bufs scratch buffers of n elements
static uint32_t ntt_batch_chunk(uint32_t batch, size_t n, size_t bufs) {
    const size_t fit = std::max<size_t>(1, NTT_BATCH_SCRATCH_BYTES / (bufs * n * 32));
    return (uint32_t)std::min<size_t>(batch, fit);
}

// The batch form of zkhip_domain_transform (include/zkhip.h).  Allocates nothing when d_dst != d_src or n <= 2^11; in place at
// n >= 2^12 it holds min(batch, max(1, NTT_BATCH_SCRATCH_BYTES / 32n)) rows of the context's workspace and runs the batch in chunks of
// that many rows.
extern "C" int zkhip_domain_transform_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* d_src, size_t src_stride, size_t n_src,
                                            uint64_t* d_dst, size_t dst_stride, uint32_t log_n, int inverse) {
    if (!c || !d_dst || (n_src && !d_src)) return ZKHIP_ERR_ARG;
    if (log_n > 30) return ZKHIP_ERR_SHAPE;
    const size_t n = (size_t)1 << log_n;
    if (n_src > n || dst_stride < n || (batch > 1 && src_stride < n_src) || batch > 65535) return ZKHIP_ERR_SHAPE;
    const bool in_place = d_dst == d_src;
    if (in_place && (n_src != n || src_stride != dst_stride)) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    if (ntt_batch_as_loop(log_n, batch)) {
        if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;                         // before the first row is written, not between two
        for (uint32_t b = 0; b < batch; ++b)
            ZK_TRY(zkhip_domain_transform(c, d_src ? d_src + 4 * (size_t)b * src_stride : nullptr, n_src, d_dst + 4 * (size_t)b * dst_stride, log_n, inverse));
        return ZKHIP_OK;
    }
    const bool scratch = in_place && log_n >= 12;
    const uint32_t chunk = scratch ? ntt_batch_chunk(batch, n, 1) : batch;
    ZK_TRY(c->reserve_ws(scratch ? (size_t)chunk * n * 32 : 0));
    if (batch == 0) return ZKHIP_OK;
    if (log_n < 12) return ntt_small_batch(c, batch, d_src, src_stride, n_src, nullptr, 0, d_dst, dst_stride, n, log_n, inverse);
    if (!scratch) return ntt_big_batch(c, batch, d_src, src_stride, n_src, nullptr, 0, d_dst, dst_stride, n, log_n, inverse, d_dst, dst_stride);
    for (uint32_t b0 = 0; b0 < batch; b0 += chunk) {
        const uint32_t cnt = std::min(chunk, batch - b0);
        ZK_TRY(ntt_big_batch(c, cnt, d_src + 4 * (size_t)b0 * src_stride, src_stride, n_src, nullptr, 0, d_dst + 4 * (size_t)b0 * dst_stride, dst_stride,
                             n, log_n, inverse, (uint64_t*)c->ws.ptr, n));
    }
    return ZKHIP_OK;
}

// The batch form of zkhip_univariate_multiply: per chunk one batched forward transform of the a rows, one of the b rows and one
// batched inverse whose gather takes their product and whose store keeps na + nb - 1 coefficients.  Holds three buffers of n elements
// per row of a chunk (two at n <= 2^11), min(batch, max(1, NTT_BATCH_SCRATCH_BYTES / (96n, resp. 64n))) rows.
extern "C" int zkhip_univariate_multiply_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* d_a, size_t a_stride, size_t na,
                                               const uint64_t* d_b, size_t b_stride, size_t nb, uint64_t* d_out, size_t out_stride) {
    if (!c || !d_a || !d_b || !d_out) return ZKHIP_ERR_ARG;
    if (na == 0 || nb == 0) return ZKHIP_ERR_SHAPE;
    const size_t unscaled = na + nb - 1;
    uint32_t log_n = 0;
    while (log_n <= 30 && ((size_t)1 << log_n) < unscaled) ++log_n;
    if (log_n > 30 || out_stride < unscaled || batch > 65535 || (batch > 1 && (a_stride < na || b_stride < nb))) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    if (ntt_batch_as_loop(log_n, batch)) {
        if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;
        for (uint32_t b = 0; b < batch; ++b)
            ZK_TRY(zkhip_univariate_multiply(c, d_a + 4 * (size_t)b * a_stride, na, d_b + 4 * (size_t)b * b_stride, nb, d_out + 4 * (size_t)b * out_stride));
        return ZKHIP_OK;
    }
    const size_t n = (size_t)1 << log_n;
    const size_t bufs = log_n < 12 ? 2 : 3;                                      // up to 2^11 points the inverse needs no work buffer
    const uint32_t chunk = ntt_batch_chunk(batch, n, bufs);
    ZK_TRY(c->reserve_ws(bufs * chunk * n * 32));
    uint64_t* ea = (uint64_t*)c->ws.ptr;
    uint64_t* eb = ea + 4 * (size_t)chunk * n;
    uint64_t* work = eb + 4 * (size_t)chunk * n;
    for (uint32_t b0 = 0; b0 < batch; b0 += chunk) {
        const uint32_t cnt = std::min(chunk, batch - b0);
        const uint64_t* a = d_a + 4 * (size_t)b0 * a_stride;
        const uint64_t* b = d_b + 4 * (size_t)b0 * b_stride;
        uint64_t* out = d_out + 4 * (size_t)b0 * out_stride;
        if (log_n < 12) {
            ZK_TRY(ntt_small_batch(c, cnt, a, a_stride, na, nullptr, 0, ea, n, n, log_n, 0));
            ZK_TRY(ntt_small_batch(c, cnt, b, b_stride, nb, nullptr, 0, eb, n, n, log_n, 0));
            ZK_TRY(ntt_small_batch(c, cnt, ea, n, n, eb, n, out, out_stride, unscaled, log_n, 1));
        } else {
            ZK_TRY(ntt_big_batch(c, cnt, a, a_stride, na, nullptr, 0, ea, n, n, log_n, 0, ea, n));
            ZK_TRY(ntt_big_batch(c, cnt, b, b_stride, nb, nullptr, 0, eb, n, n, log_n, 0, eb, n));
            ZK_TRY(ntt_big_batch(c, cnt, ea, n, n, eb, n, out, out_stride, unscaled, log_n, 1, work, n));
        }
    }
    return ZKHIP_OK;
}

// ---- DenseUnivariatePolynomial at many points, and through many points (dense_points_kernels.hpp) -----------------------------------
// The plan -- segments, chunks of jobs, scratch layout -- is dense_points_plan.hpp.  The scratch is zkhip_ctx::dense_scratch, an
// allocation of this call's own that only grows: the call takes no byte of the workspace, is never refused for a lent one, and runs
// beside proofs in flight, commits in flight and sessions.  The inverse transforms of an interpolation are ntt_small_batch /
// ntt_big_batch with that scratch as their work buffer; their twiddle tables and pass plans are the context's (NttCache).
extern "C" int zkhip_dense_points_plan_info(int op, uint32_t batch, size_t n_in, size_t n_x, uint32_t* h_info) {
    if (!h_info || (op != DP_OP_EVALUATE && op != DP_OP_INTERPOLATE)) return ZKHIP_ERR_ARG;
    const DpPlan p = dp_plan(op, batch, n_in, n_x);
    h_info[DP_INFO_REGIME] = p.regime;
    h_info[DP_INFO_SEGS] = p.segs;
    h_info[DP_INFO_LANES] = p.lanes;
    h_info[DP_INFO_LAUNCHES] = p.launches;
    h_info[DP_INFO_SCRATCH_LO] = (uint32_t)p.scratch_bytes;
    h_info[DP_INFO_SCRATCH_HI] = (uint32_t)((uint64_t)p.scratch_bytes >> 32);
    h_info[DP_INFO_CHUNK_LEN] = DP_CHUNK;
    h_info[DP_INFO_JOBS_PER_CHUNK] = p.chunk;
    return p.regime == DP_REFUSED ? ZKHIP_ERR_SHAPE : ZKHIP_OK;
}

extern "C" int zkhip_dense_points(zkhip_ctx* c, int op, uint32_t batch, const uint64_t* d_in, size_t in_stride, size_t n_in,
                                  const uint64_t* d_x, size_t x_stride, size_t n_x, uint64_t* d_out, size_t out_stride) {
    if (!c || (op != DP_OP_EVALUATE && op != DP_OP_INTERPOLATE)) return ZKHIP_ERR_ARG;
    const DpPlan p = dp_plan(op, batch, n_in, n_x);
    if (p.regime == DP_REFUSED) return ZKHIP_ERR_SHAPE;
    if (p.regime == DP_NOOP) return ZKHIP_OK;
    if (!d_out || !d_x || (n_in && !d_in) || d_out == d_in || d_out == d_x) return ZKHIP_ERR_ARG;
    if (batch > 1 && (out_stride < n_x || (in_stride && in_stride < n_in) || (x_stride && x_stride < n_x))) return ZKHIP_ERR_SHAPE;   // rows that overlap
    ZK_TRY(c->activate());
    ZK_TRY(c->dense_scratch.reserve(p.scratch_bytes, {c->stream}, &c->last_hip));
    char* const base = (char*)c->dense_scratch.ptr;
    if (p.regime == DP_EVALUATE) {
        const dim3 grid(p.grid_x, p.segs, batch);
        ProfScope ps(c, "dense_points_eval", 0.0);
        if (p.segs == 1) {
            hipLaunchKernelGGL(dp_eval_kernel<false>, grid, dim3(DP_LANES), 0, c->stream, d_in, in_stride, n_in, d_x, x_stride, n_x, d_out, out_stride, p.seg_len);
        } else {
            uint64_t* rec = (uint64_t*)(base + p.o_rec2);
            hipLaunchKernelGGL(dp_eval_kernel<true>, grid, dim3(DP_LANES), 0, c->stream, d_in, in_stride, n_in, d_x, x_stride, n_x, rec, (size_t)0, p.seg_len);
            hipLaunchKernelGGL(dp_eval_sum_kernel, dim3(p.grid_x, 1, batch), dim3(DP_LANES), 0, c->stream, (const uint64_t*)rec, p.segs, n_x, d_out, out_stride);
        }
        ZK_HIP(c, hipGetLastError());
        return ZKHIP_OK;
    }
    const uint32_t n = (uint32_t)n_x, N = 1u << p.log_N, seg_len = (uint32_t)p.seg_len;
    const bool shared = batch == 1 || x_stride == 0;                 // one node set: its 1 / D_i are computed once for the batch
    uint32_t* flag = (uint32_t*)(base + p.o_flag);
    uint64_t *winv = (uint64_t*)(base + p.o_winv), *rec1 = (uint64_t*)(base + p.o_rec1), *rec2 = (uint64_t*)(base + p.o_rec2);
    uint64_t *vals = (uint64_t*)(base + p.o_vals), *work = (uint64_t*)(base + p.o_work);
    FrArg omega;
    { const zkhost::Fr w = root_of_unity(p.log_N); std::memcpy(omega.v, w.l, 32); }
    ZK_HIP(c, hipMemsetAsync(flag, 0, 4, c->stream));
    const uint32_t node_blocks = (n + DP_LANES - 1) / DP_LANES;
    auto weights = [&](const uint64_t* x, size_t stride, uint32_t rows) {
        ProfScope ps(c, "dense_points_weights", 0.0);
        if (p.segs == 1) {
            hipLaunchKernelGGL(dp_weights_kernel<false>, dim3(node_blocks, 1, rows), dim3(DP_LANES), 0, c->stream, x, stride, n, seg_len, winv, flag);
        } else {
            hipLaunchKernelGGL(dp_weights_kernel<true>, dim3(node_blocks, p.segs, rows), dim3(DP_LANES), 0, c->stream, x, stride, n, seg_len, rec1, flag);
            hipLaunchKernelGGL(dp_weights_fold_kernel, dim3(node_blocks, 1, rows), dim3(DP_LANES), 0, c->stream, (const uint64_t*)rec1, p.segs, n, winv, flag);
        }
    };
    if (shared) weights(d_x, 0, 1);
    for (uint32_t i = 0; i < p.n_chunks; ++i) {
        const DpChunk ch = dp_chunk(p, i);
        const uint64_t* x = shared ? d_x : d_x + 4 * (size_t)ch.first * x_stride;
        const uint64_t* y = d_in + 4 * (size_t)ch.first * in_stride;
        uint64_t* out = d_out + 4 * (size_t)ch.first * out_stride;
        if (!shared) weights(x, x_stride, ch.count);
        {
            ProfScope ps(c, "dense_points_domain", 0.0);
            const size_t xs = shared ? 0 : x_stride, ws = shared ? 0 : (size_t)n;
            if (p.segs == 1) {
                hipLaunchKernelGGL(dp_domain_kernel<false>, dim3(p.grid_x, 1, ch.count), dim3(DP_LANES), 0, c->stream, y, in_stride, x, xs,
                                   (const uint64_t*)winv, ws, n, N, seg_len, omega, vals);
            } else {
                hipLaunchKernelGGL(dp_domain_kernel<true>, dim3(p.grid_x, p.segs, ch.count), dim3(DP_LANES), 0, c->stream, y, in_stride, x, xs,
                                   (const uint64_t*)winv, ws, n, N, seg_len, omega, rec2);
                hipLaunchKernelGGL(dp_domain_fold_kernel, dim3(p.grid_x, 1, ch.count), dim3(DP_LANES), 0, c->stream, (const uint64_t*)rec2, p.segs, N, vals);
            }
        }
        ZK_HIP(c, hipGetLastError());
        if (p.log_N < DP_NTT_WORK_LOG) ZK_TRY(ntt_small_batch(c, ch.count, vals, N, N, nullptr, 0, out, out_stride, n, p.log_N, 1));
        else ZK_TRY(ntt_big_batch(c, ch.count, vals, N, N, nullptr, 0, out, out_stride, n, p.log_N, 1, work, N));
    }
    // the call's single synchronisation: one flag word, raised by a lane that met D_i == 0 (a repeated node)
    uint32_t* h_flag = (uint32_t*)c->pinned_u64(ZK_PIN_RES);
    ZK_HIP(c, hipMemcpyAsync(h_flag, flag, 4, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return *h_flag ? ZKHIP_ERR_ARG : ZKHIP_OK;
}

// ---- host-side Fr helpers ------------------------------------------------------------------------------
extern "C" int zkhip_fr_from_i64(int64_t v, uint64_t* h_out) {
    if (!h_out) return ZKHIP_ERR_ARG;
    zkhost::Fr m = zkhost::fr_from_u64(v < 0 ? (uint64_t)(-(v + 1)) + 1 : (uint64_t)v);
    if (v < 0) m = zkhost::fr_sub(zkhost::fr_zero(), m);
    std::memcpy(h_out, m.l, 32);
    return ZKHIP_OK;
}
extern "C" int zkhip_fr_to_canonical(const uint64_t* h_in, uint64_t* h_out) {
    if (!h_in || !h_out) return ZKHIP_ERR_ARG;
    zkhost::Fr a, one = zkhost::fr_zero();
    std::memcpy(a.l, h_in, 32);
    one.l[0] = 1;
    zkhost::Fr c = zkhost::fr_mul(a, one);
    std::memcpy(h_out, c.l, 32);
    return ZKHIP_OK;
}
#define ZK_FR_BINOP(NAME, FN)                                                                   \
    extern "C" int NAME(const uint64_t* h_a, const uint64_t* h_b, uint64_t* h_out) {            \
        if (!h_a || !h_b || !h_out) return ZKHIP_ERR_ARG;                                       \
        zkhost::Fr a, b;                                                                        \
        std::memcpy(a.l, h_a, 32); std::memcpy(b.l, h_b, 32);                                   \
        zkhost::Fr c = zkhost::FN(a, b);                                                        \
        std::memcpy(h_out, c.l, 32);                                                            \
        return ZKHIP_OK;                                                                        \
    }
ZK_FR_BINOP(zkhip_fr_add, fr_add)
ZK_FR_BINOP(zkhip_fr_sub, fr_sub)
ZK_FR_BINOP(zkhip_fr_mul, fr_mul)

// Synthetic benchmark inputs: splitmix64-seeded xoshiro256**; an element is four draws taken as a 256-bit
// little-endian integer with the top bit masked (255 bits), redrawn while >= r -- uniform over the field -- and handed out in
// the Montgomery form the tables hold.  Host side, deterministic for a seed whatever the machine.
extern "C" int zkhip_synthetic_fr(uint64_t seed, size_t n, uint64_t* h_out) {
    if (!h_out && n) return ZKHIP_ERR_ARG;
    uint64_t st[4];
    uint64_t x = seed;
    for (int i = 0; i < 4; ++i) {                      // splitmix64
        uint64_t z = (x += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        st[i] = z ^ (z >> 31);
    }
    auto rotl = [](uint64_t v, int k) { return (v << k) | (v >> (64 - k)); };
    auto next = [&]() {                                // xoshiro256**
        const uint64_t r = rotl(st[1] * 5, 7) * 9, t = st[1] << 17;
        st[2] ^= st[0]; st[3] ^= st[1]; st[1] ^= st[2]; st[0] ^= st[3];
        st[2] ^= t; st[3] = rotl(st[3], 45);
        return r;
    };
    zkhost::Fr r2;                                     // R^2 mod r: canonical -> Montgomery is one product with it
    std::memcpy(r2.l, zkhost::FR_R2, 32);
    for (size_t i = 0; i < n; ++i) {
        zkhost::Fr c;
        for (;;) {
            for (int k = 0; k < 4; ++k) c.l[k] = next();
            c.l[3] &= 0x7FFFFFFFFFFFFFFFull;
            bool lt = false;                           // c < r ?
            for (int k = 3; k >= 0; --k) {
                if (c.l[k] != zkhost::FR_P[k]) { lt = c.l[k] < zkhost::FR_P[k]; break; }
            }
            if (lt) break;
        }
        const zkhost::Fr m = zkhost::fr_mul(c, r2);    // c * R^2 * R^-1 = c R
        std::memcpy(h_out + 4 * i, m.l, 32);
    }
    return ZKHIP_OK;
}

