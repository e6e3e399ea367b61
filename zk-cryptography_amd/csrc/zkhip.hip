// zkhip.hip -- C-ABI entry points (include/zkhip.h) and host-side launch logic.
// gfx950 only.  No CPU fallback: every entry point launches HIP kernels or fails.
#include "../../include/zkhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "host_util.hpp"
#include "mle_kernels.hpp"
#include "mle_batch_kernels.hpp"
#include "sumcheck_kernels.hpp"
#include "sumcheck_batch_kernels.hpp"
#include "multifold_kernels.hpp"
#include "mfma_fold.hpp"
#include "fold_rounds.hpp"
#include "tunables.hpp"

using namespace zk;

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
static int g_last_hip = 0;   // last HIP error seen without a context (ctx_create)
extern "C" int zkhip_version(void) { return 1; }

extern "C" const char* zkhip_status_string(int s) {
    switch (s) {
        case ZKHIP_OK: return "ok";
        case ZKHIP_ERR_HIP: return "HIP runtime error";
        case ZKHIP_ERR_SHAPE: return "shape assertion failed";
        case ZKHIP_ERR_INDEX: return "index out of bounds";
        case ZKHIP_ERR_ARG: return "invalid argument";
        case ZKHIP_ERR_NOMEM: return "out of memory";
        case ZKHIP_ERR_BUSY: return "workspace lent to a live split-phase session";
        case ZKHIP_ERR_PEER: return "another rank of the sharded prover failed";
        case ZKHIP_ERR_TIMEOUT: return "a device-side wait gave up";
        default: return "unknown";
    }
}

extern "C" int zkhip_ctx_create(zkhip_ctx** out, int device, void* stream) {
    if (!out) return ZKHIP_ERR_ARG;
    int count = 0;
    hipError_t e0 = hipGetDeviceCount(&count);
    if (e0 != hipSuccess || device < 0 || device >= count) { g_last_hip = (int)e0; return ZKHIP_ERR_HIP; }
    std::unique_ptr<zkhip_ctx> c(new zkhip_ctx());      // (nothing is enqueued yet: an error exit just lets the members go)
    c->device = device;
    if (hipSetDevice(device) != hipSuccess) return ZKHIP_ERR_HIP;
    c->stream = (hipStream_t)stream;   // NULL = the device's default (null) stream, ordered with everything
    if (pin_alloc(c->h_pinned, ZK_PINNED_BYTES) != hipSuccess) return ZKHIP_ERR_HIP;
    if (dev_alloc(c->d_small, ZK_SMALL_BYTES) != hipSuccess) return ZKHIP_ERR_NOMEM;
    *out = c.release();
    return ZKHIP_OK;
}

extern "C" int zkhip_ctx_destroy(zkhip_ctx* c) {
    if (!c) return ZKHIP_ERR_ARG;
    hipSetDevice(c->device);
    c->gkr_lanes.clear();                                             // zkhip_gkr_prove_batch's lanes: each is destroyed like this context
    hipSetDevice(c->device);
    for (int k = 0; k < zkhip_ctx::ASYNC_SLOTS; ++k) if (c->async_pend[k]) zkhip_kzg_commit_end(c, (uint32_t)k, nullptr, nullptr);   // commits never collected
    (void)c->flush_deferred();
    c->drain_streams();      // before any member goes away (by its owner, in ~zkhip_ctx)
    delete c;
    return ZKHIP_OK;
}

extern "C" int zkhip_ctx_set_stream(zkhip_ctx* c, void* stream) {
    if (!c) return ZKHIP_ERR_ARG;
    if ((hipStream_t)stream == c->stream) return ZKHIP_OK;
    // Several entry points return before their kernels have run, and they share the context's scratch buffers: work
    // enqueued on the new stream must come after what is still queued on the old one.
    ZK_TRY(c->activate());
    (void)c->flush_deferred();                  // proofs in flight finish on the stream they began on (a failure is reported by their prove_end)
    ZK_TRY(c->ensure_side_streams());
    ZK_HIP(c, hipEventRecord(c->fork_ev.get(), c->stream));
    ZK_HIP(c, hipStreamWaitEvent((hipStream_t)stream, c->fork_ev.get(), 0));
    c->stream = (hipStream_t)stream;
    return ZKHIP_OK;
}
extern "C" int zkhip_ctx_synchronize(zkhip_ctx* c) {
    if (!c) return ZKHIP_ERR_ARG;
    (void)c->flush_deferred();
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return ZKHIP_OK;
}
extern "C" int zkhip_last_hip_error(zkhip_ctx* c) { return c ? c->last_hip : g_last_hip; }

extern "C" int zkhip_malloc(zkhip_ctx* c, void** d_ptr, size_t bytes) {
    if (!c || !d_ptr) return ZKHIP_ERR_ARG;
    hipSetDevice(c->device);
    hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 1);
    if (e != hipSuccess) { c->last_hip = (int)e; return ZKHIP_ERR_NOMEM; }
    return ZKHIP_OK;
}
extern "C" int zkhip_free(zkhip_ctx* c, void* d_ptr) {
    if (!c) return ZKHIP_ERR_ARG;
    if (d_ptr) (void)zkhip_table_release(c, d_ptr);      // (a table of the commit path: its address is no longer a known table, msm.hip)
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    ZK_HIP(c, dev_free_raw(d_ptr));
    return ZKHIP_OK;
}
extern "C" int zkhip_memcpy_h2d(zkhip_ctx* c, void* d_dst, const void* h_src, size_t bytes) {
    if (!c) return ZKHIP_ERR_ARG;
    ZK_HIP(c, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return ZKHIP_OK;
}
extern "C" int zkhip_memcpy_d2h(zkhip_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
    if (!c) return ZKHIP_ERR_ARG;
    ZK_HIP(c, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return ZKHIP_OK;
}

extern "C" int zkhip_profile_enable(zkhip_ctx* c, int enable) {
    if (!c) return ZKHIP_ERR_ARG;
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    c->profiling = enable != 0;
    c->prof_used = 0;
    c->prof_records.clear();
    return ZKHIP_OK;
}
extern "C" int zkhip_profile_read(zkhip_ctx* c, const char* kernel, double* total_ms, uint64_t* launches, double* bytes) {
    if (!c || !kernel) return ZKHIP_ERR_ARG;
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    double ms = 0, by = 0;
    uint64_t cnt = 0;
    for (auto& r : c->prof_records) {
        if (std::strcmp(r.name, kernel) != 0) continue;
        float t = 0;
        ZK_HIP(c, hipEventElapsedTime(&t, c->prof_events[r.event].start.get(), c->prof_events[r.event].stop.get()));
        ms += t; by += r.bytes; ++cnt;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = cnt;
    if (bytes) *bytes = by;
    return ZKHIP_OK;
}

extern "C" int zkhip_profile_timeline(zkhip_ctx* c, uint32_t max_records, char* names, double* start_us, double* stop_us,
                                      uint32_t* count) {
    if (!c || !names || !start_us || !stop_us || !count) return ZKHIP_ERR_ARG;
    ZK_HIP(c, hipDeviceSynchronize());
    uint32_t n = 0;
    for (auto& r : c->prof_records) {
        if (n == max_records) break;
        float a = 0, b = 0;
        ZK_HIP(c, hipEventElapsedTime(&a, c->prof_events[c->prof_records[0].event].start.get(), c->prof_events[r.event].start.get()));
        ZK_HIP(c, hipEventElapsedTime(&b, c->prof_events[c->prof_records[0].event].start.get(), c->prof_events[r.event].stop.get()));
        std::snprintf(names + 32 * (size_t)n, 32, "%s", r.name);
        start_us[n] = 1e3 * a;
        stop_us[n] = 1e3 * b;
        ++n;
    }
    *count = n;
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------

// fold variable var_index of an n-entry table; r on device. with_sums -> partials (returns grid size in *np)
static int launch_fold(zkhip_ctx* c, const uint64_t* d_in, size_t n, const uint64_t* d_r, const uint64_t* h_r,
                       uint32_t var_index, uint64_t* d_out, bool with_sums, uint64_t* d_partials, uint32_t* np) {
    FrArg rv = {};
    if (h_r) std::memcpy(rv.v, h_r, 32);
    const size_t n_out = n / 2;
    const uint32_t log_half = log2_exact(n) - 1 - var_index;
    const int grid = with_sums ? mle_grid((n_out + 1) / 2) : mle_grid_stream((n_out + 1) / 2);   // with sums: one record per workgroup
    ProfScope ps(c, with_sums ? "fold_sums" : "fold", 48.0 * (double)n);
    if (with_sums)
        hipLaunchKernelGGL(fold_kernel<true>, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_in, d_out, n_out, log_half,
                           d_r, rv, d_partials);
    else {
        // at most THREE workgroups per CU (a 40 KiB LDS request the kernel never touches; section 7 of profiles/r06/NOTES.md found the sums pass
        // no slower with a quarter of the loads in flight): 0.1427 -> 0.1372 ms at 2^24, 0.70 -> 0.73 of HBM; two per CU 0.161, four 0.137, no cap 0.143.
        constexpr size_t FOLD_LDS = 40960;
        hipLaunchKernelGGL(fold_kernel<false>, dim3(grid), dim3(MLE_BLOCK), FOLD_LDS, c->stream, d_in, d_out, n_out, log_half,
                           d_r, rv, d_partials);
    }
    if (np) *np = (uint32_t)grid;
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------
// Multilinear
// ---------------------------------------------------------------------------------------
extern "C" int zkhip_mle_partial_evaluation(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_r,
                                            const uint64_t* d_r, uint32_t var_index, uint64_t* d_out) {
    if (!c || !d_evals || !d_out || (!h_r == !d_r)) return ZKHIP_ERR_ARG;
    if (!is_pow2(n) || n < 2) return ZKHIP_ERR_SHAPE;                 // utils.rs:30  (and Multilinear::new :16-20)
    if (!((size_t)var_index < n / 2)) return ZKHIP_ERR_SHAPE;          // utils.rs:31-34
    if (var_index >= log2_exact(n)) return ZKHIP_OK;                   // 2^k >= n: the pair list is empty (utils.rs:37-50), so is the table
    ZK_TRY(c->activate());
    return launch_fold(c, d_evals, n, d_r, h_r, var_index, d_out, false, nullptr, nullptr);
}

static inline int multifold_cfg() { static const int v = (int)zk::env::read(zk::env::MF); return v; }   // (ZKHIP_MF, read once: below)
// the k-variable fold of a cn-entry table in the shape that suits its output size; returns the per-workgroup sums' count
static int launch_multifold(zkhip_ctx* c, hipStream_t stream, const uint64_t* cur, size_t cn, uint32_t k, const uint64_t* d_w,
                            uint64_t* dst, uint64_t* pdst, uint32_t* n_parts) {
    const size_t m = cn >> k;
    uint32_t out_per_wg;
    // diagnostics: ZKHIP_MF=0 keeps the VALU form for an A/B on the same box (tools/ab_multifold.sh); ZKHIP_MF=r (1..9) sets the rotation of
    // the term order (tile T starts at term r * T mod 2^k; the default 1 -- 3 and 5 measured the same, 0 = every wave at term 0: 108 vs 112 us
    // before the aligned planes); ZKHIP_MF_OCC=n caps the workgroups per CU through the LDS request (all 1024 workgroups are resident at once as it is, 4 per CU; capped at 2 per CU
    // or with 36-78 KiB requested per workgroup the pass takes the same 83-85 us, alone and beside the proofs in flight: round 6)
    const int mf_cfg = multifold_cfg();
    if (m >= 8192 && k >= 4 && mf_cfg != 0) {   // streaming shape, limb products on the matrix cores (mfma_fold.hpp)
        out_per_wg = 64;
        ProfScope ps(c, "multifold", 32.0 * (double)cn + 32.0 * (double)m, stream);
        const unsigned tiles = (unsigned)(m / 64), rot = (unsigned)mf_cfg;
        static const int mf_occ = (int)zk::env::read(zk::env::MF_OCC);
        size_t q_bytes = mfm_lds_bytes(std::min<uint32_t>(1u << k, (uint32_t)MFM_CHUNK));
        if (mf_occ > 0) q_bytes = std::max(q_bytes, (size_t)(((158 * 1024 / mf_occ) - 1024) & ~255));
        if (q_bytes > 64 * 1024) ZK_TRY(c->allow_big_lds((const void*)multifold_mfma_kernel<4, 4>, 158 * 1024));   // (the kernel has ~0.6 KiB of static LDS on top)
        hipLaunchKernelGGL((multifold_mfma_kernel<4, 4>), dim3(tiles / 4), dim3(256), q_bytes, stream, cur, m, k, d_w, dst, pdst, rot);
    } else if (m >= 8192) {   // streaming shape: 64 outputs per workgroup, its waves split the terms
        out_per_wg = 64;
        // >= 64 terms per lane: every lane pays one 9-word reduction (~a product), which at 16 terms per lane made the
        // 6-variable fold of the overlapped plan 12 % slower than the 8-variable one
        const uint32_t waves = k >= 8 ? 4 : k == 7 ? 2 : 1;
        ProfScope ps(c, "multifold", 32.0 * (double)cn + 32.0 * (double)m, stream);
        ProfScope form(c, "multifold_valu", 0.0, stream);   // (a second record of the same launch: which form it was)
        hipLaunchKernelGGL((multifold_kernel<64, 4, true>), dim3((unsigned)(m / 64)), dim3(64 * waves), ((size_t)32 << k) + 32 * (size_t)(waves - 1) * 64,
                           stream, cur, m, k, d_w, dst, pdst);
    } else {                  // few outputs left: 16 per workgroup, up to 64 lanes share one output
        out_per_wg = 16;
        uint32_t waves = 16;
        while (waves * 4 > (1u << k)) waves >>= 1;   // at least one term per lane group (k >= 3 here)
        ProfScope ps(c, "multifold_small", 32.0 * (double)cn + 32.0 * (double)m, stream);
        hipLaunchKernelGGL(multifold_kernel<16>, dim3((unsigned)(m / 16)), dim3(64 * waves), ((size_t)32 << k) + 32 * (size_t)(waves - 1) * 16, stream, cur, m, k, d_w, dst, pdst);
    }
    ZK_HIP(c, hipGetLastError());
    if (n_parts) *n_parts = (uint32_t)(m / out_per_wg);
    return ZKHIP_OK;
}
// Successive folds of variable 0 (or of h_var_indices); the points are host values, passed by value per launch.
static int fold_chain(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_pts,
                      const uint32_t* var_indices, size_t n_pts, uint64_t* d_out) {
    PtsArg pa = {};
    if (n_pts) std::memcpy(pa.v, h_pts, 32 * n_pts);
    // ping-pong buffers: A holds n/2, B holds n/4
    if (n_pts == 0) {
        ZK_HIP(c, hipMemcpyAsync(d_out, d_evals, n * 32, hipMemcpyDeviceToDevice, c->stream));
        return ZKHIP_OK;
    }
    const size_t need = (n / 2 + n / 4 + 8) * 32 + (256 + n / 512 + 4096) * 32;
    ZK_TRY(c->reserve_ws(need));
    uint64_t* A = (uint64_t*)c->ws.ptr;
    uint64_t* B = A + 4 * (n / 2);
    uint64_t* d_w = B + 4 * (n / 4 + 4);
    uint64_t* d_dummy = d_w + 4 * 256;            // per-workgroup output sums of the k-variable fold (unused here; <= n / 512 of them)
    const uint64_t* cur = d_evals;
    size_t cn = n;
    size_t p0 = 0;
    // every point folds variable 0 (`evaluation`, and partial_evaluations(&r, &vec![0; k]) as GKR calls it, gkr/src/protocol.rs:64-68):
    // collapse k of them per pass (weights = eq table of those points)
    bool all_zero = true;
    if (var_indices) for (size_t q = 0; q < n_pts; ++q) all_zero = all_zero && var_indices[q] == 0;
    if (all_zero) {
        uint32_t stage = 0;
        while (cn > (size_t)TAIL_N && n_pts - p0 >= 3) {
            uint32_t k = log2_exact(cn) - TAIL_LOG;
            if (k > MF_MAX_LOGK) k = MF_MAX_LOGK;
            if (k > n_pts - p0) k = (uint32_t)(n_pts - p0);
            if (k < 3) break;
            const size_t m = cn >> k;
            const bool last = (p0 + k == n_pts);
            uint64_t* dst = last ? d_out : ((stage & 1) ? B : A);
            hipLaunchKernelGGL(eq_weights_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, pa, (uint32_t)p0, k, d_w);
            ZK_TRY(launch_multifold(c, c->stream, cur, cn, k, d_w, dst, d_dummy, nullptr));
            cur = dst; cn = m; p0 += k; ++stage;
            if (last) return ZKHIP_OK;
        }
    }
    for (size_t p = p0; p < n_pts; ++p) {
        const uint32_t k = var_indices ? var_indices[p] : 0;
        if (cn < 2 || !((size_t)k < cn / 2)) return ZKHIP_ERR_SHAPE;
        if (k >= log2_exact(cn)) return p + 1 == n_pts ? ZKHIP_OK : ZKHIP_ERR_SHAPE;   // empty table (utils.rs:37-50); a further fold of it panics
        const bool all_zero_tail = !var_indices || [&] {
            for (size_t q = p; q < n_pts; ++q) if (var_indices[q]) return false;
            return true;
        }();
        if (all_zero_tail && cn <= (size_t)TAIL_N) {
            // finish every remaining fold inside one workgroup
            ProfScope ps(c, "fold_tail", 0.0);
            ZK_TRY(c->allow_big_lds((const void*)fold_tail_kernel, TAIL_LDS_BYTES));
            hipLaunchKernelGGL(fold_tail_kernel, dim3(1), dim3(MLE_BLOCK), TAIL_LDS_BYTES, c->stream, cur, (uint32_t)cn,
                               pa, (uint32_t)p, (uint32_t)(n_pts - p), d_out);
            ZK_HIP(c, hipGetLastError());
            return ZKHIP_OK;
        }
        const bool last = (p + 1 == n_pts);
        uint64_t* dst = last ? d_out : ((cur == A) ? B : A);
        ZK_TRY(launch_fold(c, cur, cn, nullptr, h_pts + 4 * p, k, dst, false, nullptr, nullptr));
        cur = dst;
        cn /= 2;
    }
    return ZKHIP_OK;
}

extern "C" size_t zkhip_mle_partial_evaluation_len(size_t n, uint32_t var_index) {
    if (!is_pow2(n) || n < 2 || !((size_t)var_index < n / 2)) return 0;
    return var_index >= log2_exact(n) ? 0 : n / 2;
}

extern "C" int zkhip_mle_partial_evaluations(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_pts,
                                             const uint32_t* h_var_indices, size_t n_pts, uint64_t* d_out) {
    if (!c || !d_evals || !d_out || (n_pts && (!h_pts || !h_var_indices))) return ZKHIP_ERR_ARG;
    if (!is_pow2(n)) return ZKHIP_ERR_SHAPE;
    if (n_pts > ZK_MAX_ROUNDS) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    return fold_chain(c, d_evals, n, h_pts, h_var_indices, n_pts, d_out);
}

extern "C" int zkhip_mle_evaluation(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_pts,
                                    size_t n_pts, uint64_t* h_out) {
    if (!c || !d_evals || !h_out || (n_pts && !h_pts)) return ZKHIP_ERR_ARG;
    if (!is_pow2(n)) return ZKHIP_ERR_SHAPE;
    if (n_pts != log2_exact(n)) return ZKHIP_ERR_SHAPE;                // assert_eq! evaluation_form.rs:163-167
    ZK_TRY(c->activate());
    uint64_t* d_res = c->small_u64(ZK_SMALL_RES);
    const uint32_t log_n = log2_exact(n);
    if (log_n >= 17) {
        // Every point is known before the first launch, so the evaluation is ONE pass over the table: with k1 leading variables per
        // output, p(r) = sum_j eq_j(r[k1..]) * (sum_b eq_b(r[..k1]) * T[b * m + j]) -- the k1-variable fold on the matrix cores
        // whose tiles weight their 64 outputs with the eq table of the remaining points and keep only that sum (32 n bytes read,
        // nothing written but m / 64 records), then the records' sum.  Three launches: the weight tables, the pass, the sum.
        const uint32_t k1 = std::min<uint32_t>(MF_MAX_LOGK, log_n - 13), k2 = log_n - k1, s2 = k2 / 2;
        const size_t m = n >> k1, tiles = m / 64, na = (size_t)1 << (k2 - s2), nb = (size_t)1 << s2;
        ZK_TRY(c->reserve_ws((256 + na + nb + tiles + 16) * 32));
        uint64_t* d_w1 = (uint64_t*)c->ws.ptr;
        uint64_t* d_wa = d_w1 + 4 * 256;
        uint64_t* d_wb = d_wa + 4 * na;
        uint64_t* d_rec = d_wb + 4 * nb;
        PtsArg pa = {};
        std::memcpy(pa.v, h_pts, 32 * n_pts);
        const size_t lanes = ((size_t)1 << k1) + na + nb;
        hipLaunchKernelGGL(eval_weights_kernel, dim3((unsigned)((lanes + MLE_BLOCK - 1) / MLE_BLOCK)), dim3(MLE_BLOCK), 0, c->stream, pa, k1, k2, s2, d_w1, d_wa, d_wb);
        {
            ProfScope ps(c, "multifold_eval", 32.0 * (double)n);
            const size_t q_bytes = mfm_lds_bytes(std::min<uint32_t>(1u << k1, (uint32_t)MFM_CHUNK));
            if (q_bytes > 64 * 1024) ZK_TRY(c->allow_big_lds((const void*)multifold_mfma_kernel<4, 4, true>, 158 * 1024));
            hipLaunchKernelGGL((multifold_mfma_kernel<4, 4, true>), dim3((unsigned)(tiles / 4)), dim3(256), q_bytes, c->stream, d_evals, m, k1,
                               (const uint64_t*)d_w1, (uint64_t*)nullptr, d_rec, 1u, (const uint64_t*)d_wa, (const uint64_t*)d_wb, s2);
        }
        hipLaunchKernelGGL(sum_records_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t*)d_rec, (uint32_t)tiles, d_res);
        ZK_HIP(c, hipGetLastError());
    } else {
        ZK_TRY(fold_chain(c, d_evals, n, h_pts, nullptr, n_pts, d_res));
    }
    ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_res, 32, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_out, c->pinned_u64(ZK_PIN_RES), 32);
    return ZKHIP_OK;
}

// MultilinearTrait::evaluation of `batch` tables of one length, each at its own point (include/zkhip.h; the kernels:
// mle_batch_kernels.hpp, what is decided here before anything is enqueued: mle_batch_plan.hpp).  A chunk is one upload of its table
// pointers and points, one launch (two above 2^12 entries), one copy of the results and one synchronisation.
extern "C" uint32_t zkhip_mle_evaluation_batch_min(size_t n) { return is_pow2(n) ? meb_min_batch(log2_exact(n)) : 0u; }

extern "C" int zkhip_mle_evaluation_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_table_ptrs, size_t n, const uint64_t* h_points,
                                          size_t n_pts, uint64_t* h_out) {
    if (!c) return ZKHIP_ERR_ARG;
    if (batch == 0) return ZKHIP_OK;
    if (!h_table_ptrs || !h_out || (n_pts && !h_points)) return ZKHIP_ERR_ARG;
    for (uint32_t b = 0; b < batch; ++b)
        if (!h_table_ptrs[b]) return ZKHIP_ERR_ARG;
    if (!is_pow2(n)) return ZKHIP_ERR_SHAPE;
    if (n_pts != log2_exact(n)) return ZKHIP_ERR_SHAPE;                // assert_eq! evaluation_form.rs:163-167
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;                     // a commit in flight or a split-phase session holds the workspace
    const uint32_t log_n = (uint32_t)n_pts;
    const MebPlan plan = meb_plan(log_n, batch);
    if (plan.regime == MEB_SINGLE) {                                   // the single call's own path, job after job (it activates the device itself)
        for (uint32_t b = 0; b < batch; ++b)
            ZK_TRY(zkhip_mle_evaluation(c, h_table_ptrs[b], n, h_points ? h_points + 4 * (size_t)b * n_pts : nullptr, n_pts, h_out + 4 * (size_t)b));
        return ZKHIP_OK;
    }
    ZK_TRY(c->activate());
    ZK_TRY(c->reserve_ws(plan.ws_bytes));
    ZK_TRY(c->reserve_msm_pin(0, plan.pin_bytes));
    char* ws = (char*)c->ws.ptr;
    char* pin = (char*)c->msm_pin[0].ptr;
    char* pin_up = pin + meb_align((size_t)plan.chunk * 32);
    const uint64_t* const* d_tables = (const uint64_t* const*)ws;
    const uint64_t* d_pts = (const uint64_t*)(ws + plan.o_points);
    uint64_t* d_res = (uint64_t*)(ws + plan.o_results);
    uint64_t* d_rec = (uint64_t*)(ws + plan.o_records);
    void (*resident)(const uint64_t* const*, uint32_t, const uint64_t*, uint32_t, uint64_t*) =
        plan.lanes == MEB_WIDE_BLOCK ? mle_eval_batch_resident_kernel<(int)MEB_WIDE_BLOCK> : mle_eval_batch_resident_kernel<(int)MEB_BLOCK>;
    ZK_TRY(c->allow_big_lds(plan.regime == MEB_RESIDENT ? (const void*)resident : (const void*)mle_eval_batch_blocks_kernel, plan.lds_bytes));
    for (uint32_t i = 0; i < plan.n_chunks; ++i) {
        const MebChunk ch = meb_chunk(plan, batch, i);
        // (the previous chunk's upload has ended: every chunk ends in a synchronisation)
        std::memcpy(pin_up, h_table_ptrs + ch.first, (size_t)ch.count * 8);
        if (n_pts) std::memcpy(pin_up + plan.o_points, h_points + 4 * (size_t)ch.first * n_pts, (size_t)ch.count * n_pts * 32);
        ZK_HIP(c, hipMemcpyAsync(ws, pin_up, n_pts ? plan.o_points + (size_t)ch.count * n_pts * 32 : (size_t)ch.count * 8, hipMemcpyHostToDevice, c->stream));
        if (plan.regime == MEB_RESIDENT) {
            ProfScope ps(c, "mle_eval_batch", 32.0 * (double)n * ch.count);
            hipLaunchKernelGGL(resident, dim3(ch.count), dim3(plan.lanes), plan.lds_bytes, c->stream, d_tables, (uint32_t)n, d_pts,
                               (uint32_t)n_pts, d_res);
        } else {
            {
                ProfScope ps(c, "mle_eval_batch", 32.0 * (double)n * ch.count);
                hipLaunchKernelGGL(mle_eval_batch_blocks_kernel, dim3(plan.wgs_per_job, ch.count), dim3(plan.lanes), plan.lds_bytes, c->stream, d_tables, plan.h,
                                   d_pts, (uint32_t)n_pts, d_rec);
            }
            hipLaunchKernelGGL(mle_eval_batch_sum_kernel, dim3((ch.count + MLE_BLOCK - 1) / MLE_BLOCK), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t*)d_rec,
                               plan.records_per_job, ch.count, d_res);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_HIP(c, hipMemcpyAsync(pin, d_res, (size_t)ch.count * 32, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(h_out + 4 * (size_t)ch.first, pin, (size_t)ch.count * 32);
    }
    return ZKHIP_OK;
}

extern "C" int zkhip_mle_half_sums(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint64_t* h_out) {
    if (!c || !d_evals || !h_out) return ZKHIP_ERR_ARG;
    if (n == 0) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    uint64_t* d_partials = c->small_u64(ZK_SMALL_PARTIALS);
    uint64_t* d_res = c->small_u64(ZK_SMALL_RES);
    const int grid = mle_grid((n + 1) / 2);
    {
        ProfScope ps(c, "half_sums", 32.0 * (double)n);
        hipLaunchKernelGGL(half_sums_kernel, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_evals, n, d_partials);
    }
    hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, d_partials, (uint32_t)grid, d_res);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_res, 96, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_out, c->pinned_u64(ZK_PIN_RES), 96);
    return ZKHIP_OK;
}

static int distinct(zkhip_ctx* c, bool mul, const uint64_t* d_a, size_t na, const uint64_t* d_b, size_t nb,
                    uint64_t* d_out) {
    if (!c || !d_a || !d_b || !d_out) return ZKHIP_ERR_ARG;
    if (!is_pow2(na * nb)) return ZKHIP_ERR_SHAPE;   // Self::new(new_evaluations) asserts a power of two
    ZK_TRY(c->activate());
    const size_t n_out = na * nb;
    const int grid = mle_grid_stream(n_out);
    if (mul)
        hipLaunchKernelGGL(distinct_kernel<true>, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_a, d_b, nb, n_out, d_out);
    else
        hipLaunchKernelGGL(distinct_kernel<false>, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_a, d_b, nb, n_out, d_out);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}
extern "C" int zkhip_mle_add_distinct(zkhip_ctx* c, const uint64_t* d_a, size_t na, const uint64_t* d_b, size_t nb,
                                      uint64_t* d_out) { return distinct(c, false, d_a, na, d_b, nb, d_out); }
extern "C" int zkhip_mle_mul_distinct(zkhip_ctx* c, const uint64_t* d_a, size_t na, const uint64_t* d_b, size_t nb,
                                      uint64_t* d_out) { return distinct(c, true, d_a, na, d_b, nb, d_out); }

extern "C" int zkhip_mle_elementwise(zkhip_ctx* c, int op, const uint64_t* d_a, const uint64_t* d_b,
                                     const uint64_t* h_scalar, size_t n, size_t nb, uint64_t* d_out) {
    if (!c || !d_a || !d_out || op < 0 || op > 2) return ZKHIP_ERR_ARG;
    if (op == 2 ? !h_scalar : !d_b) return ZKHIP_ERR_ARG;
    if (op != 2 && nb < n) return ZKHIP_ERR_INDEX;      // rhs.evaluations[i] out of bounds (evaluation_form.rs:185,215)
    if (n == 0) return ZKHIP_OK;
    ZK_TRY(c->activate());
    const int grid = mle_grid_stream(n);
    FrArg sc = {};
    if (op == 2) {
        std::memcpy(sc.v, h_scalar, 32);
        hipLaunchKernelGGL(elementwise_kernel<2>, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_a, (const uint64_t*)nullptr, sc, n, d_out);
    } else if (op == 0) {
        hipLaunchKernelGGL(elementwise_kernel<0>, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_a, d_b, sc, n, d_out);
    } else {
        hipLaunchKernelGGL(elementwise_kernel<1>, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_a, d_b, sc, n, d_out);
    }
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

extern "C" int zkhip_mle_to_bytes(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint8_t* d_out_bytes) {
    if (!c || !d_evals || !d_out_bytes) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    hipLaunchKernelGGL(to_bytes_kernel, dim3(mle_grid_stream(n)), dim3(MLE_BLOCK), 0, c->stream, d_evals, n,
                       (uint32_t*)d_out_bytes);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

extern "C" int zkhip_mle_add_to_front(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint32_t variable_length, uint64_t* d_out) {
    if (!c || !d_evals || !d_out) return ZKHIP_ERR_ARG;
    if (!is_pow2(n) || variable_length > 40) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    const size_t n_out = n * ((size_t)2 << variable_length);
    hipLaunchKernelGGL(repeat_kernel, dim3(mle_grid_stream(n_out)), dim3(MLE_BLOCK), 0, c->stream, d_evals, n, 0u, n_out, d_out);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}
extern "C" int zkhip_mle_add_to_back(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint32_t variable_length, uint64_t* d_out) {
    if (!c || !d_evals || !d_out) return ZKHIP_ERR_ARG;
    if (!is_pow2(n) || variable_length > 40) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    if (variable_length == 0) {
        ZK_HIP(c, hipMemcpyAsync(d_out, d_evals, 32 * n, hipMemcpyDeviceToDevice, c->stream));
        return ZKHIP_OK;
    }
    const size_t n_out = n << variable_length;
    hipLaunchKernelGGL(repeat_kernel, dim3(mle_grid_stream(n_out)), dim3(MLE_BLOCK), 0, c->stream, d_evals, n, variable_length, n_out, d_out);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------
// layered circuit (GKR table builders)
// ---------------------------------------------------------------------------------------
extern "C" size_t zkhip_gkr_mle_size(uint32_t layer_index) {   // circuit/src/utils.rs:1-10
    if (layer_index == 0) return (size_t)1 << 3;
    return (size_t)1 << (layer_index + 2 * (layer_index + 1));
}
// packs the host gate arrays into the workspace as (type, in0, in1) words
static int upload_gates(zkhip_ctx* c, const uint8_t* h_gate_type, const uint32_t* h_in0, const uint32_t* h_in1, size_t n_gates,
                        uint32_t** d_gates) {
    std::vector<uint32_t> packed(3 * n_gates);
    for (size_t g = 0; g < n_gates; ++g) {
        packed[3 * g] = h_gate_type[g] ? 1u : 0u;
        packed[3 * g + 1] = h_in0[g];
        packed[3 * g + 2] = h_in1[g];
    }
    ZK_TRY(c->reserve_ws(12 * n_gates + 256));
    ZK_HIP(c, hipMemcpyAsync(c->ws.ptr, packed.data(), 12 * n_gates, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));   // `packed` is a stack temporary
    *d_gates = (uint32_t*)c->ws.ptr;
    return ZKHIP_OK;
}
extern "C" int zkhip_circuit_layer_eval(zkhip_ctx* c, const uint64_t* d_in, size_t n_in, const uint8_t* h_gate_type,
                                        const uint32_t* h_in0, const uint32_t* h_in1, size_t n_gates, uint64_t* d_out) {
    if (!c || !d_in || !d_out || (n_gates && (!h_gate_type || !h_in0 || !h_in1))) return ZKHIP_ERR_ARG;
    for (size_t g = 0; g < n_gates; ++g)
        if (h_in0[g] >= n_in || h_in1[g] >= n_in) return ZKHIP_ERR_INDEX;   // current_input[e.inputs[k]] panics
    if (n_gates == 0) return ZKHIP_OK;
    ZK_TRY(c->activate());
    uint32_t* d_gates = nullptr;
    ZK_TRY(upload_gates(c, h_gate_type, h_in0, h_in1, n_gates, &d_gates));
    hipLaunchKernelGGL(circuit_layer_kernel, dim3(mle_grid(n_gates)), dim3(MLE_BLOCK), 0, c->stream, d_in, d_gates, n_gates, d_out);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipStreamSynchronize(c->stream));   // the gate list lives in the shared workspace
    return ZKHIP_OK;
}
extern "C" int zkhip_circuit_add_mult_mle(zkhip_ctx* c, const uint8_t* h_gate_type, const uint32_t* h_in0, const uint32_t* h_in1,
                                          size_t n_gates, uint32_t layer_index, uint64_t* d_add, uint64_t* d_mul) {
    if (!c || !d_add || !d_mul || (n_gates && (!h_gate_type || !h_in0 || !h_in1))) return ZKHIP_ERR_ARG;
    if (layer_index > 12) return ZKHIP_ERR_SHAPE;   // 2^(3 l + 2) elements
    const size_t size = zkhip_gkr_mle_size(layer_index);
    const uint32_t shift = layer_index + 1;
    for (size_t g = 0; g < n_gates; ++g) {
        const size_t idx = (g << (2 * shift)) | ((size_t)h_in0[g] << shift) | h_in1[g];
        if (idx >= size) return ZKHIP_ERR_INDEX;     // add_evaluations[gate_decimal] out of bounds
    }
    if (n_gates && c->ws_loans.lent()) return ZKHIP_ERR_BUSY;    // the gate list goes through the workspace: refused before the tables are cleared
    ZK_TRY(c->activate());
    ZK_HIP(c, hipMemsetAsync(d_add, 0, 32 * size, c->stream));   // F::zero() is all-zero limbs
    ZK_HIP(c, hipMemsetAsync(d_mul, 0, 32 * size, c->stream));
    if (n_gates == 0) return ZKHIP_OK;
    uint32_t* d_gates = nullptr;
    ZK_TRY(upload_gates(c, h_gate_type, h_in0, h_in1, n_gates, &d_gates));
    hipLaunchKernelGGL(wiring_ones_kernel, dim3(mle_grid(n_gates)), dim3(MLE_BLOCK), 0, c->stream, d_gates, n_gates, shift, d_add, d_mul);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------
// basic sumcheck prover
// ---------------------------------------------------------------------------------------
// Stage plan of the prover: a table of cur_n > TAIL_N entries is folded by k variables at once, k chosen so
// that tables up to 2^20 entries land exactly on the LDS tail and larger ones shrink 256-fold per pass.
static inline uint32_t stage_k(size_t cur_n) {
    if (cur_n <= ((size_t)1 << TREE_MAX_LOG)) return 0;      // finishes inside the serial kernel
    const uint32_t lg = log2_exact(cur_n);
    uint32_t k = lg - 8;                                       // aim at a 2^8-entry table (1 fold product per helper lane)
    if (k > MF_MAX_LOGK) k = MF_MAX_LOGK;
    return k;                                                  // >= 3 here
}
// Overlapped plan (tables of 2^24 entries; measured against the stage plan at every size with the rounds at 4.5 us, tools/step_sizes.py:
// 2^19 192 / 158 us, 2^20 201 / 171, 2^21 216 / 199, 2^22 230 / 218, 2^23 259 / 253, 2^24 322 / 347 -- only where the fold is long
// enough to hide ten rounds does running them beside it pay for the two extra launches).  Identity (1) of multifold_kernels.hpp applied twice: with FINE block
// sums B_g (2^g blocks of 256 entries, g = lg - 8) the first k1 rounds run on B_k1 (grouped B_g) and the next k2 = g - k1
// rounds on fold_k1(B_g; r_1..r_k1) -- a table of 2^k2 <= 1024 entries -- so rounds k1+1 .. g need the first k1 challenges
// but NOT the folded big table.  The streaming k1-variable fold of the big table therefore runs on a side stream next to
// the serial kernel of those rounds and is joined before the fold by the next k2 variables.  k2 is as large as the serial
// kernel takes (10), so that the fold starts as early as possible: 2^24 = 6 rounds | fold (100 us) next to 10 rounds | 8
// rounds.  Same values as the round-by-round loop, bit for bit.
static inline uint32_t overlapped_min_log() {       // (ZKHIP_OVERLAP_MIN_LOG: tuning aid, read once)
    static const uint32_t v = (uint32_t)zk::env::read(zk::env::OVERLAP_MIN_LOG); return v;
}
static inline bool overlapped_plan(size_t n) { return is_pow2(n) && n >= ((size_t)1 << overlapped_min_log()) && n <= ((size_t)1 << 24); }
// A rank's SHARD takes the overlapped stage over the whole range it was built for: there it is also the form with the fewest exchanges
// (three per proof), which is what counts over the fabric.
static inline bool overlapped_shard(size_t n) { return is_pow2(n) && n >= ((size_t)1 << 19) && n <= ((size_t)1 << 24); }
static inline uint32_t overlapped_k2(size_t n) { return std::min<uint32_t>(TREE_MAX_LOG, log2_exact(n) - 8 - 3); }
extern "C" int zkhip_sumcheck_plan_log_blocks(size_t n) {
    if (!is_pow2(n)) return 0;
    return overlapped_plan(n) ? (int)(log2_exact(n) - 8) : (int)stage_k(n);
}

// min_lds: pads the dynamic LDS request.  The serial kernel that runs next to the streaming fold asks for (nearly) a whole
// CU's LDS so that no workgroup of the fold shares its CU: beside 8+ fold waves per SIMD the transcript wave ran at half speed.
static int launch_small(zkhip_ctx* c, const SmallArgs& a, SumcheckDev* st, uint64_t* d_rp, uint64_t* d_ch, size_t min_lds = 0,
                        hipStream_t stream = nullptr) {
    if (!stream) stream = c->stream;
    if (a.log_n > (uint32_t)TREE_MAX_LOG || a.n_rounds > a.log_n) return ZKHIP_ERR_SHAPE;
    const size_t lds = std::max(small_lds_bytes(a.log_n, a.weights_out ? (int)a.n_rounds : -1, a.group != 0 && a.stride == 0), min_lds);
    if (lds > 160 * 1024) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->allow_big_lds((const void*)sumcheck_small_kernel, 160 * 1024));
    ProfScope ps(c, "sumcheck_small", 0.0, stream);
    hipLaunchKernelGGL(sumcheck_small_kernel, dim3(1), dim3(SMALL_BLOCK), lds, stream, a, st, d_rp, d_ch);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// The synchronous overlapped proof (lane < 0) takes its big fold and the rounds beside it as one launch (fold_rounds.hpp) wherever that
// fold has its matrix-core form: k1 >= 4 and 2^13 outputs or more, which in this plan is from 2^22 entries on.  Below that (the vector
// form, k1 = 3) and for every proof in flight the fork stays as it is.
static inline bool fold_rounds_plan(size_t n, int lane) {
    if (lane >= 0 || !overlapped_plan(n)) return false;
    const uint32_t k2 = overlapped_k2(n), k1 = log2_exact(n) - 8 - k2;
    return multifold_cfg() != 0 && fold_rounds_serves(n >> k1, k1, small_lds_bytes(k2, (int)k2, false));
}
// serial rounds `a` (sumcheck_small_kernel's arguments) as workgroup 0 and the k-variable fold of `cur` (cn entries) into dst as the
// other workgroups of one launch.  Recorded as the fold it contains -- the bytes are the fold's -- and a second time under the form's name.
static int launch_fold_rounds(zkhip_ctx* c, hipStream_t stream, const SmallArgs& a, SumcheckDev* st, uint64_t* d_rp, uint64_t* d_ch,
                              const uint64_t* cur, size_t cn, uint32_t k, const uint64_t* d_w, uint64_t* dst) {
    const size_t m = cn >> k;
    if (a.log_n > (uint32_t)TREE_MAX_LOG || a.n_rounds > a.log_n) return ZKHIP_ERR_SHAPE;
    if (!fold_rounds_serves(m, k, small_lds_bytes(a.log_n, a.weights_out ? (int)a.n_rounds : -1, a.group != 0 && a.stride == 0)))
        return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->allow_big_lds((const void*)fold_rounds_kernel, 158 * 1024));   // (~0.5 KiB of static LDS on top)
    uint32_t cus = 0;
    ZK_TRY(c->compute_units(&cus));
    // one resident fold workgroup on every CU beside the serial workgroup's: no second generation, no tail (fold_schedule.hpp)
    const uint32_t fold_wgs = fold_schedule_workgroups(m / 64, cus);
    ProfScope ps(c, "multifold", 32.0 * (double)cn + 32.0 * (double)m, stream);
    ProfScope form(c, "multifold_rounds", 0.0, stream);   // (a second record of the same launch: which form it was)
    hipLaunchKernelGGL(fold_rounds_kernel, dim3(1 + fold_wgs), dim3(SMALL_BLOCK), FOLD_ROUNDS_LDS, stream, a, st, d_rp, d_ch,
                       cur, m, k, d_w, dst, (uint32_t)multifold_cfg());
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// the arguments of a serial launch: n_rounds rounds from round0 on, on this source; every other field zero (the transcript continues)
static SmallArgs small_rounds(const uint64_t* src, uint32_t group, uint32_t stride, uint32_t canon, uint32_t log_n, uint32_t n_rounds,
                              uint32_t round0, uint64_t* weights_out) {
    SmallArgs a = {};
    a.src = src; a.group = group; a.stride = stride; a.canon = canon; a.log_n = log_n; a.n_rounds = n_rounds; a.round0 = round0;
    a.weights_out = weights_out;
    return a;
}
// how the transcript opens (SmallArgs::first; the first serial launch of a proof alone consumes it): not at all when the launch continues
// one, else with the host's claimed sum, the device's, or lo + hi
static void small_open(SmallArgs& a, bool opens, const uint64_t* h_claimed, const uint64_t* d_claimed) {
    a.first = !opens ? 0u : h_claimed ? 2u : d_claimed ? 3u : 1u;
    if (a.first == 2) std::memcpy(a.claimed.v, h_claimed, 32);   // prove(&self) absorbs self.sum (sumcheck.rs:33-35)
    if (a.first == 3) a.d_claimed = d_claimed;
}

// the first fold of the overlapped plan (k <= 6 variables, 2^19 .. 2^24 entries) leaves its partial tables in 2 x 1024 entries (ProofLayout::p1
// below, the sharded stage's d_mid), the second one (m = 256, k <= 10) in 32 x 256
constexpr size_t SC_FINE_ENTRIES = (size_t)1 << 16;       // fine sums: n / 256 <= 2^16
constexpr size_t SC_P1_ENTRIES = 2 * 1024, SC_P2_ENTRIES = 32 * 256;
constexpr bool blockfold_fits(uint32_t m, uint32_t k_max, uint32_t room) {
    for (uint32_t k = 1; k <= k_max; ++k) {
        BlockfoldShape sh = {};
        if (!blockfold_shape(m, k, &sh) || sh.ny * m > room || sh.sl * sh.per * sh.ny != (1u << k)) return false;
    }
    return true;
}
static_assert(blockfold_fits(256, 6, SC_P1_ENTRIES) && blockfold_fits(512, 6, SC_P1_ENTRIES) && blockfold_fits(1024, 6, SC_P1_ENTRIES) &&
              blockfold_fits(256, 10, SC_P2_ENTRIES),
              "blockfold_shape: more partial tables than the prover's buffers hold");
// k-variable fold of a small table spread over the chip: partial tables P[y][m], y < *n_slices (blockfold_kernel; its grid and
// the split of the terms come from blockfold_shape, multifold_kernels.hpp)
static int launch_blockfold(zkhip_ctx* c, hipStream_t stream, const uint64_t* in, uint32_t m, uint32_t k, const uint64_t* d_w,
                            uint64_t* d_partial, uint32_t* n_slices) {
    BlockfoldShape sh;
    if (!blockfold_shape(m, k, &sh)) return ZKHIP_ERR_SHAPE;
    const uint32_t terms = 1u << k;
    ProfScope ps(c, "blockfold", 32.0 * (double)m * terms, stream);
    hipLaunchKernelGGL(blockfold_kernel, dim3(m >> sh.log_ow, sh.ny), dim3(BF_BLOCK), 0, stream, in, m, sh.sl, sh.per, d_w, d_partial);
    ZK_HIP(c, hipGetLastError());
    *n_slices = sh.ny;
    return ZKHIP_OK;
}
// fine block sums: d_fine[2^lb] = sums of the 2^lb equal consecutive blocks of the table (each >= FINE_CHUNK entries);
// d_chunk (n / FINE_CHUNK entries of scratch) is only touched when a block is longer than FINE_CHUNK
static int launch_fine_sums(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint32_t lb, uint64_t* d_fine, uint64_t* d_chunk,
                            hipStream_t stream = nullptr) {
    if (!stream) stream = c->stream;
    const size_t blk = n >> lb, n_chunks = n / FINE_CHUNK;
    uint64_t* first = blk == (size_t)FINE_CHUNK ? d_fine : d_chunk;
    {
        // (measured and dropped: waves that stay and loop over run pairs with the next pair's loads in flight -- 100-115 us
        // against 94-96 us for this one-shot form at 2^24; the loads alone take 81 us, tools/ubench_rows.hip "pieces")
        ProfScope ps(c, "fine_sums", 32.0 * (double)n, stream);
        // TWO workgroups (8 waves) per CU, through an LDS request the kernel never touches: with all the waves its registers allow
        // (6 per SIMD) the pass keeps ~48 MiB of loads in flight -- no faster (93 us against 90-91 us with two workgroups per CU, one:
        // 123 us), and every other kernel's loads queue behind them: the first rounds and small folds of the proofs in flight beside
        // it took 50-150 us instead of 10-40, 0.212 against 0.201 ms per proof (profiles/r06/NOTES.md section 7).
        // ZKHIP_FINE_LDS=<bytes> overrides (diagnostics; 0 = no cap).
        static const size_t lds = (size_t)zk::env::read(zk::env::FINE_LDS);
        if (lds > 64 * 1024) ZK_TRY(c->allow_big_lds((const void*)fine_sums_kernel, 158 * 1024));
        hipLaunchKernelGGL(fine_sums_kernel, dim3((unsigned)((n_chunks + 7) / 8)), dim3(MLE_BLOCK), lds, stream, d_evals, n_chunks, first);
    }
    if (first != d_fine)
        hipLaunchKernelGGL(group_sums_wg_kernel, dim3(1u << lb), dim3(MLE_BLOCK), 0, stream, first, (uint32_t)(blk / FINE_CHUNK), d_fine, (uint64_t*)nullptr);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// partial sums of the table `cur` (cn entries in blocks of m) at chunk = min(m, 4096) entries per workgroup, on `stream` into d_partials
// (cn / chunk values).  Returns how many partials each block has and leaves in *parts where they are: the table's entries themselves,
// and no launch, when a block is shorter than a workgroup.
static uint32_t launch_chunk_sums(zkhip_ctx* c, hipStream_t stream, const uint64_t* cur, size_t cn, size_t m, uint64_t* d_partials,
                                  const uint64_t** parts) {
    const uint32_t chunk = (uint32_t)std::min<size_t>(m, 4096);
    if (chunk < (uint32_t)MLE_BLOCK) { *parts = cur; return (uint32_t)m; }   // tiny table: every entry is its own partial
    ProfScope ps(c, "chunk_sums", 32.0 * (double)cn, stream);
    hipLaunchKernelGGL(chunk_sums_kernel, dim3((unsigned)(cn / chunk)), dim3(MLE_BLOCK), 0, stream, cur, chunk, d_partials);
    *parts = d_partials;
    return (uint32_t)(m / chunk);
}
// (2^log_blocks block sums, then the total) of a table, on the device
static int block_sums_impl(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint32_t log_blocks, uint64_t* d_out, uint64_t* h_total, bool want_total) {
    if (!c || !d_evals || !d_out) return ZKHIP_ERR_ARG;
    if (!is_pow2(n) || log_blocks > 16 || ((size_t)1 << log_blocks) > n) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    const size_t m = n >> log_blocks;
    if (log_blocks > (uint32_t)MF_CAP_LOGK) {      // fine sums (the overlapped prover's granularity)
        if (m < (size_t)FINE_CHUNK) return ZKHIP_ERR_SHAPE;
        uint64_t* d_chunk = nullptr;
        if (m > (size_t)FINE_CHUNK) { ZK_TRY(c->reserve_ws((n / FINE_CHUNK) * 32)); d_chunk = (uint64_t*)c->ws.ptr; }
        ZK_TRY(launch_fine_sums(c, d_evals, n, log_blocks, d_out, d_chunk));
        // With the total: coarse sums at the granularity the prover's first rounds want (kept for it in the context's ring), then the
        // total from those.  Without (the deferred form): nothing more here -- the prover derives the coarse sums itself, on the
        // stream of the proof (a high-priority one when the proof is in flight), instead of queueing a tiny kernel on the caller's
        // stream behind whatever streaming pass occupies the chip.
        // (Round 3 tried to have the sums pass deliver the coarse sums too and dropped both forms.  Per-workgroup sums (n / 2048 values)
        // added up by the first serial kernel's prologue: the 8 us kernel and its 6 us launch gap went, the prologue grew by 9 us and the
        // step stayed at 0.334 ms.  The workgroup that finishes LAST under a coarse block adds them up (a device-scope release + counter
        // per workgroup): that release writes the L2 back once per workgroup, 8192 times -- 0.75 ms per step instead of 0.33.)
        if (want_total) {
            const uint32_t k1 = overlapped_plan(n) && log_blocks == log2_exact(n) - 8 ? log_blocks - overlapped_k2(n) : 8;
            int cs = 0;
            ZK_TRY(c->next_coarse(&cs));
            uint64_t* coarse_canon = (uint64_t*)c->d_coarse[cs].get(), *coarse_mont = coarse_canon + 4 * 1024;
            {
                ProfScope ps(c, "coarse_sums", 0.0);
                hipLaunchKernelGGL(group_sums_wg_kernel, dim3(1u << k1), dim3(MLE_BLOCK), 0, c->stream, d_out, 1u << (log_blocks - k1), coarse_mont, coarse_canon);
            }
            {
                ProfScope ps(c, "total_sum", 0.0);
                hipLaunchKernelGGL(group_sums_wg_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, coarse_mont, 1u << k1, d_out + 4 * ((size_t)1 << log_blocks), (uint64_t*)nullptr);
            }
            c->coarse_of[cs] = d_out; c->coarse_n[cs] = n; c->coarse_k1[cs] = k1;
        }
    } else {
        const size_t n_chunks = n / std::min<size_t>(m, 4096);
        uint64_t* d_partials;
        if (n_chunks <= 8 * (size_t)ZK_MAX_PARTIALS) d_partials = c->small_u64(ZK_SMALL_PARTIALS);
        else { ZK_TRY(c->reserve_ws(n_chunks * 32)); d_partials = (uint64_t*)c->ws.ptr; }
        const uint64_t* parts = nullptr;
        const uint32_t group = launch_chunk_sums(c, c->stream, d_evals, n, m, d_partials, &parts);
        hipLaunchKernelGGL(group_sums_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, parts, group, 1u << log_blocks, d_out);
    }
    ZK_HIP(c, hipGetLastError());
    if (h_total) {
        ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_out + 4 * ((size_t)1 << log_blocks), 32, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(h_total, c->pinned_u64(ZK_PIN_RES), 32);
    }
    return ZKHIP_OK;
}

extern "C" int zkhip_mle_block_sums(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint32_t log_blocks,
                                    uint64_t* d_out, uint64_t* h_total) {
    return block_sums_impl(c, d_evals, n, log_blocks, d_out, h_total, true);
}
// The same without the total where it would cost a launch of its own (the fine granularity of the overlapped plan): a prover that
// is going to absorb the TRUE sum gets it from its own sum tree (zkhip_sumcheck_prove with both claimed-sum arguments NULL), and
// zkhip_mle_block_sums_total delivers it to a caller who wants to look at it first.
extern "C" int zkhip_mle_block_sums_deferred(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint32_t log_blocks, uint64_t* d_out) {
    return block_sums_impl(c, d_evals, n, log_blocks, d_out, nullptr, false);
}
extern "C" int zkhip_mle_block_sums_total(zkhip_ctx* c, uint64_t* d_block_sums, uint32_t log_blocks, uint64_t* h_total) {
    if (!c || !d_block_sums || !h_total || log_blocks > 16) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    // two levels: 2^(lb/2) workgroups sum runs of the block sums into the context's scratch, one workgroup adds those
    const uint32_t hi = log_blocks / 2, lo = log_blocks - hi;
    uint64_t* tmp = c->small_u64(ZK_SMALL_PARTIALS);
    hipLaunchKernelGGL(group_sums_wg_kernel, dim3(1u << hi), dim3(MLE_BLOCK), 0, c->stream, d_block_sums, 1u << lo, tmp, (uint64_t*)nullptr);
    hipLaunchKernelGGL(group_sums_wg_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, tmp, 1u << hi, d_block_sums + 4 * ((size_t)1 << log_blocks), (uint64_t*)nullptr);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_block_sums + 4 * ((size_t)1 << log_blocks), 32, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_total, c->pinned_u64(ZK_PIN_RES), 32);
    return ZKHIP_OK;
}

// Where the buffers of one proof lie in its workspace, in field elements: stage tables (n/4 + n/16 + ...; overlapped: n / 2^k1 <= n/8),
// partial sums (chunk sums of stage 0, per-workgroup sums of stage outputs), fold weights, and for the overlapped plan the fine sums
// (n/256 <= 2^16) and two sets of partial tables (<= 2 x 1024 and 32 x 256).  The tables' alignment is part of the measured speed.
struct ProofLayout { size_t tabA, tabB, partA, partB, w, w2, fine, p1, p2, total; };
constexpr ProofLayout proof_layout(size_t n, bool overlap) {
    const size_t part = n / 256 + 1024, w = (size_t)1 << TREE_MAX_LOG;
    ProofLayout l = {};
    l.tabA = 0;
    l.tabB = (overlap ? n / 8 : n / 4) + 32;
    l.partA = (overlap ? n / 8 : n / 4 + n / 16) + 64;
    l.partB = l.partA + part;
    l.w = l.partB + part;
    l.w2 = l.w + w;
    l.fine = l.w2 + w;                                 // overlapped plan only from here on
    l.p1 = l.fine + SC_FINE_ENTRIES;
    l.p2 = l.p1 + SC_P1_ENTRIES;
    l.total = overlap ? l.p2 + SC_P2_ENTRIES : l.fine;
    return l;
}
static_assert(proof_layout((size_t)1 << 24, true).tabB == 2097184 && proof_layout((size_t)1 << 24, true).partA == 2097216 &&
              proof_layout((size_t)1 << 24, true).total == 2230336 + (2 << TREE_MAX_LOG) + 65536 + 2048 + 8192,
              "the bench size's tables have moved");
// One proof in flight: its streams, events and buffers and where its transcript stands.  Plain data: the deferred second half keeps a copy.
struct ProofRun {
    hipStream_t S, F;                        // serial / fold streams
    hipEvent_t fork_ev, serial_ev;
    uint64_t *tabA, *tabB, *partA, *partB, *w, *w2, *fine, *p1, *p2;
    SumcheckDev* st;
    uint64_t *d_rp, *d_ch, *d_fin;
    long long host_delta;                    // the proof leaves through the LAST serial kernel: it writes [sum .. round polynomials] into the pinned slot itself (SmallArgs::host_delta)
    uint64_t seq;                            // ... and then stores `seq` into the slot's sequence word, which the collector spins on (zkhip_ctx::wait_proof)
    uint64_t* seq_word;
    uint32_t round;                          // rounds enqueued so far
    const uint64_t *h_claimed, *d_claimed;   // read by the launch of round 0 only (the host's pointer is the caller's: dead in a deferred half)
    // the next k rounds of the proof, on a working table of 2^k entries
    SmallArgs rounds(const uint64_t* src, uint32_t group, uint32_t stride, uint32_t canon, uint32_t k, uint64_t* weights_out) {
        SmallArgs a = small_rounds(src, group, stride, canon, k, k, round, weights_out);
        small_open(a, round == 0, h_claimed, d_claimed);
        round += k;
        return a;
    }
    // ... which are the last ones
    SmallArgs closing_rounds(const uint64_t* src, uint32_t group, uint32_t stride, uint32_t canon, uint32_t k) {
        SmallArgs a = rounds(src, group, stride, canon, k, nullptr);
        a.final_out = d_fin; a.host_delta = host_delta; a.seq = seq; a.seq_word = seq_word;
        return a;
    }
};
// `lane` < 0: on the caller's stream with the context's buffers (the synchronous call); otherwise on the private streams and buffers of
// c->lanes[lane], behind everything the caller's stream holds at this moment
static int proof_setup(zkhip_ctx* c, size_t n, bool overlap, const uint64_t* h_claimed_sum, const uint64_t* d_claimed_sum, int slot, int lane,
                       ProofRun& p) {
    const ProofLayout l = proof_layout(n, overlap);
    const size_t ws_need = l.total * 32;
    p = {};
    uint64_t *ws, *small;
    if (lane < 0) {
        ZK_TRY(c->reserve_ws(ws_need));
        ws = (uint64_t*)c->ws.ptr; small = (uint64_t*)c->d_small.get(); p.S = c->stream;
        // (The fused launch of fold_rounds_plan uses neither the fold stream nor the events.  The streams are created all the same: the
        // order in which a context's streams come into being decides which hardware queues the lanes of later proofs in flight get.)
        if (overlap) { ZK_TRY(c->ensure_fold_stream()); p.F = c->fold_stream.get(); p.fork_ev = c->fork_ev.get(); p.serial_ev = c->serial_ev.get(); }
    } else {
        ZK_TRY(c->ensure_lane(lane, ws_need));
        zkhip_ctx::ProofLane& L = c->lanes[lane];
        ws = (uint64_t*)L.ws.ptr; small = (uint64_t*)L.small.get(); p.S = L.serial; p.F = L.fold; p.fork_ev = L.fork_ev.get(); p.serial_ev = L.serial_ev.get();
        ZK_HIP(c, hipEventRecord(L.begin_ev.get(), c->stream));          // the table, its block sums and the claimed sum are ready behind this
        ZK_HIP(c, hipStreamWaitEvent(p.S, L.begin_ev.get(), 0));
    }
    p.tabA = ws + 4 * l.tabA; p.tabB = ws + 4 * l.tabB; p.partA = ws + 4 * l.partA; p.partB = ws + 4 * l.partB;
    p.w = ws + 4 * l.w; p.w2 = ws + 4 * l.w2; p.fine = ws + 4 * l.fine; p.p1 = ws + 4 * l.p1; p.p2 = ws + 4 * l.p2;
    p.st = (SumcheckDev*)(small + ZK_SMALL_STATE);
    p.d_rp = small + ZK_SMALL_ROUNDPOLYS;
    p.d_ch = small + ZK_SMALL_CHALLENGES;
    p.d_fin = small + ZK_SMALL_RES;
    ZK_TRY(c->ensure_proof_slot(slot));
    p.host_delta = ((long long)(intptr_t)c->proof_pin[slot].get() - (long long)(intptr_t)(small + ZK_SMALL_STATE)) / 8;
    p.seq = ++c->proof_seq[slot];               // per enqueued proof, never reset: a proof that fails to enqueue just leaves a value nobody stores
    p.seq_word = c->proof_word(slot);
    p.h_claimed = h_claimed_sum; p.d_claimed = d_claimed_sum;
    return ZKHIP_OK;
}
// the overlapped plan's last stage, on the stream that has the big fold's result: the 2^(8 + k2)-entry table folded by k2 variables,
// then the closing eight rounds, which deliver the proof
static int proof_last_stage(zkhip_ctx* c, ProofRun p, hipStream_t stream, uint32_t k2) {
    uint32_t ny = 0;
    ZK_TRY(launch_blockfold(c, stream, p.tabA, 256, k2, p.w2, p.p2, &ny));
    return launch_small(c, p.closing_rounds(p.p2, ny, 256, 1, 8), p.st, p.d_rp, p.d_ch, 0, stream);
}
// The overlapped plan (above stage_k).  *tail: the stream the proof ends on (the caller's may be the null stream: a null pointer says
// nothing).  *held_back: the proof's second half was kept for later (three or more proofs in flight) and records the proof's event itself.
static int proof_overlapped(zkhip_ctx* c, ProofRun& p, const uint64_t* d_evals, size_t n, const uint64_t* d_block_sums, uint32_t log_blocks,
                            int slot, int lane, int in_flight, hipStream_t* tail, bool* held_back) {
    const uint32_t g = log2_exact(n) - 8, k2 = overlapped_k2(n), k1 = g - k2;
    const hipStream_t S = p.S;
    const uint64_t* fine = d_block_sums;
    if (!fine || log_blocks != g) {             // poly_sum() was not called (or with another granularity)
        // three or more proofs in flight: this streaming pass belongs onto the caller's stream like every other one (below); the
        // serial stream follows it
        const bool on_callers = lane >= 0 && in_flight >= 3;
        ZK_TRY(launch_fine_sums(c, d_evals, n, g, p.fine, nullptr, on_callers ? c->stream : S));
        if (on_callers) {
            ZK_HIP(c, hipEventRecord(c->lanes[lane].begin_ev.get(), c->stream));
            ZK_HIP(c, hipStreamWaitEvent(S, c->lanes[lane].begin_ev.get(), 0));
        }
        fine = p.fine;
    }
    // the coarse sums poly_sum() left for this table (the newest ring entry that names its fine sums), or our own
    int cs = -1;
    for (int q = 1; q <= zkhip_ctx::COARSE_RING && cs < 0; ++q) {
        const int e = (c->coarse_next - q + 2 * zkhip_ctx::COARSE_RING) % zkhip_ctx::COARSE_RING;
        if (fine == d_block_sums && c->coarse_of[e] == fine && c->coarse_n[e] == n && c->coarse_k1[e] == k1) cs = e;
    }
    if (cs < 0) {
        ZK_TRY(c->next_coarse(&cs));
        ProfScope ps(c, "coarse_sums", 0.0, S);
        hipLaunchKernelGGL(group_sums_wg_kernel, dim3(1u << k1), dim3(MLE_BLOCK), 0, S, fine, 1u << k2, (uint64_t*)nullptr, (uint64_t*)c->d_coarse[cs].get());
    }
    const uint64_t* coarse = (const uint64_t*)c->d_coarse[cs].get();
    c->coarse_of[cs] = nullptr;                 // the entry belongs to this proof from here on:
    c->coarse_owner[cs] = slot + 1;             // the ring skips it until the proof has been collected (sumcheck_collect / prove_end)
    ZK_TRY(launch_small(c, p.rounds(coarse, 0, 0, 1, k1, p.w), p.st, p.d_rp, p.d_ch, 0, S));
    // fork: the big fold on the fold stream next to rounds k1+1 .. g.  The serial kernel of those rounds asks for
    // (nearly) a whole CU's LDS, so no fold workgroup shares its CU (beside 8+ fold waves per SIMD the transcript
    // wave ran at half speed)
    // The fork comes BEHIND the small fold: the serial kernel (next in this queue) and the big fold (another queue, behind
    // an event) then become ready together and the serial kernel's single workgroup is placed first.  Forked before
    // the small fold, the big fold filled every CU first and the serial kernel waited for one to drain (~60 us).
    uint32_t ny = 0, n_parts = 0;
    ZK_TRY(launch_blockfold(c, S, fine, 1u << k2, k1, p.w, p.p1, &ny));
    if (fold_rounds_plan(n, lane)) {
        // The synchronous proof where the fold has its matrix-core form (2^22 entries and more): no fork at all.  The big fold and the
        // serial rounds beside it are workgroups of ONE launch on the caller's stream (fold_rounds.hpp) -- workgroup 0, dispatched
        // first, is the serial kernel -- and the last stage follows in stream order: no fold stream, no event, no join.
        const SmallArgs fused = p.rounds(p.p1, ny, 1u << k2, 1, k2, p.w2);
        ZK_TRY(launch_fold_rounds(c, S, fused, p.st, p.d_rp, p.d_ch, d_evals, n, k1, p.w, p.tabA));
        *tail = S;
        return proof_last_stage(c, p, S, k2);
    }
    ZK_HIP(c, hipEventRecord(p.fork_ev, S));
    const SmallArgs b = p.rounds(p.p1, ny, 1u << k2, 1, k2, p.w2);
    if (lane >= 0 && in_flight < 3) { ZK_TRY(c->ensure_lane_fold(lane)); p.F = c->lanes[lane].fold; }
    if (lane >= 0 && in_flight >= 3) {
        // Three or more proofs in flight: the streaming passes of ALL of them on ONE stream, the caller's -- where poly_sum() puts the sums
        // passes already.  The big fold and what follows it are enqueued LATER (zkhip_ctx::deferred), behind the sums passes of the next
        // one to three tables, so that the caller's stream never stands waiting for this proof's first rounds; the serial kernel of
        // rounds k1+1 .. g goes out now, the last stage follows the fold on the serial stream.  Measured at 2^24 (profiles/r06/NOTES.md
        // section 7): 0.207 ms per proof with eight in flight against 0.233 with a fold stream per lane.
        ZK_TRY(launch_small(c, b, p.st, p.d_rp, p.d_ch, 156 * 1024, S));
        c->deferred_rc[slot] = ZKHIP_OK;
        const ProofRun held = p;
        c->deferred.emplace_back(slot, [c, held, d_evals, n, k1, k2, slot]() -> int {
            uint32_t np2 = 0;
            ZK_HIP(c, hipStreamWaitEvent(c->stream, held.fork_ev, 0));
            ZK_TRY(launch_multifold(c, c->stream, d_evals, n, k1, held.w, held.tabA, held.partA, &np2));
            ZK_HIP(c, hipEventRecord(held.serial_ev, c->stream));
            ZK_HIP(c, hipStreamWaitEvent(held.S, held.serial_ev, 0));
            ZK_TRY(proof_last_stage(c, held, held.S, k2));
            ZK_HIP(c, hipEventRecord(c->proof_ev[slot].get(), held.S));
            return ZKHIP_OK;
        });
        // how many second halves stay back: enough sums passes in front of a fold that its proof's first rounds are over when its turn
        // comes (1-3 tables), few enough that the host, which stops at its depth, still has passes queued (depth 3 / 4: 1, 5: 2, 6+: 3)
        // (a second half that cannot be enqueued is its OWN proof's failure -- recorded in deferred_rc, reported by that proof's prove_end --
        // not this proof's: this one's second half is in the queue now and the ticket must reach the caller)
        (void)c->flush_deferred((size_t)std::min(3, std::max(1, in_flight - 3)));
        *held_back = true;
        return ZKHIP_OK;
    }
    ZK_HIP(c, hipStreamWaitEvent(p.F, p.fork_ev, 0));
    ZK_TRY(launch_multifold(c, p.F, d_evals, n, k1, p.w, p.tabA, p.partA, &n_parts));
    ZK_TRY(launch_small(c, b, p.st, p.d_rp, p.d_ch, 156 * 1024, S));
    // join ON THE FOLD STREAM: the serial kernel ends well before the big fold, so its event is long set when the fold
    // ends and the last stage follows the fold in stream order (joining on the caller's stream left the chip idle for the
    // ~13 us a cross-stream dependency takes to resolve); the proof is copied from there too
    ZK_HIP(c, hipEventRecord(p.serial_ev, S));
    ZK_HIP(c, hipStreamWaitEvent(p.F, p.serial_ev, 0));
    *tail = p.F;
    return proof_last_stage(c, p, p.F, k2);
}
// The stage plan (stage_k): per stage, the k rounds on partial sums of the table and its fold by their k challenges; the serial kernel
// takes the rest.  All on the serial stream.
static int proof_stages(zkhip_ctx* c, ProofRun& p, const uint64_t* d_evals, size_t n, const uint64_t* d_block_sums, uint32_t log_blocks) {
    const uint64_t* cur = d_evals;
    size_t cn = n;
    const uint64_t* parts = nullptr;   // partial sums of `cur`, `group` consecutive ones per block of this stage
    uint32_t n_parts = 0;
    for (uint32_t stage = 0; stage_k(cn) != 0; ++stage) {
        const uint32_t k = stage_k(cn);
        const size_t m = cn >> k;
        uint32_t group;
        if (stage == 0 && d_block_sums && log_blocks >= k && log_blocks <= (uint32_t)MF_CAP_LOGK) {   // poly_sum() already streamed the table once
            parts = d_block_sums;
            group = 1u << (log_blocks - k);
        } else if (stage == 0) {
            group = launch_chunk_sums(c, p.S, cur, cn, m, p.partA, &parts);   // m >= 256 here
        } else {
            group = (uint32_t)(n_parts >> k);
        }
        ZK_TRY(launch_small(c, p.rounds(parts, group, 0, 0, k, p.w), p.st, p.d_rp, p.d_ch, 0, p.S));
        uint64_t* dst = (stage & 1) ? p.tabB : p.tabA;
        uint64_t* pdst = (stage & 1) ? p.partB : p.partA;
        ZK_TRY(launch_multifold(c, p.S, cur, cn, k, p.w, dst, pdst, &n_parts));
        parts = pdst;
        cur = dst;
        cn = m;
    }
    return launch_small(c, p.closing_rounds(cur, 0, 0, 0, log2_exact(cn)), p.st, p.d_rp, p.d_ch, 0, p.S);
}
// The prover in two halves: sumcheck_enqueue launches every kernel and the copy of the proof into pinned slot `slot`,
// sumcheck_collect waits for that copy (polling its event) and hands the proof out.  A caller with several tables to prove
// begins the next proof before it collects the previous one (zkhip_sumcheck_prove_begin / _end): the kernels of successive
// proofs run in stream order, what disappears is the idle time between them (host wake-up, return, next call's first launch).
static int sumcheck_enqueue(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_claimed_sum,
                            const uint64_t* d_claimed_sum, const uint64_t* d_block_sums, uint32_t log_blocks, int slot, int lane, int in_flight = 1) {
    const bool overlap = overlapped_plan(n);
    ProofRun p;
    ZK_TRY(proof_setup(c, n, overlap, h_claimed_sum, d_claimed_sum, slot, lane, p));
    hipStream_t tail_stream = p.S;            // where the last kernels of the proof run (the overlapped plan ends on its fold stream)
    if (overlap) {
        bool held_back = false;
        ZK_TRY(proof_overlapped(c, p, d_evals, n, d_block_sums, log_blocks, slot, lane, in_flight, &tail_stream, &held_back));
        if (held_back) return ZKHIP_OK;
    } else {
        ZK_TRY(proof_stages(c, p, d_evals, n, d_block_sums, log_blocks));
    }
    // results -> host: written by the last kernel into the pinned slot (no copy launch); the collector polls the event behind it
    // the event the collector polls; the caller's stream stays ordered behind the proof (the next call reuses the scratch)
    ZK_HIP(c, hipEventRecord(c->proof_ev[slot].get(), tail_stream));
    // (a proof on a lane of its own is joined to the caller's stream when it is collected, so that the caller's next poly_sum() does not wait for it)
    if (lane < 0 && tail_stream != c->stream) ZK_HIP(c, hipStreamWaitEvent(c->stream, c->proof_ev[slot].get(), 0));
    return ZKHIP_OK;
}
// by_word: the synchronous call, whose caller waits for THIS proof and nothing else.  A proof in flight is collected by its event as
// before: prove_end joins the caller's stream to the proof right after (hipStreamWaitEvent), and with the event not yet signalled that
// join becomes a real barrier in front of the next tables' streaming passes -- measured, 0.2018 against 0.1969 ms per proof with six
// in flight (profiles/serial_path/NOTES.md).
static int sumcheck_collect(zkhip_ctx* c, int slot, uint32_t n_vars, uint64_t* h_sum, uint64_t* h_round_polys, uint64_t* h_challenges, bool by_word) {
    // The sequence word says the mirror is complete while the last kernel may still be writing its transcript state and final table and
    // its event is not signalled yet.  Nothing below or after this call relies on that kernel being over: the coarse sums were read by
    // the proof's FIRST serial kernel, which the last one follows; the device scratch, the workspace and the mirror are reused in stream
    // order only (the caller's stream waits for proof_ev, a lane's next proof begins behind it, a growing workspace synchronises its
    // streams first), and zkhip_ctx_synchronize / zkhip_ctx_destroy drain the streams themselves.
    const int wrc = by_word ? c->wait_proof(slot) : c->wait_event(c->proof_ev[slot].get());
    c->release_coarse(slot);                    // the proof's kernels are done with their coarse sums (or the device is lost)
    ZK_TRY(wrc);
    const uint64_t* pin = (const uint64_t*)c->proof_pin[slot].get();
    const uint64_t* span = c->small_u64(ZK_SMALL_STATE);
    const SumcheckDev* st = (const SumcheckDev*)c->small_u64(ZK_SMALL_STATE);
    std::memcpy(h_sum, pin + ((const uint64_t*)st->sum - span), 32);
    std::memcpy(h_round_polys, pin + (c->small_u64(ZK_SMALL_ROUNDPOLYS) - span), 64 * (size_t)n_vars);
    std::memcpy(h_challenges, pin + (c->small_u64(ZK_SMALL_CHALLENGES) - span), 32 * (size_t)n_vars);
    return ZKHIP_OK;
}
static int sumcheck_check_args(zkhip_ctx* c, const uint64_t* d_evals, size_t n) {
    if (!c || !d_evals) return ZKHIP_ERR_ARG;
    if (!is_pow2(n)) return ZKHIP_ERR_SHAPE;   // Multilinear::new evaluation_form.rs:16-20
    if (log2_exact(n) > ZK_MAX_ROUNDS) return ZKHIP_ERR_SHAPE;
    return ZKHIP_OK;
}

extern "C" int zkhip_sumcheck_prove(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_claimed_sum,
                                    const uint64_t* d_claimed_sum, const uint64_t* d_block_sums, uint32_t log_blocks,
                                    uint64_t* h_sum,
                                    uint64_t* h_round_polys, uint64_t* h_challenges) {
    ZK_TRY(sumcheck_check_args(c, d_evals, n));
    if (!h_sum) return ZKHIP_ERR_ARG;
    const uint32_t n_vars = log2_exact(n);
    if (n_vars && (!h_round_polys || !h_challenges)) return ZKHIP_ERR_ARG;
    for (int k = 0; k < zkhip_ctx::PROOF_SLOTS; ++k) if (c->proof_pending[k]) return ZKHIP_ERR_BUSY;     // proofs in flight own the result slots
    ZK_TRY(c->activate());
    if (n == 1) {   // no rounds: nothing is proven; report the sum the transcript would have absorbed
        if (h_claimed_sum) { std::memcpy(h_sum, h_claimed_sum, 32); return ZKHIP_OK; }
        ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_claimed_sum ? d_claimed_sum : d_evals, 32, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(h_sum, c->pinned_u64(ZK_PIN_RES), 32);
        return ZKHIP_OK;
    }
    ZK_TRY(sumcheck_enqueue(c, d_evals, n, h_claimed_sum, d_claimed_sum, d_block_sums, log_blocks, 0, -1));
    return sumcheck_collect(c, 0, n_vars, h_sum, h_round_polys, h_challenges, true);
}
// Sumcheck::prove in flight: begin enqueues the whole proof and returns a ticket, end waits for it and delivers the outputs of
// zkhip_sumcheck_prove.  Up to eight proofs of tables with >= 2 entries may be in flight, each on streams and buffers of its own
// (zkhip_ctx::ProofLane): the streaming passes of one run while the transcript rounds of the others hash.
extern "C" int zkhip_sumcheck_prove_begin(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_claimed_sum,
                                          const uint64_t* d_claimed_sum, const uint64_t* d_block_sums, uint32_t log_blocks,
                                          uint32_t* ticket) {
    ZK_TRY(sumcheck_check_args(c, d_evals, n));
    if (!ticket || n < 2) return ZKHIP_ERR_ARG;
    int slot = -1;
    for (int k = 0; k < zkhip_ctx::PROOF_SLOTS; ++k) if (!c->proof_pending[k]) { slot = k; break; }
    if (slot < 0) return ZKHIP_ERR_BUSY;
    ZK_TRY(c->activate());
    int in_flight = 1;
    for (int k = 0; k < zkhip_ctx::PROOF_SLOTS; ++k) in_flight += c->proof_pending[k] != 0;
    ZK_TRY(sumcheck_enqueue(c, d_evals, n, h_claimed_sum, d_claimed_sum, d_block_sums, log_blocks, slot, slot, in_flight));
    c->proof_pending[slot] = log2_exact(n);
    *ticket = (uint32_t)slot;
    return ZKHIP_OK;
}
extern "C" int zkhip_sumcheck_prove_end(zkhip_ctx* c, uint32_t ticket, uint64_t* h_sum, uint64_t* h_round_polys, uint64_t* h_challenges) {
    if (!c || ticket >= (uint32_t)zkhip_ctx::PROOF_SLOTS || !c->proof_pending[ticket]) return ZKHIP_ERR_ARG;
    const uint32_t n_vars = c->proof_pending[ticket];
    int rc = c->activate();
    if (rc == ZKHIP_OK) {
        (void)c->flush_deferred(0, (int)ticket);          // the proof's second half, if it is still held back (and those of the older proofs in front of it)
        rc = c->deferred_rc[ticket];
        c->deferred_rc[ticket] = ZKHIP_OK;
        if (rc != ZKHIP_OK) {                   // the proof never got its last stage: drain what did get out, there is nothing to collect
            (void)hipStreamSynchronize(c->lanes[ticket].serial);
            (void)hipStreamSynchronize(c->stream);
            c->release_coarse((int)ticket);
        }
    }
    if (rc == ZKHIP_OK) {
        if (h_sum && h_round_polys && h_challenges) rc = sumcheck_collect(c, (int)ticket, n_vars, h_sum, h_round_polys, h_challenges, false);
        else { rc = c->wait_event(c->proof_ev[ticket].get()); c->release_coarse((int)ticket); }   // abandoned: just wait it out
        if (hipStreamWaitEvent(c->stream, c->proof_ev[ticket].get(), 0) != hipSuccess && rc == ZKHIP_OK) rc = ZKHIP_ERR_HIP;   // the caller's stream is ordered behind the proof again
    }
    c->proof_pending[ticket] = 0;
    return rc;
}

// ---------------------------------------------------------------------------------------
// a batch of proofs in one launch (sumcheck_batch_kernels.hpp): both provers' batched entry points end here
// ---------------------------------------------------------------------------------------
// Proofs b0 .. of `batch` tables (basic: k = 1, absorb_sum) or table groups (composed), chunk after chunk.  A chunk is one upload
// of its table pointers (and claimed sums), one launch of one workgroup per proof, one copy of all results and one synchronisation.
//   chunk = SCB_CHUNK proofs; with rounds in global memory as many as SCB_SLAB_BYTES of slabs allow, never fewer than SCB_MIN_CHUNK.
// The caller has checked the arguments: n a power of two >= 2, 1 <= k <= 5, k * n <= SCB_MAX_ENTRIES, batch >= 1.
bool zk_sumcheck_batch_serves(uint32_t batch, bool basic, uint32_t k, size_t n) {
    return n >= 2 && (size_t)k * n <= SCB_MAX_ENTRIES && batch >= scb_min_batch(basic, k, n);
}
int zk_sumcheck_batch_run(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_table_ptrs, uint32_t k, size_t n, bool absorb_sum,
                          const uint64_t* h_claimed_sums, uint64_t* h_sums, uint64_t* h_round_polys, uint64_t* h_challenges) {
    if (k < 1 || k > 5 || n < 2 || (size_t)k * n > SCB_MAX_ENTRIES || (absorb_sum && k != 1)) return ZKHIP_ERR_ARG;
    const uint32_t n_vars = log2_exact(n);
    const uint32_t resident_len = scb_resident_len(k, n);
    const size_t slab_per = resident_len < n ? (size_t)k * (n / 2) * 32 : 0;
    const uint32_t bc_max = std::min(batch, scb_chunk(slab_per));
    const uint32_t out_words = scb_out_words(k, n_vars, absorb_sum);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // workspace: [table pointers | claimed sums] (uploaded) [results] [slabs]; pinned: [results] [table pointers | claimed sums]
    const size_t o_claim = al((size_t)bc_max * k * 8), stage_bytes = o_claim + (h_claimed_sums ? al((size_t)bc_max * 32) : 0);
    const size_t out_bytes = al((size_t)bc_max * out_words * 8), o_slab = stage_bytes + out_bytes;
    ZK_TRY(c->reserve_ws(o_slab + (size_t)bc_max * slab_per));
    ZK_TRY(c->reserve_msm_pin(0, out_bytes + stage_bytes));
    char* ws = (char*)c->ws.ptr;
    char* pin = (char*)c->msm_pin[0].ptr;
    void (*fn)(SumcheckBatchArgs) = nullptr;
    switch (k) {
        case 1: fn = absorb_sum ? sumcheck_batch_kernel<1, true> : sumcheck_batch_kernel<1, false>; break;
        case 2: fn = sumcheck_batch_kernel<2, false>; break;
        case 3: fn = sumcheck_batch_kernel<3, false>; break;
        case 4: fn = sumcheck_batch_kernel<4, false>; break;
        default: fn = sumcheck_batch_kernel<5, false>; break;
    }
    const size_t lds = scb_lds_bytes(k, resident_len);
    ZK_TRY(c->allow_big_lds((const void*)fn, lds > 64 * 1024 ? SCB_MAX_LDS_BYTES : lds));   // raised once per kernel, to the family's largest request
    SumcheckBatchArgs a = {};
    a.tables = (const uint64_t* const*)ws;
    a.claimed = h_claimed_sums ? (const uint64_t*)(ws + o_claim) : nullptr;
    a.out = (uint64_t*)(ws + stage_bytes);
    a.slab = (uint64_t*)(ws + o_slab);
    a.n = (uint32_t)n; a.resident_len = resident_len; a.out_words = out_words;
    const int block = scb_block(k, n);
    const size_t rp_words = 4 * (size_t)n_vars * (k + 1), ch_words = 4 * (size_t)n_vars;
    for (uint32_t b0 = 0; b0 < batch; b0 += bc_max) {
        const uint32_t bc = std::min(bc_max, batch - b0);
        // (the previous chunk's upload has ended: every chunk ends in a synchronisation)
        std::memcpy(pin + out_bytes, h_table_ptrs + (size_t)b0 * k, (size_t)bc * k * 8);
        if (h_claimed_sums) std::memcpy(pin + out_bytes + o_claim, h_claimed_sums + 4 * (size_t)b0, (size_t)bc * 32);
        ZK_HIP(c, hipMemcpyAsync(ws, pin + out_bytes, h_claimed_sums ? o_claim + (size_t)bc * 32 : (size_t)bc * k * 8, hipMemcpyHostToDevice, c->stream));
        {
            ProfScope ps(c, "sumcheck_batch", 32.0 * (double)k * (double)n * bc);
            hipLaunchKernelGGL(fn, dim3(bc), dim3(block), lds, c->stream, a);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_HIP(c, hipMemcpyAsync(pin, a.out, (size_t)bc * out_words * 8, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipStreamSynchronize(c->stream));
        for (uint32_t p = 0; p < bc; ++p) {
            const uint64_t* w = (const uint64_t*)pin + (size_t)p * out_words;
            if (absorb_sum) { std::memcpy(h_sums + 4 * (size_t)(b0 + p), w, 32); w += 4; }
            std::memcpy(h_round_polys + (size_t)(b0 + p) * rp_words, w, 8 * rp_words);
            std::memcpy(h_challenges + (size_t)(b0 + p) * ch_words, w + rp_words, 8 * ch_words);
        }
    }
    return ZKHIP_OK;
}

// Sumcheck::prove of `batch` tables of one length (include/zkhip.h).  What the batch kernel does not serve (zk_sumcheck_batch_serves:
// fewer proofs than scb_min_batch, a table of one entry -- no rounds --, tables above SCB_MAX_ENTRIES entries) goes through
// zkhip_sumcheck_prove one after another.
extern "C" int zkhip_sumcheck_prove_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_table_ptrs, size_t n,
                                          const uint64_t* h_claimed_sums, uint64_t* h_sums, uint64_t* h_round_polys, uint64_t* h_challenges) {
    if (!c) return ZKHIP_ERR_ARG;
    if (batch == 0) return ZKHIP_OK;
    if (!h_table_ptrs || !h_sums) return ZKHIP_ERR_ARG;
    for (uint32_t b = 0; b < batch; ++b) ZK_TRY(sumcheck_check_args(c, h_table_ptrs[b], n));
    const uint32_t n_vars = log2_exact(n);
    if (n_vars && (!h_round_polys || !h_challenges)) return ZKHIP_ERR_ARG;
    for (int s = 0; s < zkhip_ctx::PROOF_SLOTS; ++s) if (c->proof_pending[s]) return ZKHIP_ERR_BUSY;     // proofs in flight own the result slots
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;                                                      // a split-phase session holds the workspace
    ZK_TRY(c->activate());
    if (zk_sumcheck_batch_serves(batch, true, 1, n))
        return zk_sumcheck_batch_run(c, batch, h_table_ptrs, 1, n, true, h_claimed_sums, h_sums, h_round_polys, h_challenges);
    auto claimed = [&](uint32_t b) { return h_claimed_sums ? h_claimed_sums + 4 * (size_t)b : nullptr; };
    auto rp = [&](uint32_t b) { return n_vars ? h_round_polys + 8 * (size_t)n_vars * b : nullptr; };
    auto ch = [&](uint32_t b) { return n_vars ? h_challenges + 4 * (size_t)n_vars * b : nullptr; };
    if (batch == 1 || n == 1 || n > SCB_MAX_ENTRIES) {     // one after another
        for (uint32_t b = 0; b < batch; ++b)
            ZK_TRY(zkhip_sumcheck_prove(c, h_table_ptrs[b], n, claimed(b), nullptr, nullptr, 0, h_sums + 4 * (size_t)b, rp(b), ch(b)));
        return ZKHIP_OK;
    }
    // a few proofs of a batchable size: up to PROOF_SLOTS of them in flight, collected in order -- what measured faster than the batch
    // kernel below scb_min_batch proofs, and faster than one after another from two proofs on
    constexpr uint32_t W = (uint32_t)zkhip_ctx::PROOF_SLOTS;
    uint32_t ticket[W], begun = 0, ended = 0;
    int rc = ZKHIP_OK;
    while (begun < batch && rc == ZKHIP_OK) {
        if (begun - ended == W) {
            rc = zkhip_sumcheck_prove_end(c, ticket[ended % W], h_sums + 4 * (size_t)ended, rp(ended), ch(ended));
            ++ended;
            if (rc != ZKHIP_OK) break;
        }
        rc = zkhip_sumcheck_prove_begin(c, h_table_ptrs[begun], n, claimed(begun), nullptr, nullptr, 0, &ticket[begun % W]);
        if (rc == ZKHIP_OK) ++begun;
    }
    for (; ended < begun; ++ended) {       // after an error: the proofs still in flight are waited for and dropped
        const int r = rc == ZKHIP_OK ? zkhip_sumcheck_prove_end(c, ticket[ended % W], h_sums + 4 * (size_t)ended, rp(ended), ch(ended))
                                     : zkhip_sumcheck_prove_end(c, ticket[ended % W], nullptr, nullptr, nullptr);
        if (rc == ZKHIP_OK) rc = r;
    }
    return rc;
}

// ---------------------------------------------------------------------------------------
// split-phase prover for a table sharded over several GPUs
// ---------------------------------------------------------------------------------------
struct zkhip_sc_state {
    zkhip_ctx* c;
    const uint64_t* cur;     // current local table
    size_t cn;               // its length
    uint64_t *A, *B;         // ping-pong buffers (n/2, n/4 entries)
    uint64_t* small;         // [SumcheckDev 64 u64][round polys 8*R][challenges 4*R][partials 8*MLE_MAX_GRID][tail 4*TAIL_N]
    uint32_t round, np;
    bool partials_valid;
    // A/B, small and stage_buf are views: of the context's workspace (ws_loan held; the common, single-state case) or of own_tables, and
    // of the context's cached pair (sc_loan held) or of own_small / own_stage
    DevMem own_tables, own_small, own_stage;
    ZkLoan ws_loan, sc_loan;
    // stage form
    uint64_t* stage_buf;     // [weights 4*512][partials X 4*P][partials Y 4*P][block sums 4*513]
    size_t stage_parts_cap;
    uint32_t stage_k_cur, stage_world, stage_idx, n_parts;
    const uint64_t* parts;
    // overlapped stage (zkhip_sc_overlap_*): scratch inside B -- fine sums, fold weights of both halves, partial tables, local table
    uint32_t ov_k1 = 0, ov_k2 = 0, ov_ny1 = 0, ov_phase = 0;
    uint64_t* ov_fine() { return B; }
    uint64_t* ov_w1() { return B + 4 * SC_FINE_ENTRIES; }
    uint64_t* ov_w2() { return ov_w1() + 4 * ((size_t)1 << TREE_MAX_LOG); }
    uint64_t* ov_p2() { return ov_w2() + 4 * ((size_t)1 << TREE_MAX_LOG); }      // <= 32 x 256
    uint64_t* ov_loc() { return ov_p2() + 4 * SC_P2_ENTRIES; }                   // 256
    uint64_t* sw() { return stage_buf; }
    uint64_t* spx() { return stage_buf + 4 * ((size_t)1 << MF_CAP_LOGK); }
    uint64_t* spy() { return spx() + 4 * stage_parts_cap; }
    uint64_t* sbs() { return spy() + 4 * stage_parts_cap; }
    SumcheckDev* dev() { return (SumcheckDev*)small; }
    uint64_t* rp() { return small + 64; }
    uint64_t* ch() { return rp() + 8 * ZK_MAX_ROUNDS; }
    uint64_t* partials() { return ch() + 4 * ZK_MAX_ROUNDS; }
    uint64_t* fin() { return partials() + 8 * (size_t)MLE_MAX_GRID; }
};

extern "C" int zkhip_sc_begin(zkhip_ctx* c, const uint64_t* d_local, size_t n_local, zkhip_sc_state** out) {
    if (!c || !d_local || !out) return ZKHIP_ERR_ARG;
    if (!is_pow2(n_local)) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    std::unique_ptr<zkhip_sc_state> st(new zkhip_sc_state());      // an error exit releases what the state owns and returns its loans
    st->c = c; st->cur = d_local; st->cn = n_local; st->round = 0; st->np = 0; st->partials_valid = false;
    st->A = st->B = st->small = st->stage_buf = nullptr;
    const size_t small_u64 = 64 + 12 * (size_t)ZK_MAX_ROUNDS + 8 * (size_t)MLE_MAX_GRID + 16;
    st->stage_parts_cap = std::max<size_t>(n_local / 256, 64) + 64;
    if (!c->sc_loans.lent() && c->sc_small && c->sc_stage_cap >= st->stage_parts_cap) {
        st->sc_loan = ZkLoan(c->sc_loans);
        st->stage_parts_cap = c->sc_stage_cap;
    } else {
        if (dev_alloc(st->own_small, small_u64 * 8) != hipSuccess) return ZKHIP_ERR_NOMEM;
        if (dev_alloc(st->own_stage, (((size_t)1 << MF_CAP_LOGK) + 2 * st->stage_parts_cap + ((size_t)1 << MF_CAP_LOGK) + 1 + 8) * 32) != hipSuccess) return ZKHIP_ERR_NOMEM;
    }
    st->small = (uint64_t*)(st->sc_loan ? c->sc_small : st->own_small).get();
    st->stage_buf = (uint64_t*)(st->sc_loan ? c->sc_stage : st->own_stage).get();
    if (n_local >= 2) {
        const size_t bytes = (n_local / 2 + n_local / 4 + 4) * 32;
        if (!c->ws_loans.lent()) {       // steady state: no allocation per prove
            ZK_TRY(c->reserve_ws(bytes));
            st->A = (uint64_t*)c->ws.ptr;
            st->ws_loan = ZkLoan(c->ws_loans);
        } else {                         // several states alive at once (tests drive shards in lockstep)
            if (dev_alloc(st->own_tables, bytes) != hipSuccess) return ZKHIP_ERR_NOMEM;
            st->A = (uint64_t*)st->own_tables.get();
        }
    }
    st->B = st->A ? st->A + 4 * (n_local / 2) : nullptr;
    st->stage_k_cur = 0; st->stage_world = 1; st->stage_idx = 0; st->n_parts = 0; st->parts = nullptr;
    *out = st.release();
    return ZKHIP_OK;
}

// ---- stage form -------------------------------------------------------------------------------------
// The plans are PURE functions of (entries per shard, world): a rank that failed -- possibly before it had a state at all -- still
// walks the exchange schedule of the protocol with them (shard_protocol.hpp, "a failing rank must not hang its peers").
int zk_sc_plan_stage(size_t cn, uint32_t world, uint32_t* k_out) {
    if (!k_out || !is_pow2(world) || !is_pow2(cn)) return ZKHIP_ERR_ARG;
    uint32_t k;
    if (world == 1) {
        k = stage_k(cn);                        // the single-GPU plan
    } else {
        // Every stage costs an exchange: use as few as the kernels allow (<= MF_CAP_LOGK variables per stage, the
        // gathered tail takes zkhip_sc_tail_capacity() entries) and spread the variables evenly over them.
        const uint32_t lg = log2_exact(cn * world);
        const uint32_t tail_log = log2_exact((size_t)zkhip_sc_tail_capacity());
        if (lg <= tail_log) k = 0;
        else {
            const uint32_t need = lg - tail_log;
            const uint32_t stages = (need + MF_CAP_LOGK - 1) / MF_CAP_LOGK;
            k = std::max<uint32_t>((need + stages - 1) / stages, 3);   // a stage folds at least 3 variables (overshooting the tail size is fine)
        }
    }
    while (k && (cn >> k) < 16) --k;           // the local k-variable fold needs >= 16 outputs per workgroup
    if (k < 3) k = 0;                           // too little left: gather the tables and finish replicated
    *k_out = k;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_stage_plan(zkhip_sc_state* st, uint32_t world, uint32_t* k_out) {
    if (!st || !k_out || !is_pow2(world)) return ZKHIP_ERR_ARG;
    uint32_t k = 0;
    ZK_TRY(zk_sc_plan_stage(st->cn, world, &k));
    st->stage_k_cur = k;
    st->stage_world = world;
    *k_out = k;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_stage_block_sums(zkhip_sc_state* st, uint64_t* d_out) {
    if (!st || !d_out || st->stage_k_cur == 0) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    const uint32_t k = st->stage_k_cur;
    const size_t m = st->cn >> k;
    if (st->stage_idx == 0) {
        const uint64_t* parts = nullptr;
        const uint32_t group = launch_chunk_sums(c, c->stream, st->cur, st->cn, m, st->spx(), &parts);
        hipLaunchKernelGGL(group_sums_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, parts, group, 1u << k, st->sbs());
    } else {
        hipLaunchKernelGGL(group_sums_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, st->parts, st->n_parts >> k, 1u << k, st->sbs());
    }
    ZK_HIP(c, hipMemcpyAsync(d_out, st->sbs(), 32 * ((size_t)1 << k), hipMemcpyDeviceToDevice, c->stream));
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_stage_absorb(zkhip_sc_state* st, const uint64_t* d_gathered, uint32_t world, const uint64_t* h_claimed) {
    if (!st || !d_gathered || st->stage_k_cur == 0 || world != st->stage_world) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    const uint32_t k = st->stage_k_cur;
    SmallArgs a = small_rounds(d_gathered, world, 1u << k, 0, k, k, st->round, st->sw());
    small_open(a, st->round == 0, h_claimed, nullptr);
    ZK_TRY(launch_small(c, a, st->dev(), st->rp(), st->ch()));
    st->round += k;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_stage_fold(zkhip_sc_state* st) {
    if (!st || st->stage_k_cur == 0) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    const uint32_t k = st->stage_k_cur;
    const size_t m = st->cn >> k;
    uint64_t* dst = (st->cur == st->A) ? st->B : st->A;     // m <= n_local/8 fits either buffer
    uint64_t* pdst = (st->parts == st->spx() || st->stage_idx == 0) ? st->spy() : st->spx();
    uint32_t n_parts = 0;
    ZK_TRY(launch_multifold(c, c->stream, st->cur, st->cn, k, st->sw(), dst, pdst, &n_parts));
    st->parts = pdst;
    st->n_parts = n_parts;
    st->cur = dst;
    st->cn = m;
    st->partials_valid = false;
    st->stage_k_cur = 0;
    st->stage_idx++;
    return ZKHIP_OK;
}
// ---- overlapped stage: the single-GPU plan of 2^19..2^24-entry tables (sumcheck_enqueue) in exchange form --------------
// The local shard is summed once at FINE_CHUNK granularity.  Exchange 1 carries the 2^k1 coarse sums (k1 rounds on them,
// replicated); the fine sums folded by those k1 variables are the block sums of the next k2 rounds, exchange 2 carries them
// while the k1-variable fold of the shard runs on the context's fold stream; after the k2 rounds the fold's output is folded
// by the k2 variables into a 256-entry local table (gathered by the caller for the last rounds).  Three exchanges in all,
// as in the plain stage form, with the big fold hidden behind the second one and the serial kernel of the k2 rounds.
int zk_sc_plan_overlap(size_t cn, uint32_t world, uint32_t* k1, uint32_t* k2, uint32_t* mid_entries, uint32_t* ny_out) {
    if (!k1 || !k2 || !mid_entries || !is_pow2(world)) return ZKHIP_ERR_ARG;
    *k1 = *k2 = *mid_entries = 0;
    if (ny_out) *ny_out = 0;
    if (!overlapped_shard(cn)) return ZKHIP_OK;
    if ((size_t)256 * world > (size_t)zkhip_sc_tail_capacity()) return ZKHIP_OK;      // the gathered 256-entry tables must fit the tail
    const uint32_t g = log2_exact(cn) - 8;
    const uint32_t ov_k2 = overlapped_k2(cn), ov_k1 = g - ov_k2;
    BlockfoldShape sh;
    if (!blockfold_shape(1u << ov_k2, ov_k1, &sh)) return ZKHIP_ERR_SHAPE;
    *k1 = ov_k1; *k2 = ov_k2; *mid_entries = sh.ny << ov_k2;
    if (ny_out) *ny_out = sh.ny;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_overlap_plan(zkhip_sc_state* st, uint32_t world, uint32_t* k1, uint32_t* k2, uint32_t* mid_entries) {
    if (!st || !k1 || !k2 || !mid_entries || !is_pow2(world)) return ZKHIP_ERR_ARG;
    *k1 = *k2 = *mid_entries = 0;
    if (st->round != 0 || st->stage_idx != 0 || st->ov_phase != 0) return ZKHIP_OK;
    uint32_t ny = 0;
    ZK_TRY(zk_sc_plan_overlap(st->cn, world, k1, k2, mid_entries, &ny));
    if (!*k1) return ZKHIP_OK;
    st->ov_k1 = *k1; st->ov_k2 = *k2; st->ov_ny1 = ny;
    st->stage_world = world;
    return ZKHIP_OK;
}
// d_out: the 2^k1 coarse block sums of the local shard (canonical integers; they add up across ranks all the same)
extern "C" int zkhip_sc_overlap_sums(zkhip_sc_state* st, uint64_t* d_out) {
    if (!st || !d_out || st->ov_k1 == 0 || st->ov_phase != 0) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    const uint32_t g = st->ov_k1 + st->ov_k2;
    ZK_TRY(launch_fine_sums(c, st->cur, st->cn, g, st->ov_fine(), nullptr));
    hipLaunchKernelGGL(group_sums_wg_kernel, dim3(1u << st->ov_k1), dim3(MLE_BLOCK), 0, c->stream, st->ov_fine(), 1u << st->ov_k2, (uint64_t*)nullptr, d_out);
    ZK_HIP(c, hipGetLastError());
    st->ov_phase = 1;
    return ZKHIP_OK;
}
// d_gathered: [world][2^k1] coarse sums in rank order.  Runs rounds 1..k1, starts the k1-variable fold of the shard on the fold
// stream and leaves this rank's partial block sums of the next k2 rounds in d_mid (mid_entries values).
extern "C" int zkhip_sc_overlap_rounds1(zkhip_sc_state* st, const uint64_t* d_gathered, uint32_t world, const uint64_t* h_claimed, uint64_t* d_mid) {
    if (!st || !d_gathered || !d_mid || st->ov_phase != 1 || world != st->stage_world) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    ZK_TRY(c->ensure_fold_stream());
    const uint32_t k1 = st->ov_k1, k2 = st->ov_k2;
    SmallArgs a = small_rounds(d_gathered, world, 1u << k1, 1, k1, k1, 0, st->ov_w1());
    small_open(a, true, h_claimed, nullptr);
    ZK_TRY(launch_small(c, a, st->dev(), st->rp(), st->ch()));
    uint32_t ny = 0, n_parts = 0;
    ZK_TRY(launch_blockfold(c, c->stream, st->ov_fine(), 1u << k2, k1, st->ov_w1(), d_mid, &ny));
    if (ny != st->ov_ny1) return ZKHIP_ERR_SHAPE;
    ZK_HIP(c, hipEventRecord(c->fork_ev.get(), c->stream));
    ZK_HIP(c, hipStreamWaitEvent(c->fold_stream.get(), c->fork_ev.get(), 0));
    ZK_TRY(launch_multifold(c, c->fold_stream.get(), st->cur, st->cn, k1, st->ov_w1(), st->A, st->spx(), &n_parts));
    ZK_HIP(c, hipEventRecord(c->join_ev.get(), c->fold_stream.get()));
    st->round = k1;
    st->ov_phase = 2;
    return ZKHIP_OK;
}
// d_gathered: [world][mid_entries].  Runs rounds k1+1..k1+k2 beside the fold, joins it and folds its output by the k2
// variables: the local table is 256 entries afterwards (zkhip_sc_local_table).
extern "C" int zkhip_sc_overlap_rounds2(zkhip_sc_state* st, const uint64_t* d_gathered, uint32_t world) {
    if (!st || !d_gathered || st->ov_phase != 2 || world != st->stage_world) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    const uint32_t k1 = st->ov_k1, k2 = st->ov_k2;
    const SmallArgs b = small_rounds(d_gathered, world * st->ov_ny1, 1u << k2, 1, k2, k2, k1, st->ov_w2());
    // no exclusive-CU request here (cf. sumcheck_enqueue): the exchange puts this launch tens of microseconds behind the fold's
    // start, the chip is full by then and a whole free CU only appears when the fold drains
    ZK_TRY(launch_small(c, b, st->dev(), st->rp(), st->ch()));
    ZK_HIP(c, hipStreamWaitEvent(c->stream, c->join_ev.get(), 0));
    uint32_t ny = 0;
    ZK_TRY(launch_blockfold(c, c->stream, st->A, 256, k2, st->ov_w2(), st->ov_p2(), &ny));
    if (ny > 32) return ZKHIP_ERR_SHAPE;
    hipLaunchKernelGGL(slice_sums_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, st->ov_p2(), ny, 256u, st->ov_loc());
    ZK_HIP(c, hipGetLastError());
    st->cur = st->ov_loc();
    st->cn = 256;
    st->round = k1 + k2;
    st->partials_valid = false;
    st->stage_idx++;
    st->ov_phase = 3;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_local_len(zkhip_sc_state* st, size_t* n) {
    if (!st || !n) return ZKHIP_ERR_ARG;
    *n = st->cn;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_local_half_sums(zkhip_sc_state* st, uint64_t* d_out) {
    if (!st || !d_out) return ZKHIP_ERR_ARG;
    if (st->cn < 2) return ZKHIP_ERR_SHAPE;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    if (!st->partials_valid) {   // first round (later rounds: the fold already produced them)
        const int grid = mle_grid((st->cn + 3) / 4);
        ProfScope ps(c, "half_sums", 32.0 * (double)st->cn);
        hipLaunchKernelGGL(half_sums_kernel, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, st->cur, st->cn, st->partials());
        st->np = (uint32_t)grid;
    }
    hipLaunchKernelGGL(finish_sums_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, st->partials(), st->np, st->fin());
    ZK_HIP(c, hipMemcpyAsync(d_out, st->fin(), 64, hipMemcpyDeviceToDevice, c->stream));
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_absorb(zkhip_sc_state* st, const uint64_t* d_gathered, uint32_t world, const uint64_t* h_claimed) {
    if (!st || !d_gathered || world == 0) return ZKHIP_ERR_ARG;
    if (st->round >= ZK_MAX_ROUNDS) return ZKHIP_ERR_SHAPE;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    FrArg z = {};
    SmallArgs o = {};                           // (carries `first` and the claimed sum only)
    small_open(o, st->round == 0, h_claimed, nullptr);
    hipLaunchKernelGGL(sumcheck_round_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, d_gathered, world, st->dev(), st->round,
                       o.first, o.claimed, 0u, z, z, st->rp(), st->ch());
    ZK_HIP(c, hipGetLastError());
    st->round++;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_fold(zkhip_sc_state* st) {
    if (!st) return ZKHIP_ERR_ARG;
    if (st->cn < 2 || st->round == 0) return ZKHIP_ERR_SHAPE;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    uint64_t* dst = (st->cur == st->A) ? st->B : st->A;
    const bool sums = st->cn >= 4;   // the folded table still has two halves to sum
    ZK_TRY(launch_fold(c, st->cur, st->cn, st->ch() + 4 * (st->round - 1), nullptr, 0, dst, sums, st->partials(), &st->np));
    st->partials_valid = sums;
    st->cur = dst;
    st->cn /= 2;
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_local_value(zkhip_sc_state* st, uint64_t* d_out) {
    if (!st || !d_out) return ZKHIP_ERR_ARG;
    if (st->cn != 1) return ZKHIP_ERR_SHAPE;
    ZK_HIP(st->c, hipMemcpyAsync(d_out, st->cur, 32, hipMemcpyDeviceToDevice, st->c->stream));
    return ZKHIP_OK;
}
extern "C" int zkhip_sc_local_table(zkhip_sc_state* st, uint64_t* d_out) {
    if (!st || !d_out) return ZKHIP_ERR_ARG;
    ZK_HIP(st->c, hipMemcpyAsync(d_out, st->cur, 32 * st->cn, hipMemcpyDeviceToDevice, st->c->stream));
    return ZKHIP_OK;
}
// The gathered table may be twice what the serial kernel holds: its first round then runs on its own (half sums, transcript,
// fold: four small launches) -- cheaper than one more round of the exchange protocol.
extern "C" int zkhip_sc_tail_capacity(void) { return 2 << TREE_MAX_LOG; }
extern "C" int zkhip_sc_tail(zkhip_sc_state* st, const uint64_t* d_values, uint32_t m, const uint64_t* h_claimed) {
    if (!st || !d_values) return ZKHIP_ERR_ARG;
    if (!is_pow2(m) || m > (2u << TREE_MAX_LOG)) return ZKHIP_ERR_SHAPE;
    if (m == 1) return ZKHIP_OK;
    zkhip_ctx* c = st->c;
    ZK_TRY(c->activate());
    if (m > (1u << TREE_MAX_LOG)) {
        if (st->round >= ZK_MAX_ROUNDS) return ZKHIP_ERR_SHAPE;
        FrArg z = {};
        SmallArgs o = {};                       // (carries `first` and the claimed sum only)
        small_open(o, st->round == 0, h_claimed, nullptr);
        const int grid = mle_grid((m + 3) / 4);
        uint64_t* folded = st->partials() + 64;              // m/2 entries behind the two records of half sums
        hipLaunchKernelGGL(half_sums_kernel, dim3(grid), dim3(MLE_BLOCK), 0, c->stream, d_values, (size_t)m, st->partials());
        hipLaunchKernelGGL(sumcheck_round_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, st->partials(), (uint32_t)grid, st->dev(), st->round,
                           o.first, o.claimed, 0u, z, z, st->rp(), st->ch());
        ZK_TRY(launch_fold(c, d_values, m, st->ch() + 4 * st->round, nullptr, 0, folded, false, nullptr, nullptr));
        st->round++;
        d_values = folded;
        m >>= 1;
    }
    const uint32_t lg = log2_exact(m);
    SmallArgs a = small_rounds(d_values, 0, 0, 0, lg, lg, st->round, nullptr);
    small_open(a, st->round == 0, h_claimed, nullptr);
    a.final_out = st->fin();
    ZK_TRY(launch_small(c, a, st->dev(), st->rp(), st->ch()));
    st->round += a.log_n;
    return ZKHIP_OK;
}
// ends a state: its loans go back, and its own small / stage pair goes to the context's cache or away
static void sc_release(zkhip_sc_state* raw) {
    std::unique_ptr<zkhip_sc_state> st(raw);
    zkhip_ctx* c = st->c;
    if (st->sc_loan) return;
    // the first finished state's set is kept for the next prove instead of being freed; and when the cached set (not in use) is too small
    // for shards of this size (a steady stream of them would allocate and free per prove) this larger set replaces it.  (The caller has
    // waited for the stream: finish / abort synchronise before they release.)
    if (!c->sc_small || (!c->sc_loans.lent() && st->stage_parts_cap > c->sc_stage_cap)) {
        c->sc_small = std::move(st->own_small); c->sc_stage = std::move(st->own_stage); c->sc_stage_cap = st->stage_parts_cap;
    }
}
extern "C" int zkhip_sc_finish(zkhip_sc_state* st, uint64_t* h_sum, uint64_t* h_rp, uint64_t* h_ch, uint32_t* n_rounds) {
    if (!st) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    int rc = ZKHIP_OK;
    if (c->activate() != ZKHIP_OK) rc = ZKHIP_ERR_HIP;
    // one copy of [state | round polynomials | challenges] (contiguous in `small`) into pinned memory
    const size_t span = 64 + 12 * (size_t)ZK_MAX_ROUNDS;
    static_assert(ZK_PIN_END - ZK_PIN_PROOF >= 64 + 12 * ZK_MAX_ROUNDS, "pinned proof area too small");
    uint64_t* pin = c->pinned_u64(ZK_PIN_PROOF);
    if (rc == ZKHIP_OK && hipMemcpyAsync(pin, st->small, 8 * span, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = ZKHIP_ERR_HIP;
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc = ZKHIP_ERR_HIP;
    if (st->ov_phase == 2 && c->fold_stream.get() && hipStreamSynchronize(c->fold_stream.get()) != hipSuccess) rc = ZKHIP_ERR_HIP;   // un-joined fold (see zkhip_sc_abort)
    if (rc == ZKHIP_OK) {
        if (h_sum) std::memcpy(h_sum, pin + ((const uint64_t*)st->dev()->sum - st->small), 32);
        if (h_rp && st->round) std::memcpy(h_rp, pin + 64, 64 * (size_t)st->round);
        if (h_ch && st->round) std::memcpy(h_ch, pin + 64 + 8 * ZK_MAX_ROUNDS, 32 * (size_t)st->round);
    }
    if (n_rounds) *n_rounds = st->round;
    sc_release(st);
    return rc;
}
extern "C" int zkhip_sc_abort(zkhip_sc_state* st) {
    if (!st) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = st->c;
    int rc = ZKHIP_OK;
    if (c->activate() != ZKHIP_OK || hipStreamSynchronize(c->stream) != hipSuccess) rc = ZKHIP_ERR_HIP;   // kernels may still read the buffers
    // between zkhip_sc_overlap_rounds1 and _rounds2 the shard's k1-variable fold runs on the fold stream and is joined to
    // c->stream only inside _rounds2: an abort in that window must wait for it too (it reads the caller's table and writes the
    // workspace and the cached stage buffer that sc_release hands back)
    if (c->fold_stream.get() && hipStreamSynchronize(c->fold_stream.get()) != hipSuccess) rc = ZKHIP_ERR_HIP;
    sc_release(st);
    return rc;
}

// ---- FiatShamirTranscript on bytes of the caller's choice (the device hash held against an independent SHA-256) ----
namespace zk {
static __global__ __launch_bounds__(64) void transcript_blocks_kernel(const uint32_t* __restrict__ blocks, uint32_t n_blocks, uint32_t* __restrict__ digest) {
    __shared__ uint32_t kw[64];
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    for (uint32_t b = 0; b < n_blocks; ++b) {
        uint32_t blk[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) blk[j] = blocks[16 * (size_t)b + j];
        sha256_compress_wave(h, blk, kw);
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) digest[i] = h[i];
    }
}
}  // namespace zk
extern "C" int zkhip_transcript_challenge(zkhip_ctx* c, const uint8_t* h_prefix32, const uint8_t* h_bytes, size_t n, uint8_t* h_digest32) {
    if (!c || !h_digest32 || (n && !h_bytes)) return ZKHIP_ERR_ARG;
    if (n >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    // the padded message as big-endian words (FIPS 180-4 5.1.1): prefix || bytes || 0x80 || 0 ... || bit length
    const size_t len = (h_prefix32 ? 32 : 0) + n, n_blocks = (len + 9 + 63) / 64;
    std::vector<uint8_t> msg(64 * n_blocks, 0);
    if (h_prefix32) std::memcpy(msg.data(), h_prefix32, 32);
    if (n) std::memcpy(msg.data() + (h_prefix32 ? 32 : 0), h_bytes, n);
    msg[len] = 0x80;
    const uint64_t bits = 8 * (uint64_t)len;
    for (int i = 0; i < 8; ++i) msg[64 * n_blocks - 1 - i] = (uint8_t)(bits >> (8 * i));
    std::vector<uint32_t> words(16 * n_blocks);
    for (size_t w = 0; w < words.size(); ++w)
        words[w] = ((uint32_t)msg[4 * w] << 24) | ((uint32_t)msg[4 * w + 1] << 16) | ((uint32_t)msg[4 * w + 2] << 8) | msg[4 * w + 3];
    ZK_TRY(c->reserve_ws(4 * words.size() + 64));
    uint32_t* d_words = (uint32_t*)c->ws.ptr;
    uint32_t* d_digest = d_words + words.size();
    ZK_HIP(c, hipMemcpyAsync(d_words, words.data(), 4 * words.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(zk::transcript_blocks_kernel, dim3(1), dim3(64), 0, c->stream, (const uint32_t*)d_words, (uint32_t)n_blocks, d_digest);
    ZK_HIP(c, hipGetLastError());
    uint32_t out[8];
    ZK_HIP(c, hipMemcpyAsync(out, d_digest, 32, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 4; ++j) h_digest32[4 * i + j] = (uint8_t)(out[i] >> (24 - 8 * j));
    return ZKHIP_OK;
}

#ifdef ZK_STAMPS
extern "C" int zkhip_debug_read_stamps(zkhip_ctx* c, unsigned long long* h_out /*64*8*/) {
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    ZK_HIP(c, hipMemcpyFromSymbol(h_out, HIP_SYMBOL(zk::g_zk_stamps), 64 * 8 * 8));
    return ZKHIP_OK;
}
#endif
