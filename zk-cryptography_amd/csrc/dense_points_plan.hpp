// dense_points_plan.hpp -- what zkhip_dense_points (ntt.hip) decides on the host before it enqueues anything: how a job's inner range
// is cut into segments so that a call with few points still fills the chip, how a batch of interpolations is cut into chunks of jobs,
// the grids, and the layout of the call's scratch (an allocation of the context's own, never its workspace).  Functions of
// (op, batch, n_in, n_x) alone: the entry point, its kernels (dense_points_kernels.hpp), zkhip_dense_points_plan_info and
// tests/cpp/dense_points_plan_check.cpp share this one definition.  No HIP in here.
//
// Both ops are an O(inner x points) loop that is private to a lane: a lane owns one POINT and walks the INNER range.
//   EVALUATE     points = the n_x arguments of a job, inner = its n_in coefficients.  Grid (point blocks, segments, jobs): a workgroup
//                stages its segment of the coefficients in LDS, DP_CHUNK at a time from the top down, and every lane runs Horner for its
//                own point.  With S > 1 segments a lane scales its value by x^(seg * seg_len) and stores a record; a second launch adds
//                a point's S records.  Field addition is exact: the cut changes no limb.
//   INTERPOLATE  inner = the n nodes of a job, in three stages per chunk of jobs:
//                1. weights: points = the n nodes; lane i forms D_i = prod_{j != i} (x_i - x_j) over its segment, the segments'
//                   partial products are multiplied, and 1 / D_i is stored (D_i == 0 raises the call's flag);
//                2. domain values: points = the N = 2^ceil(log2 n) powers of the domain's generator; from (Num, Den) = (0, 1) a lane
//                   takes Num <- Num (z - x_i) + s_i Den, Den <- Den (z - x_i) over its segment's nodes, s_i = y_i / D_i; segments
//                   A then B combine as (Num_A Den_B + Num_B Den_A, Den_A Den_B).  After the last node Num = P(z), without a division;
//                3. one batched inverse transform of the N values per job keeps the first n coefficients.
//
// The tunables below -- lanes, the staged chunk and the rule that picks S -- are recorded with what was measured and what was not in
// profiles/dense_points/NOTES.md ("Tunables").
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zk {

constexpr uint32_t DP_LANES = 256;            // lanes of a workgroup = points of a point block (NOTES "Tunables": not compared with 512 or 1024)
constexpr uint32_t DP_CHUNK = 256;            // inner elements staged in LDS at a time: one per lane, 8 KiB (16 KiB with the nodes' s_i beside them)
constexpr uint32_t DP_TARGET_WGS = 512;       // a first launch with fewer workgroups than this is cut into segments: two per CU of the 256
constexpr uint32_t DP_MAX_SEGS = 64;          // records a point's combine walks at most
constexpr uint32_t DP_MAX_BATCH = 65535;      // jobs of a call: the grid's third dimension
constexpr uint32_t DP_MAX_GRID_X = 65536;     // point blocks of a launch; a workgroup strides over the rest
constexpr size_t DP_MAX_N = (size_t)1 << 40;  // coefficients or points of a job: far beyond the device's memory, and no product below overflows
constexpr uint32_t DP_INTERP_MAX_LOG = 14;   // interpolation: n <= 2^14 (beyond that a product tree is the right tool)
constexpr size_t DP_INTERP_MAX = (size_t)1 << DP_INTERP_MAX_LOG;
constexpr uint32_t DP_NTT_WORK_LOG = 12;      // from 2^12 points the inverse transform runs in passes and needs a work buffer per job
constexpr size_t DP_SCRATCH_BYTES = (size_t)256 << 20;   // what a chunk of interpolations may hold before its records (ntt.hip's bound for its own batches)

enum DpOp : int { DP_OP_EVALUATE = 0, DP_OP_INTERPOLATE = 1 };
enum DpRegime : uint32_t { DP_NOOP = 0, DP_EVALUATE = 1, DP_INTERPOLATE = 2, DP_REFUSED = 3 };

constexpr size_t dp_align(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr size_t dp_ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }
constexpr uint32_t dp_log2_ceil(size_t n) {
    uint32_t l = 0;
    while (((size_t)1 << l) < n) ++l;
    return l;
}

struct DpPlan {
    DpRegime regime;
    uint32_t batch;
    size_t n_inner;                  // coefficients (evaluate) or nodes (interpolate) of a job
    size_t n_points;                 // lanes of the widest first launch per job: n_x (evaluate) or N (interpolate, stage 2)
    uint32_t log_N;                  // interpolate: log2 of the transform domain; 0 otherwise
    uint32_t segs;                   // S: segments of the inner range, >= 1
    size_t seg_len;                  // inner elements of a segment but the last: a multiple of DP_CHUNK
    uint32_t lanes;                  // DP_LANES
    uint32_t grid_x;                 // point blocks of the widest launch, capped at DP_MAX_GRID_X
    uint32_t chunk, n_chunks;        // jobs per launch chain and chains: evaluate runs the batch as one
    uint32_t launches;               // per chunk (interpolate: with nodes of the job's own; shared nodes run stage 1 once per call)
    // the scratch: [flag][1 / D_i][stage-1 records][stage-2 records or evaluate's records][domain values][transform work]
    size_t o_flag, o_winv, o_rec1, o_rec2, o_vals, o_work, scratch_bytes;
};

// segment s of the inner range: [first, first + count)
struct DpSeg { size_t first, count; };
constexpr DpSeg dp_seg(const DpPlan& p, uint32_t s) {
    const size_t first = (size_t)s * p.seg_len;
    const size_t left = first < p.n_inner ? p.n_inner - first : 0;
    return {first, left < p.seg_len ? left : p.seg_len};
}
// chunk i of the batch: jobs [first, first + count)
struct DpChunk { uint32_t first, count; };
constexpr DpChunk dp_chunk(const DpPlan& p, uint32_t i) {
    const uint32_t first = i * p.chunk;
    return {first, p.batch - first < p.chunk ? p.batch - first : p.chunk};
}

// S and the segment length for `wgs` workgroups of a first launch without a cut
constexpr void dp_cut(DpPlan& p, size_t wgs) {
    const size_t chunks = dp_ceil_div(p.n_inner, DP_CHUNK);
    size_t want = wgs >= DP_TARGET_WGS ? 1 : dp_ceil_div(DP_TARGET_WGS, wgs ? wgs : 1);
    if (want > DP_MAX_SEGS) want = DP_MAX_SEGS;
    if (want > chunks) want = chunks;
    if (want < 1) want = 1;
    const size_t per = chunks ? dp_ceil_div(chunks, want) : 0;           // staged chunks of a segment
    p.seg_len = per * DP_CHUNK;
    p.segs = per ? (uint32_t)dp_ceil_div(chunks, per) : 1u;               // no empty segment
}

// DP_REFUSED: ZKHIP_ERR_SHAPE (too many jobs; interpolation with n_in != n_x or more than 2^14 nodes).  DP_NOOP: nothing to do.
constexpr DpPlan dp_plan(int op, uint32_t batch, size_t n_in, size_t n_x) {
    DpPlan p = {};
    p.batch = batch;
    p.lanes = DP_LANES;
    p.segs = 1;
    if ((op != DP_OP_EVALUATE && op != DP_OP_INTERPOLATE) || batch > DP_MAX_BATCH || n_in > DP_MAX_N || n_x > DP_MAX_N ||
        (op == DP_OP_INTERPOLATE && (n_in != n_x || n_x > DP_INTERP_MAX))) {
        p.regime = DP_REFUSED;
        return p;
    }
    if (batch == 0 || n_x == 0) return p;                                  // DP_NOOP
    p.n_inner = n_in;
    p.o_flag = 0;
    p.o_winv = dp_align(4);
    if (op == DP_OP_EVALUATE) {
        p.regime = DP_EVALUATE;
        p.n_points = n_x;
        p.chunk = batch;
        p.n_chunks = 1;
        const size_t blocks = dp_ceil_div(n_x, DP_LANES);
        p.grid_x = (uint32_t)(blocks < DP_MAX_GRID_X ? blocks : DP_MAX_GRID_X);
        dp_cut(p, blocks * batch);
        p.launches = p.segs > 1 ? 2u : 1u;
        p.o_rec1 = p.o_rec2 = p.o_winv;
        const size_t rec = p.segs > 1 ? dp_align((size_t)batch * p.segs * n_x * 32) : 0;
        p.o_vals = p.o_work = p.scratch_bytes = p.o_rec2 + rec;
        return p;
    }
    p.regime = DP_INTERPOLATE;
    p.log_N = dp_log2_ceil(n_x);
    const size_t N = (size_t)1 << p.log_N;
    const bool work = p.log_N >= DP_NTT_WORK_LOG;
    p.n_points = N;
    const size_t per_job = 32 * (n_x + N + (work ? N : 0));
    const size_t fit = DP_SCRATCH_BYTES / per_job ? DP_SCRATCH_BYTES / per_job : 1;
    p.chunk = (uint32_t)(batch < fit ? batch : fit);
    p.n_chunks = (batch + p.chunk - 1) / p.chunk;
    const size_t blocks = dp_ceil_div(N, DP_LANES);
    p.grid_x = (uint32_t)blocks;                                           // <= 2^14 / 256
    dp_cut(p, blocks * p.chunk);
    const uint32_t ntt = !work ? 1u : 1u + (p.log_N - 8 + 6) / 7;          // ntt.hip: one launch up to 2^11, the first eight stages and passes of <= 7 beyond
    p.launches = (p.segs > 1 ? 4u : 2u) + ntt;
    p.o_rec1 = p.o_winv + dp_align((size_t)p.chunk * n_x * 32);
    p.o_rec2 = p.o_rec1 + (p.segs > 1 ? dp_align((size_t)p.chunk * p.segs * n_x * 32) : 0);
    p.o_vals = p.o_rec2 + (p.segs > 1 ? dp_align((size_t)p.chunk * p.segs * N * 64) : 0);
    p.o_work = p.o_vals + dp_align((size_t)p.chunk * N * 32);
    p.scratch_bytes = p.o_work + (work ? dp_align((size_t)p.chunk * N * 32) : 0);
    return p;
}

// the words zkhip_dense_points_plan_info reports
enum : uint32_t { DP_INFO_REGIME = 0, DP_INFO_SEGS = 1, DP_INFO_LANES = 2, DP_INFO_LAUNCHES = 3, DP_INFO_SCRATCH_LO = 4, DP_INFO_SCRATCH_HI = 5,
                  DP_INFO_CHUNK_LEN = 6, DP_INFO_JOBS_PER_CHUNK = 7, DP_INFO_WORDS = 8 };

}  // namespace zk
