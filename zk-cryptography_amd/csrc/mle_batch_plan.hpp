// mle_batch_plan.hpp -- what zkhip_mle_evaluation_batch (zkhip.hip) decides on the host before it enqueues anything: which of its three
// regimes serves a batch, how the batch is cut into chunks, how many workgroups and records a job takes, the dynamic LDS of a workgroup
// and the layout of a chunk in the context's workspace.  Functions of (log2 n, batch) alone: the entry point, the kernels' index of a
// block's weight (mle_batch_kernels.hpp) and tests/test_mle_batch_plan_cpu.py share this one definition.  No HIP in here.
//
//   RESIDENT  n <= 2^12: one workgroup per job stages the table in LDS and folds it to its value (fold_tail_kernel's body).
//   BLOCKS    2^13 <= n <= 2^16, h = log2(n) - 12: workgroup (q, b) of a grid (2^h, jobs) folds entries [q 2^12, (q + 1) 2^12) of
//             table b with points h .. n_pts - 1, weights the value with eq_q(points 0 .. h - 1) and stores one record; a second
//             launch sums each job's 2^h records.  Point 0 is the MOST significant index bit (`evaluation` folds variable 0 first),
//             so the bit of q that point i selects is bit h - 1 - i: meb_weight_bit.
//   SINGLE    n >= 2^17, one job, or fewer jobs than meb_min_batch: zkhip_mle_evaluation's own path, job after job.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zk {

constexpr uint32_t MEB_TAIL_LOG = 12;        // the largest table one workgroup folds in LDS (TAIL_LOG of mle_kernels.hpp: 128 KiB of the CU's 160)
constexpr uint32_t MEB_MAX_LOG = 16;         // the largest table the kernels take: 2^4 blocks
constexpr uint32_t MEB_CHUNK = 1024;         // jobs per launch (Multilinear.BATCH_CHUNK of the Python mirror)
constexpr uint32_t MEB_BLOCK = 256;          // lanes of a workgroup (MLE_BLOCK) ...
constexpr uint32_t MEB_WIDE_BLOCK = 1024;    // ... and of one that stages 2^MEB_WIDE_LOG entries or more
// Measured with 2^12 staged entries only -- tables of 2^12 entries and every block of a larger one --, where 1024 lanes took 7-10 % less
// than 256 (profiles/mle_batch/NOTES.md, "Lanes").  Smaller tables were not compared and keep 256.
constexpr uint32_t MEB_WIDE_LOG = 12;
static_assert(MEB_WIDE_LOG <= MEB_TAIL_LOG, "a block of a larger table is staged whole: the blocks kernel has MEB_WIDE_BLOCK lanes");
constexpr size_t MEB_MAX_LDS_BYTES = 160 * 1024;

enum MebRegime : uint32_t { MEB_SINGLE = 0, MEB_RESIDENT = 1, MEB_BLOCKS = 2 };

// The fewest jobs the kernels take at this size; 0: no batch is taken (n >= 2^17).  Measured against the loop of single calls per size
// class (profiles/mle_batch/NOTES.md, "The threshold"): two jobs already gain at every size the kernels serve.
constexpr uint32_t meb_min_batch(uint32_t log_n) { return log_n > MEB_MAX_LOG ? 0u : 2u; }

constexpr MebRegime meb_regime(uint32_t log_n, uint32_t batch) {
    return (log_n > MEB_MAX_LOG || batch <= 1 || batch < meb_min_batch(log_n)) ? MEB_SINGLE : log_n <= MEB_TAIL_LOG ? MEB_RESIDENT : MEB_BLOCKS;
}

// which way point i (< h) of a job weights block q (< 2^h): 1 -> the factor r_i, 0 -> 1 - r_i
constexpr uint32_t meb_weight_bit(uint32_t q, uint32_t h, uint32_t i) { return (q >> (h - 1 - i)) & 1u; }

constexpr uint32_t meb_lanes(uint32_t staged_log) { return staged_log >= MEB_WIDE_LOG ? MEB_WIDE_BLOCK : MEB_BLOCK; }

constexpr size_t meb_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct MebPlan {
    MebRegime regime;
    uint32_t log_n, h;               // h: log2 of the blocks per job (0 when resident)
    uint32_t chunk;                  // jobs of a full chunk: min(batch, MEB_CHUNK)
    uint32_t n_chunks;
    uint32_t wgs_per_job;            // workgroups of the first launch per job: 2^h
    uint32_t records_per_job;        // records the second launch sums per job: 2^h with blocks, none when resident
    uint32_t launches;               // per chunk
    uint32_t lanes;                  // of a workgroup of the first launch
    size_t lds_bytes;                // dynamic LDS of a workgroup: 32 bytes per staged entry
    // the chunk in the workspace: [table pointers | points] (one upload) [results] [records]; the pinned stage holds [results] [pointers | points]
    size_t o_points, upload_bytes, o_results, o_records, ws_bytes, pin_bytes;
};

// The plan of `batch` jobs on tables of 2^log_n entries.  MEB_SINGLE (and batch == 0) plans nothing: no chunk, no launch, no byte.
constexpr MebPlan meb_plan(uint32_t log_n, uint32_t batch) {
    MebPlan p = {};
    p.regime = batch ? meb_regime(log_n, batch) : MEB_SINGLE;
    p.log_n = log_n;
    if (p.regime == MEB_SINGLE) return p;
    p.h = p.regime == MEB_BLOCKS ? log_n - MEB_TAIL_LOG : 0u;
    p.chunk = batch < MEB_CHUNK ? batch : MEB_CHUNK;
    p.n_chunks = (batch + p.chunk - 1) / p.chunk;
    p.wgs_per_job = 1u << p.h;
    p.records_per_job = p.regime == MEB_BLOCKS ? 1u << p.h : 0u;
    p.launches = p.regime == MEB_BLOCKS ? 2u : 1u;
    p.lds_bytes = (size_t)32 << (log_n - p.h);
    p.lanes = meb_lanes(log_n - p.h);
    p.o_points = meb_align((size_t)p.chunk * 8);
    p.upload_bytes = p.o_points + meb_align((size_t)p.chunk * log_n * 32);
    p.o_results = p.upload_bytes;
    p.o_records = p.o_results + meb_align((size_t)p.chunk * 32);
    p.ws_bytes = p.o_records + meb_align((size_t)p.chunk * p.records_per_job * 32);
    p.pin_bytes = meb_align((size_t)p.chunk * 32) + p.upload_bytes;
    return p;
}

// chunk i of the batch: jobs [first, first + count)
struct MebChunk { uint32_t first, count; };
constexpr MebChunk meb_chunk(const MebPlan& p, uint32_t batch, uint32_t i) {
    const uint32_t first = i * p.chunk;
    return {first, batch - first < p.chunk ? batch - first : p.chunk};
}

}  // namespace zk
