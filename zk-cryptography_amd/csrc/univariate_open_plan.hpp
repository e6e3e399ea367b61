// univariate_open_plan.hpp -- what zkhip_univariate_kzg_open_batch (msm.hip) decides on the host before it launches anything: the checks on
// the lengths, how the batch is cut into chunks, and where a job's quotient and its row of workgroup values and carries lie in the chunk's
// scratch.  Functions of (n_points, the polynomials' lengths) alone; the entry point and tests/cpp/univariate_open_plan_check.cpp share
// this one definition.  No HIP in here.
//
// A JOB is one opening that needs the device: a polynomial of at least one coefficient.  (Length 0 is answered on the host.  Length 1 has
// no quotient, but its evaluation c0 is delivered by the scan as the single call delivers it: it is a job of one workgroup and commits
// nothing.)  A job of at most UOP_BLOCK coefficients is SHORT -- one workgroup scans it in one launch --, every other is LONG: three
// launches (scan, top, apply; horner_jobs_kernels.hpp) with a row of one value and one carry per workgroup.
//
// A CHUNK is the longest run of consecutive jobs for which all of this holds:
//   - at most UOP_CHUNK_JOBS = 1024 jobs (a job is grid.y of the scans; the table of one chunk is 64 KiB);
//   - its scratch -- the quotients, 32-byte elements and 256-byte aligned per job, then the long jobs' rows -- is at most
//     UOP_SCRATCH_MAX = 64 MiB, whatever `batch` is: device scratch does not grow with the batch.  A job whose own quotient is larger is
//     a chunk of its own and takes what the single call takes for it (32 n bytes).
// The chunk's non-empty quotients go to the routes of zkhip_kzg_commit_polys, which cuts them again by its own rules (commit_polys_plan.hpp).
//
// ONE ROUTE.  A shape that measured no faster here than a loop of zkhip_univariate_kzg_open would run as that loop inside the call; none
// did (tools/perf_univariate_open_batch.py on one MI355X, ms per opening, profiles/univariate_open_batch/NOTES.md; loop / batch):
//   plain points   2^8: B = 2 / 8 / 64: 0.79 / 0.42, 0.80 / 0.126, 0.78 / 0.027;   2^12: 1.17 / 0.58, 1.17 / 0.160, 1.17 / 0.050;
//                  2^14: 1.09 / 0.61, 1.07 / 0.212, 1.08 / 0.106;                  2^16: 1.09 / 0.70, 1.10 / 0.37, 1.09 / 0.33
//   table          2^8: 0.78 / 0.174, 0.78 / 0.054, 0.81 / 0.015;                  2^12: 1.16 / 0.45, 1.16 / 0.140, 1.16 / 0.034;
//                  2^14: 1.10 / 0.51, 1.08 / 0.144, 1.07 / 0.078;                  2^16: 1.09 / 0.58, 1.09 / 0.46, 1.09 / 0.43
// The smallest gain is 1.55 x (2^16, B = 2, plain points), ten quartile ranges of the legs apart.  Beyond 2^16 coefficients the commits
// are commit_polys_plan.hpp's single route -- the caller's own commits, three in flight -- so the batch still saves the loop's two
// synchronisations per opening.  One opening (batch == 1) is the single call's path.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/zkhip.h"

namespace zk {

constexpr size_t UOP_BLOCK = 2048;                       // HS_T * HS_L of mle_kernels.hpp (msm.hip asserts it): coefficients per workgroup
constexpr uint32_t UOP_CHUNK_JOBS = 1024;                // jobs per chunk
constexpr size_t UOP_SCRATCH_MAX = (size_t)64 << 20;     // bytes of quotients and rows per chunk (a lone larger job excepted)

struct UopJob {
    uint32_t index;                                 // the opening's place in the batch
    size_t n;                                       // coefficients, >= 1
    uint32_t n_blocks;                              // workgroups of its scan
    size_t q_off;                                   // quotient: 32-byte elements from the base of the chunk's scratch (n - 1 of them)
    size_t row_off;                                 // LONG: its n_blocks values, then its n_blocks carries, in 32-byte elements from the same base
};
struct UopChunk {
    uint32_t first, count;                          // jobs [first, first + count) of UopPlan::jobs
    uint32_t n_short, n_long, max_blocks;           // max_blocks: workgroups of the longest LONG job
    uint32_t n_commits;                             // jobs with a quotient (n >= 2)
    size_t scratch_bytes;
};
struct UopPlan {
    int status = ZKHIP_OK;
    std::vector<UopJob> jobs;                       // in the order of the batch
    std::vector<UopChunk> chunks;
    size_t scratch_max = 0;                         // the largest chunk's scratch
};

inline bool uop_short(size_t n) { return n <= UOP_BLOCK; }
inline size_t uop_al(size_t x) { return (x + 255) & ~(size_t)255; }

// the single call's checks on a length, in its order: ZKHIP_ERR_INDEX (univariate_kzg.rs:75), then ZKHIP_ERR_SHAPE
inline int uop_check(size_t n_points, const size_t* len, uint32_t batch) {
    for (uint32_t b = 0; b < batch; ++b) {
        if (len[b] == 0) continue;
        if (len[b] - 1 > n_points) return ZKHIP_ERR_INDEX;
        if (len[b] >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;
    }
    return ZKHIP_OK;
}

inline UopPlan uop_plan(size_t n_points, const size_t* len, uint32_t batch) {
    UopPlan p;
    p.status = uop_check(n_points, len, batch);
    if (p.status != ZKHIP_OK) return p;
    UopChunk ch = {};
    auto close = [&]() {
        if (!ch.count) return;
        p.scratch_max = std::max(p.scratch_max, ch.scratch_bytes);
        p.chunks.push_back(ch);
        ch = UopChunk{};
        ch.first = (uint32_t)p.jobs.size();
    };
    for (uint32_t b = 0; b < batch; ++b) {
        const size_t n = len[b];
        if (n == 0) continue;
        UopJob j = {};
        j.index = b;
        j.n = n;
        j.n_blocks = (uint32_t)((n + UOP_BLOCK - 1) / UOP_BLOCK);
        const size_t q_bytes = uop_al(32 * (n - 1)), row_bytes = uop_short(n) ? 0 : uop_al(64 * (size_t)j.n_blocks);
        if (ch.count && (ch.count == UOP_CHUNK_JOBS || ch.scratch_bytes + q_bytes + row_bytes > UOP_SCRATCH_MAX)) close();
        j.q_off = ch.scratch_bytes / 32;
        j.row_off = (ch.scratch_bytes + q_bytes) / 32;
        ch.scratch_bytes += q_bytes + row_bytes;
        ++ch.count;
        if (uop_short(n)) ++ch.n_short;
        else { ++ch.n_long; ch.max_blocks = std::max(ch.max_blocks, j.n_blocks); }
        if (n >= 2) ++ch.n_commits;
        p.jobs.push_back(j);
    }
    close();
    return p;
}

}  // namespace zk
