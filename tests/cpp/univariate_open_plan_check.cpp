// The chunk planner of zkhip_univariate_kzg_open_batch (csrc/univariate_open_plan.hpp) without a GPU and without HIP: built by
// tests/test_univariate_open_plan_cpu.py with the host compiler under -fsanitize=address,undefined.  For every list of lengths: the
// status is the single call's; the chunks cover every job (a polynomial of at least one coefficient) exactly once and in order; a
// chunk holds at most UOP_CHUNK_JOBS jobs and at most UOP_SCRATCH_MAX bytes unless it is one job; quotients and rows lie inside the
// chunk's scratch, 256-byte aligned and without overlap.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../zk-cryptography_amd/csrc/univariate_open_plan.hpp"

using namespace zk;

static int checked = 0;
#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static UopPlan run(const char* what, size_t n_points, const std::vector<size_t>& len, int want_status) {
    const UopPlan p = uop_plan(n_points, len.data(), (uint32_t)len.size());
    REQUIRE(p.status == want_status);
    REQUIRE(uop_check(n_points, len.data(), (uint32_t)len.size()) == want_status);
    if (want_status != ZKHIP_OK) { REQUIRE(p.chunks.empty() && p.jobs.empty()); ++checked; return p; }
    // the jobs: every polynomial of >= 1 coefficient, in the order of the batch
    size_t at = 0;
    for (uint32_t b = 0; b < len.size(); ++b) {
        if (len[b] == 0) continue;
        REQUIRE(at < p.jobs.size() && p.jobs[at].index == b && p.jobs[at].n == len[b]);
        REQUIRE(p.jobs[at].n_blocks == (len[b] + UOP_BLOCK - 1) / UOP_BLOCK);
        ++at;
    }
    REQUIRE(at == p.jobs.size());
    // the chunks: consecutive, covering, within the bounds
    uint32_t next = 0;
    size_t scratch_max = 0;
    for (const UopChunk& ch : p.chunks) {
        REQUIRE(ch.first == next && ch.count >= 1 && ch.count <= UOP_CHUNK_JOBS);
        REQUIRE(ch.n_short + ch.n_long == ch.count);
        REQUIRE(ch.count == 1 || ch.scratch_bytes <= UOP_SCRATCH_MAX);
        uint32_t n_short = 0, n_long = 0, max_blocks = 0, n_commits = 0;
        std::vector<std::pair<size_t, size_t>> spans;                    // [begin, end) in bytes
        for (uint32_t k = 0; k < ch.count; ++k) {
            const UopJob& j = p.jobs[ch.first + k];
            if (uop_short(j.n)) ++n_short;
            else { ++n_long; if (j.n_blocks > max_blocks) max_blocks = j.n_blocks; }
            if (j.n >= 2) ++n_commits;
            REQUIRE((32 * j.q_off) % 256 == 0);
            if (j.n > 1) spans.push_back({32 * j.q_off, 32 * j.q_off + 32 * (j.n - 1)});
            if (!uop_short(j.n)) {
                REQUIRE((32 * j.row_off) % 256 == 0);
                spans.push_back({32 * j.row_off, 32 * j.row_off + 64 * (size_t)j.n_blocks});
            }
        }
        REQUIRE(n_short == ch.n_short && n_long == ch.n_long && max_blocks == ch.max_blocks && n_commits == ch.n_commits);
        size_t end = 0;
        for (const auto& s : spans) {                                   // laid out in order: no span begins before the one in front ends
            REQUIRE(s.first >= end && s.second <= ch.scratch_bytes);
            end = s.second;
        }
        if (ch.scratch_bytes > scratch_max) scratch_max = ch.scratch_bytes;
        next += ch.count;
    }
    REQUIRE(next == p.jobs.size());
    REQUIRE(scratch_max == p.scratch_max);
    std::printf("%-34s jobs %6zu chunks %3zu scratch_max %zu\n", what, p.jobs.size(), p.chunks.size(), p.scratch_max);
    ++checked;
    return p;
}

int main() {
    const size_t big = (size_t)1 << 32;
    UopPlan p = run("empty", 16, {}, ZKHIP_OK);
    REQUIRE(p.chunks.empty());
    p = run("all zeros", 16, {0, 0, 0}, ZKHIP_OK);
    REQUIRE(p.chunks.empty() && p.jobs.empty());
    p = run("{1}", 0, {1}, ZKHIP_OK);                                    // a quotient of no coefficient needs no point
    REQUIRE(p.chunks.size() == 1 && p.chunks[0].n_commits == 0 && p.chunks[0].n_short == 1 && p.scratch_max == 0);
    p = run("{2}", 1, {2}, ZKHIP_OK);
    REQUIRE(p.chunks.size() == 1 && p.chunks[0].n_commits == 1 && p.scratch_max == 256);
    run("{2}, no point", 0, {2}, ZKHIP_ERR_INDEX);
    p = run("1025 x 3", 4096, std::vector<size_t>(1025, 3), ZKHIP_OK);
    REQUIRE(p.chunks.size() == 2 && p.chunks[0].count == UOP_CHUNK_JOBS && p.chunks[1].count == 1 && p.chunks[1].first == UOP_CHUNK_JOBS);
    p = run("1024 x 3", 4096, std::vector<size_t>(1024, 3), ZKHIP_OK);
    REQUIRE(p.chunks.size() == 1);
    p = run("zeros between", 4096, {0, 3, 0, 0, 1, 5, 0}, ZKHIP_OK);
    REQUIRE(p.jobs.size() == 3 && p.jobs[0].index == 1 && p.jobs[1].index == 4 && p.jobs[2].index == 5 && p.chunks[0].n_commits == 2);
    p = run("2047 2048 2049", 4096, {2047, 2048, 2049, 4095, 4096, 4097}, ZKHIP_OK);
    REQUIRE(p.chunks.size() == 1 && p.chunks[0].n_short == 2 && p.chunks[0].n_long == 4 && p.chunks[0].max_blocks == 3);
    REQUIRE(p.jobs[1].n_blocks == 1 && p.jobs[2].n_blocks == 2 && p.jobs[4].n_blocks == 2 && p.jobs[5].n_blocks == 3);
    // one job whose quotient alone exceeds the scratch bound: a chunk of its own, between its neighbours' chunks
    const size_t huge = UOP_SCRATCH_MAX / 32 + 2;
    p = run("one job above the bound", huge, {3, huge, 3, 3}, ZKHIP_OK);
    REQUIRE(p.chunks.size() == 3 && p.chunks[0].count == 1 && p.chunks[1].count == 1 && p.chunks[2].count == 2);
    REQUIRE(p.chunks[1].scratch_bytes > UOP_SCRATCH_MAX && p.jobs[1].q_off == 0);
    // many jobs that fill the bound together
    p = run("40 x 2^16", (size_t)1 << 16, std::vector<size_t>(40, (size_t)1 << 16), ZKHIP_OK);
    REQUIRE(p.chunks.size() == 2 && p.scratch_max <= UOP_SCRATCH_MAX);
    // the largest length served and the first refused
    p = run("2^31 - 1", big, {((size_t)1 << 31) - 1}, ZKHIP_OK);
    REQUIRE(p.chunks.size() == 1 && p.jobs[0].n_blocks == ((size_t)1 << 20));
    run("2^31", big, {(size_t)1 << 31}, ZKHIP_ERR_SHAPE);
    run("2^31 behind others", big, {3, 0, (size_t)1 << 31}, ZKHIP_ERR_SHAPE);
    run("too long for the SRS", 100, {101, 102}, ZKHIP_ERR_INDEX);
    run("as long as the SRS allows", 100, {101, 100}, ZKHIP_OK);
    run("index before shape", 100, {(size_t)1 << 31}, ZKHIP_ERR_INDEX);
    std::printf("checked %d length lists\n", checked);
    return 0;
}
