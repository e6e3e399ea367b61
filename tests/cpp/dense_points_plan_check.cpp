// dense_points_plan_check.cpp -- stand-alone program around csrc/dense_points_plan.hpp for tests/test_dense_points_plan_cpu.py (g++, no
// HIP).  For both ops, batch in {0, 1, 2, 3, 64, 65535} and n in {0, 1, 2, 63, 64, 65, 255, 256, 257, 2^11, 2^11 + 1, 2^14} -- for
// evaluation every pair (n_in, n_x) of them --: the segments tile the inner range exactly, in whole staged chunks; the chunks of jobs
// partition the batch; the scratch regions follow each other without overlap and hold what the kernels index; the grid dimensions
// stay within HIP's limits; a cut happens only where the first launch would not fill the chip; and the refusals: more than 65535
// jobs, interpolation with n_in != n_x or with 2^14 + 1 nodes.
// Prints one line per violation and "checked <cases>"; exit status 1 on a violation.
#include <cstdio>
#include <vector>

#include "../../zk-cryptography_amd/csrc/dense_points_plan.hpp"

using namespace zk;

static int bad = 0, cases = 0;
static void expect(bool ok, const char* what, size_t a, size_t b, size_t c) {
    ++cases;
    if (!ok && bad++ < 20) std::printf("%s (%zu, %zu, %zu)\n", what, a, b, c);
}

static size_t al(size_t x) { return (x + 255) / 256 * 256; }

static void check(int op, uint32_t batch, size_t n_in, size_t n_x) {
    const DpPlan p = dp_plan(op, batch, n_in, n_x);
    if (op == DP_OP_INTERPOLATE && n_in != n_x) {
        expect(p.regime == DP_REFUSED, "interpolation needs as many values as nodes", batch, n_in, n_x);
        return;
    }
    if (batch == 0 || n_x == 0) {
        expect(p.regime == DP_NOOP && p.launches == 0 && p.scratch_bytes == 0 && p.n_chunks == 0, "nothing to do plans nothing", batch, n_in, n_x);
        return;
    }
    expect(p.regime == (op == DP_OP_EVALUATE ? DP_EVALUATE : DP_INTERPOLATE), "regime", batch, n_in, n_x);
    expect(p.lanes == DP_LANES && p.lanes % 64 == 0 && p.lanes <= 1024, "lanes of a workgroup", batch, n_in, p.lanes);
    // the segments tile the inner range exactly, each but the last a whole number of staged chunks
    size_t next = 0;
    bool tiles = p.segs >= 1 && p.segs <= DP_MAX_SEGS && p.seg_len % DP_CHUNK == 0 && p.n_inner == n_in;
    for (uint32_t s = 0; s < p.segs; ++s) {
        const DpSeg g = dp_seg(p, s);
        tiles = tiles && g.first == next && (g.count > 0 || n_in == 0) && g.count <= p.seg_len && (s + 1 == p.segs || g.count == p.seg_len);
        next = g.first + g.count;
    }
    expect(tiles && next == n_in, "the segments tile the inner range", batch, n_in, n_x);
    expect(dp_seg(p, p.segs).count == 0, "nothing lies beyond the last segment", batch, n_in, n_x);
    // the chunks of jobs partition the batch
    uint32_t job = 0;
    bool parts = p.chunk >= 1 && p.n_chunks == (batch + p.chunk - 1) / p.chunk;
    for (uint32_t i = 0; i < p.n_chunks; ++i) {
        const DpChunk c = dp_chunk(p, i);
        parts = parts && c.first == job && c.count >= 1 && c.count <= p.chunk && (i + 1 == p.n_chunks || c.count == p.chunk);
        job = c.first + c.count;
    }
    expect(parts && job == batch, "the chunks partition the batch", batch, n_in, n_x);
    // grids: (point blocks, segments, jobs of a chunk)
    const size_t blocks = (p.n_points + DP_LANES - 1) / DP_LANES;
    expect(p.grid_x >= 1 && p.grid_x <= DP_MAX_GRID_X && (p.grid_x == blocks || (blocks > DP_MAX_GRID_X && p.grid_x == DP_MAX_GRID_X)), "point blocks", batch, n_x, p.grid_x);
    expect((uint64_t)p.grid_x * DP_LANES < ((uint64_t)1 << 32) && p.segs <= 65535 && p.chunk <= 65535, "grid dimensions within HIP's limits", p.grid_x, p.segs, p.chunk);
    // a cut only where the first launch would not fill the chip, and then not far beyond it
    const size_t uncut = blocks * p.chunk;
    expect(p.segs == 1 || uncut < DP_TARGET_WGS, "no cut where the points fill the chip", batch, n_in, n_x);
    expect(p.segs == 1 || uncut * (p.segs - 1) < DP_TARGET_WGS, "no more segments than the target asks for", batch, n_in, n_x);
    expect(p.segs <= (n_in + DP_CHUNK - 1) / DP_CHUNK || p.segs == 1, "a segment is at least one staged chunk", batch, n_in, n_x);
    // the scratch: regions in order, each as large as what the kernels index, none overlapping
    expect(p.o_flag == 0 && p.o_winv >= 4 && p.o_winv <= p.o_rec1 && p.o_rec1 <= p.o_rec2 && p.o_rec2 <= p.o_vals && p.o_vals <= p.o_work && p.o_work <= p.scratch_bytes,
           "the regions follow each other", batch, n_in, n_x);
    expect(p.o_winv % 32 == 0 && p.o_rec1 % 32 == 0 && p.o_rec2 % 32 == 0 && p.o_vals % 32 == 0 && p.o_work % 32 == 0, "field elements are aligned", batch, n_in, n_x);
    if (op == DP_OP_EVALUATE) {
        expect(p.n_chunks == 1 && p.chunk == batch && p.n_points == n_x && p.log_N == 0, "evaluation runs the batch as one chain", batch, n_in, n_x);
        expect(p.launches == (p.segs > 1 ? 2u : 1u), "launches", batch, n_in, p.launches);
        const size_t rec = p.segs > 1 ? (size_t)batch * p.segs * n_x * 32 : 0;
        expect(p.scratch_bytes - p.o_rec2 >= rec && p.scratch_bytes == p.o_rec2 + al(rec), "the records' region", batch, n_in, n_x);
        return;
    }
    const size_t n = n_x, N = (size_t)1 << p.log_N;
    expect(N >= n && (N == 1 || N / 2 < n) && p.n_points == N, "the transform domain is the power of two at or above n", batch, n, N);
    const bool work = p.log_N >= 12;
    expect(p.o_rec1 - p.o_winv >= (size_t)p.chunk * n * 32, "room for 1 / D_i of every job of a chunk", batch, n, p.chunk);
    expect(p.o_rec2 - p.o_rec1 >= (p.segs > 1 ? (size_t)p.chunk * p.segs * n * 32 : 0), "room for the partial products", batch, n, p.segs);
    expect(p.o_vals - p.o_rec2 >= (p.segs > 1 ? (size_t)p.chunk * p.segs * N * 64 : 0), "room for the (Num, Den) records", batch, n, p.segs);
    expect(p.o_work - p.o_vals >= (size_t)p.chunk * N * 32, "room for the domain values", batch, n, N);
    expect(p.scratch_bytes - p.o_work >= (work ? (size_t)p.chunk * N * 32 : 0), "room for the transform's work rows", batch, n, N);
    expect((size_t)p.chunk * 32 * (n + N + (work ? N : 0)) <= DP_SCRATCH_BYTES || p.chunk == 1, "a chunk's rows stay under the bound", batch, n, p.chunk);
    expect(p.scratch_bytes <= DP_SCRATCH_BYTES + ((size_t)32 << 20), "and its records add little", batch, n, p.scratch_bytes);
    const uint32_t ntt = work ? 2u : 1u;                                  // 2^12 .. 2^14: the first eight stages and one pass
    expect(p.launches == (p.segs > 1 ? 4u : 2u) + ntt, "launches", batch, n, p.launches);
}

int main() {
    const std::vector<uint32_t> batches = {0, 1, 2, 3, 64, 65535};
    const std::vector<size_t> sizes = {0, 1, 2, 63, 64, 65, 255, 256, 257, (size_t)1 << 11, ((size_t)1 << 11) + 1, (size_t)1 << 14};
    for (uint32_t batch : batches)
        for (size_t n_in : sizes)
            for (size_t n_x : sizes) {
                check(DP_OP_EVALUATE, batch, n_in, n_x);
                check(DP_OP_INTERPOLATE, batch, n_in, n_x);
            }
    // many points: the grid is capped and the workgroups stride
    check(DP_OP_EVALUATE, 1, 5, ((size_t)1 << 30) + 7);
    // few points against many coefficients are cut, many points are not
    expect(dp_plan(DP_OP_EVALUATE, 1, (size_t)1 << 14, 3).segs == DP_MAX_SEGS, "one point block against 2^14 coefficients", 1, 1 << 14, 3);
    expect(dp_plan(DP_OP_EVALUATE, 64, (size_t)1 << 14, 4096).segs == 1, "64 x 16 point blocks need no cut", 64, 1 << 14, 4096);
    expect(dp_plan(DP_OP_INTERPOLATE, 1, (size_t)1 << 14, (size_t)1 << 14).segs == 8, "64 point blocks of one job: eight segments", 1, 1 << 14, 0);
    // the refusals
    for (int op = 0; op < 2; ++op) {
        expect(dp_plan(op, 65536, 4, 4).regime == DP_REFUSED, "more than 65535 jobs", op, 65536, 4);
        expect(dp_plan(op, 1, DP_MAX_N + 1, DP_MAX_N + 1).regime == DP_REFUSED, "sizes no device holds", op, 0, 0);
    }
    expect(dp_plan(DP_OP_INTERPOLATE, 1, DP_INTERP_MAX + 1, DP_INTERP_MAX + 1).regime == DP_REFUSED, "2^14 + 1 nodes", 1, DP_INTERP_MAX + 1, 0);
    expect(dp_plan(DP_OP_INTERPOLATE, 1, DP_INTERP_MAX, DP_INTERP_MAX).regime == DP_INTERPOLATE, "2^14 nodes", 1, DP_INTERP_MAX, 0);
    expect(dp_plan(DP_OP_EVALUATE, 1, DP_INTERP_MAX + 1, DP_INTERP_MAX + 1).regime == DP_EVALUATE, "evaluation has no such bound", 1, DP_INTERP_MAX + 1, 0);
    expect(dp_plan(2, 1, 4, 4).regime == DP_REFUSED && dp_plan(-1, 1, 4, 4).regime == DP_REFUSED, "no such op", 2, 0, 0);
    std::printf("checked %d\n", cases);
    return bad ? 1 : 0;
}
