// commit_polys_plan.hpp -- what zkhip_kzg_commit_polys (msm.hip) decides on the host before it launches anything: which route serves a
// batch of polynomials against ONE SRS, how the batch is cut into chunks, and what a chunk occupies in the context's workspace.
// Functions of (n_points, the polynomials' lengths, table or plain points) alone; the entry point, its diagnostic
// (zkhip_commit_polys_plan_info) and tests/cpp/commit_polys_plan_check.cpp share this one definition.  No HIP in here.
//
//   SINGLE   one polynomial, or a shape no batched route serves faster than the caller's own single commits (below): the call runs
//            them itself -- the single call's path for one polynomial, three commits in flight (zkhip_kzg_commit_begin / _end) for more.
//   SHORT    a table is given, no polynomial is longer than CPP_SMALL_MAX and the batch holds at most CPP_SHORT_TOTAL_MAX scalars: the
//            plane sums of the short commits with the polynomial as a grid dimension, in chunks of at most CPP_SMALL_CHUNK polynomials
//            (one copy, one synchronisation per chunk).
//   BUCKET   everything else: chunks of consecutive polynomials, each ONE pass of the bucket pipeline in the geometry mode "several
//            problems, one set of points" (msm_geometry.hpp).
//
// The thresholds, measured (tools/perf_commit_batch.py on one MI355X, ms per polynomial, profiles/commit_batch/NOTES.md; (a) a loop of
// single commits, (b) the same three in flight, (c) this call):
//   plain points, bucket route   2^13: B = 2 / 8 / 64: (c) 0.50 / 0.149 / 0.062 against (b) 0.76 / 0.55 / 0.50;  2^16: 0.59 / 0.35 / 0.29
//                                against 0.77 / 0.59 / 0.53;  2^18: 1.27 / 1.02 / 0.98 against 1.24 / 1.09 / 1.01 -- within a few per
//                                cent, the pass is throughput bound either way: CPP_PLAIN_MAX = 2^16.
//   table, bucket route          2^14: B = 3 / 8 / 64: 0.294 / 0.127 / 0.077 against (b) 0.321 / 0.320 / 0.282;  2^16 (four problems per
//                                pass: 2^18 buckets each): 0.48 / 0.42 / 0.40 against 0.47 / 0.44 / 0.40 -- no gain; 2^18: 7 % behind (b):
//                                CPP_TABLE_MAX = 2^14.  Two polynomials tie with (b) at every size (2^13: 0.402 / 0.401): from three on.
//   table, short or bucket       the plane sums redo the digits of every pair once per plane: 0.2 ms + ~54 ns per scalar, against ~0.9 ms
//                                + ~0.03 ms per polynomial for a pass of the bucket pipeline.  2^8: B = 8 short 0.047 / bucket 0.097,
//                                B = 64 0.0203 / 0.0138;  2^12: B = 2 0.346 / 0.468, B = 3 0.299 / 0.315, B = 8 0.252 / 0.124,
//                                B = 64 0.227 / 0.0315: CPP_SHORT_TOTAL_MAX = 2^13 scalars in the batch.
//
// A BUCKET chunk is the longest run of polynomials for which all of this holds:
//   - at most MSM_MAX_PROBLEMS problems, at most MSM_MAX_WINS digit windows and SORT_MAX_PARTS sort partitions -- counted at the widths
//     log2(n_j) - CPP_DELTA with plain points (msm_build_geometry starts one bit below the size and narrows the windows until the
//     partitions fit: it ends at CPP_DELTA at the latest, and never narrower than this rule allows, so the lists a lane of the
//     accumulate pass walks stay at 2^CPP_DELTA .. 2^(CPP_DELTA + 1) points) and at the table's own widths with the table, where a
//     problem owns one set of 2^(hi - 1) buckets (2^16 points: hi = 19, 1024 partitions, four problems per pass);
//   - fewer than 2^31 scalars and (point, window) pairs;
//   - its workspace (cpp_ws_bytes: the carve-up of msm_enqueue) is at most CPP_WS_MAX = 512 MiB, whatever `batch` is -- about what ONE
//     commit of 2^20 scalars occupies (509 MB), which a context that commits at that size holds anyway.  A chunk of one polynomial takes
//     what the single commit takes.  The call keeps two chunks in flight (the host epilogues of one beside the passes of the next).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "msm_geometry.hpp"

namespace zk {

constexpr size_t CPP_SMALL_MAX = 4096;              // MSM_SMALL_MAX of msm.hip
constexpr uint32_t CPP_SMALL_CHUNK = 64;            // polynomials per chunk of the short route (OPEN_BATCH_CHUNK's reasoning: >= 64 x ~15 planes of waves fill the chip)
constexpr size_t CPP_WS_MAX = (size_t)512 << 20;
constexpr int CPP_DELTA = 3;
constexpr size_t CPP_SHORT_TOTAL_MAX = (size_t)1 << 13;      // scalars of a batch the short route serves
constexpr size_t CPP_PLAIN_MAX = (size_t)1 << 16;            // the longest polynomial of a batch the bucket route serves with plain points ...
constexpr size_t CPP_TABLE_MAX = (size_t)1 << 14;            // ... and with the table,
constexpr uint32_t CPP_TABLE_MIN_BATCH = 3;                  //     from this many polynomials on
// sizes of msm_kernels.hpp that the workspace carve-up depends on (msm.hip asserts that they are the kernels')
constexpr size_t CPP_SORT_TILE = 2048, CPP_COUNT_BINS = 1024, CPP_HEAVY_REC = 2048, CPP_HEAVY_LEVELS = 4, CPP_HEAVY_REC_BYTES = 16,
                 CPP_OVERFLOW_BYTES = 20;

enum CppRoute : uint32_t { CPP_SINGLE = 0, CPP_SHORT = 1, CPP_BUCKET = 2 };

// the bytes msm_enqueue carves out of the workspace for a pass of geometry g over n_total scalars; n_conv: the points it converts into
// the internal layout (the longest polynomial of the chunk; 0 with the table)
inline size_t cpp_ws_bytes(const MsmGeometry& g, size_t n_total, size_t n_conv) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t n_buckets = g.pl.n_buckets, n_segments = n_buckets / MSM_SEG, n_wgs = (n_total + CPP_SORT_TILE - 1) / CPP_SORT_TILE;
    const size_t rec_cap = g.items / g.heavy_min + g.items / CPP_HEAVY_REC + 2, slots_cap = 3 * (g.items / CPP_HEAVY_REC) + 8;
    size_t t = 3 * al(n_buckets * 4) + al(CPP_COUNT_BINS * 4) + al(CPP_OVERFLOW_BYTES);                  // counts, offsets, order | bins | heavy counters
    t += al(g.items * 4) + al(g.items * 8) + al(n_wgs * g.pl.n_parts * 4) + 2 * al(((size_t)g.pl.n_parts + 1) * 4);   // sorted, items, workgroup counts, partition counts / offsets
    t += al(n_conv * 128) + al(n_buckets * 256) + 2 * al(n_segments * 256) + al((size_t)g.pl.n_terms * 192);      // points, buckets, segment sums, terms
    t += al((size_t)g.pl.n_rc * 256) + al(CPP_HEAVY_LEVELS * rec_cap * CPP_HEAVY_REC_BYTES) + al(slots_cap * 256);     // rows / columns, heavy records and partial sums
    return t;
}

// digit windows and sort partitions of ONE problem of nj scalars in a pass of several (msm_build_geometry_at at `delta`)
struct CppCost { uint32_t wins, parts; };
inline CppCost cpp_problem_cost(size_t nj, size_t n_points, bool table, int delta) {
    CppCost k = {};
    if (table) {
        const MsmLevelWidths lw = msm_table_widths(n_points);
        k.wins = lw.W;
        k.parts = lw.hi - 1 > 8 ? 1u << (lw.hi - 1 - 8) : 1u;
        return k;
    }
    int lg = 0;
    while (((size_t)1 << lg) < nj) ++lg;
    const uint32_t c = (uint32_t)std::min(16, std::max(8, lg - delta));
    const uint32_t w = (256 + c - 1) / c, hi = (256 + w - 1) / w, n_hi = 256 - w * (hi - 1);
    k.wins = w;
    for (uint32_t v = 0; v < w; ++v) {
        const uint32_t cv = v < n_hi ? hi : hi - 1;
        k.parts += cv - 1 > 8 ? 1u << (cv - 1 - 8) : 1u;
    }
    return k;
}

struct CppChunk {
    uint32_t first, count;                          // polynomials [first, first + count) of the (non-empty) polynomials handed to cpp_plan
    MsmProblems pr;                                 // BUCKET: the chunk's problems (off: running sum of the lengths) ...
    std::shared_ptr<const MsmGeometry> geo;         // ... and its geometry, mode "one set of points"
    size_t n_total, n_conv, ws_bytes;               // BUCKET: scalars of the pass, points converted, workspace
};
struct CppPlan {
    CppRoute route = CPP_SINGLE;
    int status = ZKHIP_OK;                          // ZKHIP_ERR_SHAPE: a polynomial no geometry serves (>= 2^31 scalars or table entries)
    std::vector<CppChunk> chunks;
};

// len[0 .. batch): the polynomials' lengths, all in [1, n_points].  small_on: the short path is not switched off (ZKHIP_MSM_SMALL).
inline CppPlan cpp_plan(size_t n_points, const size_t* len, uint32_t batch, bool table, bool small_on = true) {
    CppPlan p;
    if (batch == 0) return p;
    size_t longest = 0;
    for (uint32_t b = 0; b < batch; ++b) longest = std::max(longest, len[b]);
    if (longest >= ((size_t)1 << 31) || (table && n_points * msm_table_widths(n_points).W >= ((size_t)1 << 31))) { p.status = ZKHIP_ERR_SHAPE; return p; }
    size_t total = 0;
    for (uint32_t b = 0; b < batch; ++b) total += len[b];
    auto singles = [&]() {
        p.route = CPP_SINGLE;
        p.chunks.clear();
        for (uint32_t b = 0; b < batch; ++b) p.chunks.push_back(CppChunk{b, 1, {}, nullptr, len[b], table ? 0 : len[b], 0});
    };
    if (batch == 1) { singles(); return p; }
    if (table && small_on && longest <= CPP_SMALL_MAX && total <= CPP_SHORT_TOTAL_MAX) {
        p.route = CPP_SHORT;
        for (uint32_t b = 0; b < batch; b += CPP_SMALL_CHUNK) p.chunks.push_back(CppChunk{b, std::min(CPP_SMALL_CHUNK, batch - b), {}, nullptr, 0, 0, 0});
        return p;
    }
    if (longest > (table ? CPP_TABLE_MAX : CPP_PLAIN_MAX) || (table && batch < CPP_TABLE_MIN_BATCH)) { singles(); return p; }
    p.route = CPP_BUCKET;
    bool any_multi = false;
    for (uint32_t first = 0; first < batch;) {
        // the longest run the counted limits allow ...
        uint32_t count = 0, wins = 0, parts = 0;
        size_t total = 0, items = 0;
        while (first + count < batch && count < (uint32_t)MSM_MAX_PROBLEMS) {
            const size_t nj = len[first + count];
            const CppCost k = cpp_problem_cost(nj, n_points, table, CPP_DELTA);
            if (count && (wins + k.wins > (uint32_t)MSM_MAX_WINS || parts + k.parts > (uint32_t)SORT_MAX_PARTS ||
                          total + nj >= ((size_t)1 << 31) || items + nj * 32 >= ((size_t)1 << 31)))      // (<= 32 windows per problem)
                break;
            wins += k.wins; parts += k.parts; total += nj; items += nj * 32;
            ++count;
        }
        // ... shortened until its geometry builds and its workspace is within the bound (a chunk of one is a single commit's pass)
        CppChunk ch = {};
        for (;;) {
            ch = CppChunk{};
            ch.first = first; ch.count = count;
            ch.pr.n = count;
            for (uint32_t j = 0; j < count; ++j) {
                ch.pr.off[j + 1] = ch.pr.off[j] + (uint32_t)len[first + j];
                ch.n_conv = std::max(ch.n_conv, len[first + j]);
            }
            ch.n_total = ch.pr.off[count];
            if (table) ch.n_conv = 0;
            // the same shape as the chunk before (a uniform batch): the same geometry
            const CppChunk* prev = p.chunks.empty() ? nullptr : &p.chunks.back();
            if (prev && prev->count == count && std::equal(prev->pr.off, prev->pr.off + count + 1, ch.pr.off)) {
                ch.geo = prev->geo;
            } else {
                auto g = std::make_shared<MsmGeometry>();
                const int rc = msm_build_geometry(ch.pr, table, table ? n_points : 0, *g, true);
                if (rc != ZKHIP_OK) {
                    if (count == 1) { p.status = rc; p.chunks.clear(); return p; }
                    --count;
                    continue;
                }
                ch.geo = g;
            }
            ch.ws_bytes = cpp_ws_bytes(*ch.geo, ch.n_total, ch.n_conv);
            if (count == 1 || ch.ws_bytes <= CPP_WS_MAX) break;
            const uint32_t fit = (uint32_t)((double)count * (double)CPP_WS_MAX / (double)ch.ws_bytes);
            count = std::max<uint32_t>(1, std::min(count - 1, fit));
        }
        std::memcpy(ch.pr.win_first, ch.geo->win_first, sizeof(ch.pr.win_first));
        any_multi = any_multi || count > 1;
        p.chunks.push_back(ch);
        first += count;
    }
    // no chunk holds two polynomials: the batch has nothing to share, and the call is the loop of single commits
    if (!any_multi) singles();
    return p;
}

}  // namespace zk
