// msm.hip -- C-ABI entry points of the KZG commit path (MSM over G1) and SRS generation.
// gfx950 only.  No CPU fallback: every entry point launches HIP kernels or fails.
#include "../../include/zkhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "commit_polys_plan.hpp"
#include "ctx.hpp"
#include "host_util.hpp"
#include "host_g1.hpp"
#include "horner_jobs_kernels.hpp"
#include "mle_kernels.hpp"
#include "msm_kernels.hpp"
#include "msm_small_fold.hpp"
#include "srs_kernels.hpp"
#include "tunables.hpp"
#include "univariate_open_plan.hpp"

using namespace zk;

// ---------------------------------------------------------------------------------------
// KZG commit (MSM)
// ---------------------------------------------------------------------------------------
// Geometry of one pass (msm_kernels.hpp: MsmWin / MsmSet / MsmPlan): how every problem's 256 scalar bits are cut into digit windows,
// and the bucket sets behind them.
//   one problem:   uniform windows of c bits, c = 16 from 2^13 points on (one lane per bucket: the accumulate pass wants many short
//                  lists, so the window is as wide as the sort allows as soon as the bucket reduction is not the larger cost; measured
//                  with tools/perf_msm.py while the width was a run-time choice: below 2^13 every c ends at the ~1 ms latency floor of the reduction
//                  passes).  16 x 16 = 256: the top window has 15 significant bits, half full, never sparse.
//   shifted table: at 2^20 points thirteen digit windows of 20 / 19 bits on ONE bucket set of 2^19 buckets; widths by SRS size (msm_table_widths).
//   several:       every problem gets a width of its OWN, log2(n_j) - delta bits (lists of 2^delta .. 2^(delta+1) points: the accumulate pass
//                  takes as long as its longest lists, and every further bit doubles the buckets the reduction passes walk), as w = ceil(256 / c)
//                  windows of the two widths ceil(256 / w) and one less that add up to exactly 256 -- so no window of any problem is
//                  sparse (a 3-bit top window put an eighth of all points into each of 4 buckets: the heavy-bucket passes, 0.6 ms) and
//                  all problems share ONE pass of every kernel (MultilinearKZG::open at 2^20: twenty problems, ~0.45 M buckets).
// the geometries of the last few shapes (an opening builds its twenty-problem geometry twice per call otherwise: ~0.1 ms of host time each)
static int msm_geometry(const MsmProblems& pr, bool shared, size_t table_stride, std::shared_ptr<const MsmGeometry>* out, bool one_points = false) {
    struct Entry { MsmProblems pr; bool shared; size_t stride; std::shared_ptr<const MsmGeometry> geo; bool one_points; };
    static std::mutex mu;
    static std::vector<Entry> cache;
    std::lock_guard<std::mutex> lk(mu);
    for (const Entry& e : cache)
        if (e.shared == shared && e.one_points == one_points && e.stride == table_stride && e.pr.n == pr.n && std::memcmp(e.pr.off, pr.off, sizeof(uint32_t) * (pr.n + 1)) == 0) {
            *out = e.geo;
            return ZKHIP_OK;
        }
    auto g = std::make_shared<MsmGeometry>();
    ZK_TRY(msm_build_geometry(pr, shared, table_stride, *g, one_points));
    if (cache.size() >= 8) cache.erase(cache.begin());
    cache.push_back({pr, shared, table_stride, g, one_points});
    *out = g;
    return ZKHIP_OK;
}
// d_table (nullable): shifted-SRS table in the internal layout, entry w * table_stride + i = 2^(20 w) * point i; then
// d_points_xy is not read and there is exactly one problem.
// A commit in two halves, so that a caller with several commits in a row (MultilinearKZG::open) can run the host epilogue
// of one while the GPU works on the next: msm_enqueue launches everything and the copy of the (set, term) points into
// pinned slot `slot` (workspace from byte offset ws_off; *ws_used = what it occupies), msm_finish waits for that copy
// and runs the epilogue.
struct MsmPending {
    std::shared_ptr<const MsmGeometry> geo;
    MsmProblems pr;
    size_t n_out = 0;
    int slot = 0;
    ZkLoan ws_loan;     // a commit in flight (zkhip_kzg_commit_begin) holds the workspace until it has ended
};
void MsmPendingDelete::operator()(MsmPending* p) const { delete p; }
// ONE SET OF POINTS (zkhip_kzg_commit_polys): the problems of the pass are polynomials of their own -- device buffers read in place
// through `ptrs`, d_scalars is not read -- against the first points of ONE SRS (d_points_xy / d_table, d_points_inf: the points' flags);
// n_conv: the points the pass converts (the longest problem; the workspace holds n_conv x 128 bytes of them, not one copy per problem);
// geo: the geometry the planner built for the chunk (mode "one set of points"), or null to build it here
struct MsmPolys { MsmPtrTable ptrs; size_t n_conv; std::shared_ptr<const MsmGeometry> geo; };
static_assert(CPP_SORT_TILE == (size_t)SORT_TILE && CPP_COUNT_BINS == (size_t)MSM_COUNT_BINS && CPP_HEAVY_REC == (size_t)MSM_HEAVY_REC &&
              CPP_HEAVY_LEVELS == (size_t)MSM_HEAVY_LEVELS && CPP_HEAVY_REC_BYTES == sizeof(MsmHeavyRec) && CPP_OVERFLOW_BYTES == sizeof(MsmOverflow),
              "commit_polys_plan.hpp sizes a chunk's workspace with the kernels' constants");
static int msm_enqueue(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, const uint64_t* d_scalars, size_t n,
                       const MsmProblems& pr_in, const uint32_t* d_table, size_t table_stride, size_t ws_off, int slot, MsmPending* pend,
                       size_t* ws_used, const MsmPolys* polys = nullptr) {
    std::shared_ptr<const MsmGeometry> geo_p = polys ? polys->geo : nullptr;
    if (!geo_p) ZK_TRY(msm_geometry(pr_in, d_table != nullptr, table_stride, &geo_p, polys != nullptr));
    const MsmGeometry& geo = *geo_p;
    MsmProblems pr = pr_in;
    std::memcpy(pr.win_first, geo.win_first, sizeof(pr.win_first));
    MsmPlan pl = geo.pl;
    const size_t n_buckets = pl.n_buckets;
    const size_t n_segments = n_buckets / MSM_SEG;
    const size_t n_out = pl.n_terms;
    // workspace carve-up (all 256-byte aligned)
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_counts = 0;
    const size_t o_offsets = o_counts + al(n_buckets * 4);
    const size_t o_order = o_offsets + al(n_buckets * 4);
    const size_t o_bins = o_order + al(n_buckets * 4);                  // the order pass's bins and, right behind them, the heavy lists' counters:
    const size_t o_ovf = o_bins + al(MSM_COUNT_BINS * 4);               //   ONE memset clears both
    const size_t o_sorted = o_ovf + al(sizeof(MsmOverflow));
    const size_t n_wgs = (n + SORT_TILE - 1) / SORT_TILE;
    const size_t o_items = o_sorted + al(geo.items * 4);
    const size_t o_wgc = o_items + al(geo.items * 8);
    const size_t o_pcnt = o_wgc + al(n_wgs * pl.n_parts * 4);
    const size_t o_poff = o_pcnt + al((pl.n_parts + 1) * 4);
    const size_t o_points = o_poff + al((pl.n_parts + 1) * 4);          // SRS in the internal 28-bit-limb layout
    const size_t n_conv = polys ? polys->n_conv : n;                    // one set of points: the longest problem's worth, once
    const size_t o_buckets = o_points + al(d_table ? 0 : n_conv * 128);
    const size_t o_segs = o_buckets + al(n_buckets * 256);
    const size_t o_sega = o_segs + al(n_segments * 256);
    const size_t o_terms = o_sega + al(n_segments * 256);
    // heavy buckets (msm_kernels.hpp pass 4b/4c): more than heavy_min points, so at most items / heavy_min of them;
    // a bucket of k points files ceil(k / MSM_HEAVY_REC) level-0 records and, above one record, a <= 256-way tree over them
    const uint32_t heavy_min = geo.heavy_min;
    const size_t items_max = geo.items;
    const size_t rec_cap = items_max / heavy_min + items_max / MSM_HEAVY_REC + 2;
    const size_t slots_cap = 3 * (items_max / MSM_HEAVY_REC) + 8;
    const size_t o_rc = o_terms + al(n_out * 192);                       // rows / columns of the segment sums (msm_rowcol_kernel)
    const size_t o_rec = o_rc + al((size_t)pl.n_rc * 256);
    const size_t o_part = o_rec + al(MSM_HEAVY_LEVELS * rec_cap * sizeof(MsmHeavyRec));
    const size_t total = o_part + al(slots_cap * 256);
    if (ws_used) *ws_used = total;
    if (!pend) return ZKHIP_OK;                     // size query only
    // a commit in flight lives in a region of the workspace its caller reserved before it took the loan: nothing to reserve, it must fit
    if (pend->ws_loan) { if (ws_off + total > c->ws.bytes) return ZKHIP_ERR_BUSY; }
    else ZK_TRY(c->reserve_ws(ws_off + total));
    char* ws = (char*)c->ws.ptr + ws_off;
    uint32_t* counts = (uint32_t*)(ws + o_counts);
    uint32_t* offsets = (uint32_t*)(ws + o_offsets);
    uint32_t* sorted = (uint32_t*)(ws + o_sorted);
    uint32_t* order = (uint32_t*)(ws + o_order);
    uint32_t* bins = (uint32_t*)(ws + o_bins);
    const uint32_t* points_u = d_table ? d_table : (const uint32_t*)(ws + o_points);
    uint32_t* rc = (uint32_t*)(ws + o_rc);
    uint2* items = (uint2*)(ws + o_items);
    uint32_t* wg_counts = (uint32_t*)(ws + o_wgc);
    uint32_t* part_count = (uint32_t*)(ws + o_pcnt);
    uint32_t* part_off = (uint32_t*)(ws + o_poff);
    uint32_t* buckets = (uint32_t*)(ws + o_buckets);
    uint32_t* segs = (uint32_t*)(ws + o_segs);
    uint32_t* sega = (uint32_t*)(ws + o_sega);
    uint64_t* terms = (uint64_t*)(ws + o_terms);
    MsmOverflow* ovf = (MsmOverflow*)(ws + o_ovf);
    MsmHeavyRec* rec = (MsmHeavyRec*)(ws + o_rec);
    uint32_t* partials = (uint32_t*)(ws + o_part);

    {   // the geometry tables: device copy of this slot, uploaded when they differ from the last commit's
        const size_t b_wins = al(geo.wins.size() * sizeof(MsmWin)), b_sets = al(geo.sets.size() * sizeof(MsmSet));
        const size_t b_part = al(geo.part_set.size() * 2), b_rcwg = al(geo.rcwg_set.size() * 2), b_term = al(geo.termwg_set.size() * 2);
        const size_t bytes = b_wins + b_sets + b_part + b_rcwg + b_term;
        ZK_TRY(c->reserve_msm_tab(slot, bytes));
        char* dev = (char*)c->msm_tab_dev[slot].ptr;
        if (c->msm_tab_geo[slot] != geo_p) {
            char* pin = (char*)c->msm_tab_pin[slot].ptr;
            // the staging buffer may still feed the upload of the slot's previous commit only if that commit has not been waited for;
            // every caller ends (msm_finish / stream synchronize) a slot's commit before it enqueues the next one there
            std::memcpy(pin, geo.wins.data(), geo.wins.size() * sizeof(MsmWin));
            std::memcpy(pin + b_wins, geo.sets.data(), geo.sets.size() * sizeof(MsmSet));
            std::memcpy(pin + b_wins + b_sets, geo.part_set.data(), geo.part_set.size() * 2);
            std::memcpy(pin + b_wins + b_sets + b_part, geo.rcwg_set.data(), geo.rcwg_set.size() * 2);
            std::memcpy(pin + b_wins + b_sets + b_part + b_rcwg, geo.termwg_set.data(), geo.termwg_set.size() * 2);
            ZK_HIP(c, hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, c->stream));
            c->msm_tab_geo[slot] = geo_p;
        }
        pl.wins = (const MsmWin*)dev;
        pl.sets = (const MsmSet*)(dev + b_wins);
        pl.part_set = (const uint16_t*)(dev + b_wins + b_sets);
        pl.rcwg_set = (const uint16_t*)(dev + b_wins + b_sets + b_part);
        pl.termwg_set = (const uint16_t*)(dev + b_wins + b_sets + b_part + b_rcwg);
    }
    const int grid_n = (int)std::min<size_t>((n_conv + MSM_BLOCK - 1) / MSM_BLOCK, 256 * 8);
    if (!d_table) {
        ProfScope ps(c, "msm_convert_points", 224.0 * (double)n_conv);
        hipLaunchKernelGGL(msm_convert_points_kernel, dim3(grid_n), dim3(MSM_BLOCK), 0, c->stream, d_points_xy, n_conv, (uint32_t*)(ws + o_points));
    }
    {   // two-level counting sort of the (point, window) pairs by bucket; also yields counts[] and offsets[]
        ProfScope ps(c, "msm_sort", 32.0 * (double)n);
        if (polys) hipLaunchKernelGGL(msm_sort_count_ptrs_kernel, dim3((unsigned)n_wgs), dim3(MSM_BLOCK), 0, c->stream, polys->ptrs, d_points_inf, n, pl, pr, wg_counts);
        else hipLaunchKernelGGL(msm_sort_count_kernel, dim3((unsigned)n_wgs), dim3(MSM_BLOCK), 0, c->stream, d_scalars, d_points_inf, n, pl, pr, wg_counts);
        hipLaunchKernelGGL(msm_sort_bases_kernel, dim3((pl.n_parts + MSM_BLOCK / 64 - 1) / (MSM_BLOCK / 64)), dim3(MSM_BLOCK), 0, c->stream, wg_counts,
                           (uint32_t)n_wgs, pl.n_parts, part_count);
        hipLaunchKernelGGL(msm_sort_part_scan_kernel, dim3(1), dim3(1024), 0, c->stream, part_count, pl.n_parts, part_off);
        if (polys) hipLaunchKernelGGL(msm_sort_scatter_ptrs_kernel, dim3((unsigned)n_wgs), dim3(MSM_BLOCK), 0, c->stream, polys->ptrs, d_points_inf, n, pl, pr,
                                      wg_counts, part_off, items);
        else hipLaunchKernelGGL(msm_sort_scatter_kernel, dim3((unsigned)n_wgs), dim3(MSM_BLOCK), 0, c->stream, d_scalars, d_points_inf, n, pl, pr,
                                wg_counts, part_off, items);
        // level 2 also takes the histogram of the bucket counts (the order pass) and files the heavy buckets: both cleared here
        ZK_HIP(c, hipMemsetAsync(bins, 0, (size_t)(o_sorted - o_bins), c->stream));      // bins + MsmOverflow
        hipLaunchKernelGGL(msm_sort_local_kernel, dim3(pl.n_parts), dim3(SORT_LOCAL_BLOCK), 0, c->stream, items, part_off, pl, sorted, counts, offsets,
                           heavy_min, ovf, rec, (uint32_t)rec_cap, bins);
    }
    {
        // heavy buckets (none with uniform scalars: four empty launches): filed by the sort and summed by passes 4b / 4c IN
        // FRONT of the accumulate pass (on a second stream beside it they did not find a free slot for most of its duration -- its
        // first workgroups walk the longest lists and hold every register of the chip)
        ProfScope ps(c, "msm_overflow", 0.0);
        hipLaunchKernelGGL(msm_heavy_points_kernel, dim3(512) /* 64 KiB of LDS each: two per CU are resident, the records are walked in a loop */, dim3(MSM_BLOCK), MSM_BLOCK * 256, c->stream, points_u, sorted, ovf, rec,
                           partials, buckets);
        for (int level = 1; level < MSM_HEAVY_LEVELS; ++level)
            hipLaunchKernelGGL(msm_heavy_tree_kernel, dim3(level == 1 ? 256 : 16), dim3(MSM_BLOCK), MSM_BLOCK * 256, c->stream, ovf,
                               (uint32_t)level, rec + (size_t)level * rec_cap, partials, buckets);
    }
    {   // bucket order by descending point count
        ProfScope ps(c, "msm_order", 0.0);
        const unsigned gb = (unsigned)((n_buckets + MSM_BLOCK - 1) / MSM_BLOCK);
        hipLaunchKernelGGL(msm_order_scan_kernel, dim3(1), dim3(1024), 0, c->stream, bins);
        hipLaunchKernelGGL(msm_order_scatter_kernel, dim3(gb), dim3(MSM_BLOCK), 0, c->stream, counts, (uint32_t)n_buckets, bins, order);
    }
    {
        ProfScope ps(c, "msm_accumulate", 128.0 * (double)n);
        hipLaunchKernelGGL(msm_accumulate_kernel, dim3((unsigned)((n_buckets + MSM_BLOCK - 1) / MSM_BLOCK)), dim3(MSM_BLOCK), 0,
                           c->stream, points_u, sorted, offsets, counts, order, (uint32_t)n_buckets, heavy_min, buckets);
    }
    {
        ProfScope ps(c, "msm_segment", 0.0);
        hipLaunchKernelGGL(msm_segment_kernel, dim3((unsigned)((n_segments + MSM_BLOCK - 1) / MSM_BLOCK)), dim3(MSM_BLOCK), 0,
                           c->stream, buckets, (uint32_t)n_segments, segs, sega);
    }
    {
        ProfScope ps(c, "msm_terms", 0.0);
        // one wave per workgroup: lines and trees are summed inside a wave, without LDS
        hipLaunchKernelGGL(msm_rowcol_kernel, dim3(pl.n_rcwg), dim3(64), 0, c->stream, segs, sega, pl, rc);
        hipLaunchKernelGGL(msm_rowcol_terms_kernel, dim3(pl.n_termwg), dim3(64), 0, c->stream, rc, pl, terms);
    }
    ZK_HIP(c, hipGetLastError());
    ZK_TRY(c->reserve_msm_pin(slot, n_out * 192));
    ZK_HIP(c, hipMemcpyAsync(c->msm_pin[slot].ptr, terms, n_out * 192, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipEventRecord(c->msm_ev[slot].get(), c->stream));
    pend->geo = geo_p;
    pend->pr = pr;
    pend->n_out = n_out;
    pend->slot = slot;
    return ZKHIP_OK;
}
static int msm_finish(zkhip_ctx* c, const MsmPending& pend, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    ZK_HIP(c, hipEventSynchronize(c->msm_ev[pend.slot].get()));
    const MsmGeometry& geo = *pend.geo;
    const MsmProblems& pr = pend.pr;
    const uint64_t* h_terms = (const uint64_t*)c->msm_pin[pend.slot].ptr;
    // host epilogue, per problem: sum over its (set, term) points of 2^exp * point
    auto finish = [&](uint32_t j) {
        std::vector<zkhost::Xyzz> pts;
        std::vector<uint32_t> exps;
        for (uint32_t s = geo.prob_set_first[j]; s < geo.prob_set_first[j + 1]; ++s) {
            const uint32_t n_terms = (geo.sets[s].bits & 0xffu) - MSM_SEG_LOG;      // 1 + n_bits
            for (uint32_t t = 0; t < n_terms; ++t) {
                zkhost::Xyzz p;
                std::memcpy(&p, &h_terms[24 * ((size_t)geo.sets[s].term_base + t)], 192);
                pts.push_back(p);
                exps.push_back(geo.set_exp[s] + (t == 0 ? 0 : MSM_SEG_LOG + (t - 1)));
            }
        }
        zkhost::Xyzz res = zkhost::weighted_sum_pow2(pts, exps);
        h_out_inf[j] = zkhost::xyzz_to_affine(res, h_out_xy + 12 * (size_t)j) ? 0 : 1;
    };
    // the chains of different problems are independent (~0.25 ms each): a batch spreads them over the context's host threads, the
    // largest problems (most points) first
    ZkHostPool* pool = pr.n > 1 ? c->pool() : nullptr;
    if (!pool) {
        for (uint32_t j = 0; j < pr.n; ++j) finish(j);
    } else {
        pool->run(pr.n, [&](unsigned j) { finish(j); });
    }
    return ZKHIP_OK;
}
static int msm_commit_multi(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, const uint64_t* d_scalars, size_t n,
                            const MsmProblems& pr, uint64_t* h_out_xy, uint8_t* h_out_inf, const uint32_t* d_table = nullptr,
                            size_t table_stride = 0) {
    MsmPending pend;
    ZK_TRY(msm_enqueue(c, d_points_xy, d_points_inf, d_scalars, n, pr, d_table, table_stride, 0, 0, &pend, nullptr));
    return msm_finish(c, pend, h_out_xy, h_out_inf);
}
static int msm_commit(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, const uint64_t* d_scalars, size_t n,
                      uint64_t* h_out_xy, uint8_t* h_out_inf) {
    MsmProblems one = {};
    one.n = 1;
    one.off[1] = (uint32_t)n;
    return msm_commit_multi(c, d_points_xy, d_points_inf, d_scalars, n, one, h_out_xy, h_out_inf);
}

extern "C" int zkhip_kzg_commit(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf,
                                size_t n_points, const uint64_t* d_scalars, size_t n_scalars, int require_equal_len,
                                uint64_t* h_out_xy, uint8_t* h_out_inf) {
    if (!c || !h_out_xy || !h_out_inf) return ZKHIP_ERR_ARG;
    if (require_equal_len && n_points != n_scalars) return ZKHIP_ERR_SHAPE;   // multilinear_kzg.rs:36-41
    if (n_scalars > n_points) return ZKHIP_ERR_INDEX;                          // univariate_kzg.rs:53
    const size_t n = n_scalars;
    if (n == 0) { std::memset(h_out_xy, 0, 96); *h_out_inf = 1; return ZKHIP_OK; }   // P::G1::default()
    if (!d_points_xy || !d_scalars) return ZKHIP_ERR_ARG;
    if (n >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    return msm_commit(c, d_points_xy, d_points_inf, d_scalars, n, h_out_xy, h_out_inf);
}

// A table begins with a 128-byte HEADER (magic, kind, the number of points it was built for, its window widths, its number of entries):
// the layout of a table is a function of its size AND of a tuning variable read once per process (msm_level_table_widths), the kernels address
// it blindly, and a table built for another size -- or by a process that ran with another value -- would give a silently wrong commitment.
// zkhip_kzg_commit_table / _commit_begin / zkhip_kzg_open_tables compare the header with the geometry they are about to use (one 128-byte read
// the first time a (table, size) pair is seen in the process, remembered until a table is built at that address again) -> ZKHIP_ERR_ARG on a
// mismatch.  (Not re-read: a buffer the library did not build, placed at a remembered address.)
constexpr size_t ZK_TABLE_HEADER_BYTES = 128;
constexpr uint64_t ZK_TABLE_MAGIC = 0x31304c42544b5a00ull;       // "\0ZKTBL01"
enum : uint32_t { ZK_TABLE_SHIFTED_SRS = 1, ZK_TABLE_LEVELS = 2 };
struct ZkTableHeader {
    uint64_t magic;
    uint32_t kind, version;
    uint64_t n_points, entries;
    uint32_t W, hi, n_hi;          // the widths of the (first, largest) table
    uint32_t widths_hash;          // FNV-1a over (h, W, hi, n_hi) of every level (level tables)
    uint8_t pad_[ZK_TABLE_HEADER_BYTES - 48];
};
static_assert(sizeof(ZkTableHeader) == ZK_TABLE_HEADER_BYTES, "one 128-byte entry in front of the table");
// tables whose header has been compared with the geometry of (kind, n_points): one list per PROCESS (contexts are per thread and share
// SRS objects), forgotten whenever a table is built at that address again
namespace {
struct TableOk { const void* p; size_t n; uint32_t kind; int device; };
std::mutex g_table_ok_mutex;
std::vector<TableOk> g_table_ok;
bool table_remembered(const zkhip_ctx* c, const void* p, size_t n, uint32_t kind) {
    std::lock_guard<std::mutex> lk(g_table_ok_mutex);
    for (const auto& t : g_table_ok) if (t.p == p && t.n == n && t.kind == kind && t.device == c->device) return true;
    return false;
}
void table_remember(const zkhip_ctx* c, const void* p, size_t n, uint32_t kind) {
    std::lock_guard<std::mutex> lk(g_table_ok_mutex);
    if (g_table_ok.size() >= 64) g_table_ok.erase(g_table_ok.begin());
    g_table_ok.push_back(TableOk{p, n, kind, c->device});
}
void table_forget(const zkhip_ctx* c, const void* p) {
    std::lock_guard<std::mutex> lk(g_table_ok_mutex);
    for (size_t i = g_table_ok.size(); i-- > 0;) if (g_table_ok[i].p == p && g_table_ok[i].device == c->device) g_table_ok.erase(g_table_ok.begin() + i);
}
}  // namespace
// the owner is about to free (or reuse) the buffer of a shifted-SRS table or of level tables: its address is no longer a known table
extern "C" int zkhip_table_release(zkhip_ctx* c, const void* d_table) {
    if (!c || !d_table) return ZKHIP_ERR_ARG;
    table_forget(c, d_table);
    return ZKHIP_OK;
}
static size_t level_tables_first(size_t n_points, size_t* lvl_off);
static ZkTableHeader table_header_for(uint32_t kind, size_t n_points) {
    ZkTableHeader h;
    std::memset(&h, 0, sizeof(h));
    h.magic = ZK_TABLE_MAGIC; h.kind = kind; h.version = 1; h.n_points = n_points;
    uint32_t fnv = 2166136261u;
    auto mix = [&](uint32_t v) { for (int b = 0; b < 4; ++b) { fnv ^= (v >> (8 * b)) & 0xffu; fnv *= 16777619u; } };
    if (kind == ZK_TABLE_SHIFTED_SRS) {
        const MsmLevelWidths lw = msm_table_widths(n_points);
        h.W = lw.W; h.hi = lw.hi; h.n_hi = lw.n_hi; h.entries = (uint64_t)lw.W * n_points;
        mix((uint32_t)n_points); mix(lw.W); mix(lw.hi); mix(lw.n_hi);
    } else {
        const size_t first = level_tables_first(n_points, nullptr);
        for (size_t q = first; q >= 1; q /= 2) {
            const MsmLevelWidths lw = msm_level_table_widths(q, 2 * first - 1);
            if (q == first) { h.W = lw.W; h.hi = lw.hi; h.n_hi = lw.n_hi; }
            h.entries += (uint64_t)lw.W * q;
            mix((uint32_t)q); mix(lw.W); mix(lw.hi); mix(lw.n_hi);
        }
    }
    h.widths_hash = fnv;
    return h;
}
static int table_write_header(zkhip_ctx* c, void* d_table, uint32_t kind, size_t n_points) {
    const ZkTableHeader h = table_header_for(kind, n_points);
    ZK_HIP(c, hipMemcpy(d_table, &h, sizeof(h), hipMemcpyHostToDevice));      // (once per SRS; synchronous)
    table_remember(c, d_table, n_points, kind);
    return ZKHIP_OK;
}
// -> the table proper (behind the header), or nullptr with *rc set
static const uint32_t* table_check(zkhip_ctx* c, const void* d_table, uint32_t kind, size_t n_points, int* rc) {
    *rc = ZKHIP_OK;
    if (!table_remembered(c, d_table, n_points, kind)) {
        ZkTableHeader got;
        if (hipMemcpy(&got, d_table, sizeof(got), hipMemcpyDeviceToHost) != hipSuccess) { *rc = ZKHIP_ERR_HIP; return nullptr; }
        const ZkTableHeader want = table_header_for(kind, n_points);
        if (std::memcmp(&got, &want, 48) != 0) { *rc = ZKHIP_ERR_ARG; return nullptr; }     // not a table, another kind, another size, other widths
        table_remember(c, d_table, n_points, kind);
    }
    return (const uint32_t*)((const char*)d_table + ZK_TABLE_HEADER_BYTES);
}

// ---------------------------------------------------------------------------------------
// commits in flight: a commit is a throughput-bound accumulate pass followed by latency-bound reduction passes (chains of
// ~25 us point additions on a mostly idle chip) and a host epilogue; a prover that commits several polynomials in a row
// hides the latter behind the next commits' accumulate passes.  Three slots (2 / 3 / 4 in flight: 3.03 / 2.91 / 2.98 ms per 2^20-point
// commit; the accumulate pass and the sort are throughput work, only the reductions and the epilogue hide); same results as the synchronous calls.
// ---------------------------------------------------------------------------------------
extern "C" int zkhip_kzg_commit_begin(zkhip_ctx* c, const uint64_t* d_points_xy, const void* d_table_with_header, const uint8_t* d_points_inf,
                                      size_t n_points, const uint64_t* d_scalars, size_t n_scalars, int require_equal_len,
                                      uint32_t* ticket) {
    if (!c || !ticket || (!d_points_xy == !d_table_with_header)) return ZKHIP_ERR_ARG;
    if (require_equal_len && n_points != n_scalars) return ZKHIP_ERR_SHAPE;   // multilinear_kzg.rs:36-41
    if (n_scalars > n_points) return ZKHIP_ERR_INDEX;                          // univariate_kzg.rs:53
    const size_t n = n_scalars;
    if (n == 0 || !d_scalars) return ZKHIP_ERR_ARG;                           // nothing to overlap: use the synchronous call
    if (n >= ((size_t)1 << 31) || (d_table_with_header && n_points * msm_table_widths(n_points).W >= ((size_t)1 << 31))) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    const uint32_t* d_table = nullptr;
    if (d_table_with_header) {
        int trc = ZKHIP_OK;
        d_table = table_check(c, d_table_with_header, ZK_TABLE_SHIFTED_SRS, n_points, &trc);       // built for THESE n_points, with the widths used below?
        if (!d_table) return trc;
    }
    int slot = -1;
    bool any = false;
    for (int k = zkhip_ctx::ASYNC_SLOTS - 1; k >= 0; --k) { if (!c->async_pend[k]) slot = k; else any = true; }
    if (slot < 0) return ZKHIP_ERR_BUSY;
    MsmProblems one = {};
    one.n = 1;
    one.off[1] = (uint32_t)n;
    size_t used = 0;
    ZK_TRY(msm_enqueue(c, nullptr, nullptr, nullptr, n, one, (const uint32_t*)d_table, n_points, 0, 0, nullptr, &used));
    used = (used + 4095) & ~(size_t)4095;
    if (!any) {
        if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;
        ZK_TRY(c->reserve_ws(zkhip_ctx::ASYNC_SLOTS * used));
        c->async_region = std::max(used, c->ws.bytes / zkhip_ctx::ASYNC_SLOTS & ~(size_t)4095);
    } else if (used > c->async_region) {
        return ZKHIP_ERR_BUSY;            // a larger commit than the one in flight: end that one first
    }
    ZK_TRY(c->ensure_side_streams());
    std::unique_ptr<MsmPending, MsmPendingDelete> pend(new (std::nothrow) MsmPending());
    if (!pend) return ZKHIP_ERR_NOMEM;
    pend->ws_loan = ZkLoan(c->ws_loans);      // the workspace stays lent until the last commit in flight has ended
    hipStream_t const main_stream = c->stream;
    int rc = ZKHIP_OK;
    if (hipEventRecord(c->fork_ev.get(), main_stream) != hipSuccess || hipStreamWaitEvent(c->side[slot].get(), c->fork_ev.get(), 0) != hipSuccess) rc = ZKHIP_ERR_HIP;
    if (rc == ZKHIP_OK) {
        c->stream = c->side[slot].get();
        rc = msm_enqueue(c, d_points_xy, d_points_inf, d_scalars, n, one, (const uint32_t*)d_table, n_points, (size_t)slot * c->async_region, slot,
                         pend.get(), nullptr);
        c->stream = main_stream;
    }
    if (rc != ZKHIP_OK) {
        // a partially enqueued commit may have kernels running on the side stream: drain them before the slot, its workspace
        // region and its pinned buffer are handed out again
        hipStreamSynchronize(c->side[slot].get());
        return rc;
    }
    c->async_pend[slot] = std::move(pend);
    *ticket = (uint32_t)slot;
    return ZKHIP_OK;
}
extern "C" int zkhip_kzg_commit_end(zkhip_ctx* c, uint32_t ticket, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    if (!c || ticket >= (uint32_t)zkhip_ctx::ASYNC_SLOTS || !c->async_pend[ticket]) return ZKHIP_ERR_ARG;
    const std::unique_ptr<MsmPending, MsmPendingDelete> pend = std::move(c->async_pend[ticket]);     // ended (and its loan returned) on every exit
    int rc = c->activate();
    if (rc == ZKHIP_OK && h_out_xy && h_out_inf) rc = msm_finish(c, *pend, h_out_xy, h_out_inf);
    else if (hipStreamSynchronize(c->side[ticket].get()) != hipSuccess) rc = ZKHIP_ERR_HIP;            // abandoned: just drain it
    if (hipStreamWaitEvent(c->stream, c->msm_ev[ticket].get(), 0) != hipSuccess && rc == ZKHIP_OK) rc = ZKHIP_ERR_HIP;   // workspace reuse stays ordered
    return rc;
}

// ---------------------------------------------------------------------------------------
// SRS fingerprint: the first two and last two points with their infinity flags, in ONE launch and ONE copy
// ---------------------------------------------------------------------------------------
static __global__ void srs_fingerprint_kernel(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n, uint64_t* __restrict__ out) {
    const uint32_t t = threadIdx.x;                 // 52 threads: 4 points x (12 words + 1 flag)
    if (t >= 52) return;
    const uint32_t k = t / 13, w = t - 13 * k;
    const size_t idx[4] = {(size_t)0, n > 1 ? (size_t)1 : (size_t)0, n > 1 ? n - 2 : (size_t)0, n - 1};
    out[t] = w < 12 ? xy[12 * idx[k] + w] : (inf ? (uint64_t)inf[idx[k]] : 0);
}
extern "C" int zkhip_srs_fingerprint(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n_points, uint64_t* h_out) {
    if (!c || !d_points_xy || !h_out) return ZKHIP_ERR_ARG;
    if (n_points == 0) { std::memset(h_out, 0, 52 * 8); return ZKHIP_OK; }
    ZK_TRY(c->activate());
    if (!c->d_fingerprint) ZK_HIP(c, dev_alloc(c->d_fingerprint, 512));      // a buffer of its own: commits in flight hold the workspace
    // a stream of the highest priority: with commits in flight the one-wave kernel takes the next slot that frees instead of queueing
    // behind the thousands of workgroups of an accumulate pass (109 us per call on the caller's stream, rocprofv3 of the bench's in-flight leg)
    ZK_HIP(c, ensure_stream(c->guard_stream, Prio::High));
    ZK_HIP(c, ensure_event(c->guard_ev));
    uint64_t* pin = c->pinned_u64(ZK_PIN_PTS);      // (evaluation points' staging area: no prover runs during this call)
    static_assert(ZK_PIN_PROOF - ZK_PIN_PTS >= 52, "staging area too small");
    ZK_HIP(c, hipEventRecord(c->guard_ev.get(), c->stream));                         // behind whatever the caller's stream still does to the SRS
    ZK_HIP(c, hipStreamWaitEvent(c->guard_stream.get(), c->guard_ev.get(), 0));
    hipLaunchKernelGGL(srs_fingerprint_kernel, dim3(1), dim3(64), 0, c->guard_stream.get(), d_points_xy, d_points_inf, n_points, (uint64_t*)c->d_fingerprint.get());
    ZK_HIP(c, hipMemcpyAsync(pin, c->d_fingerprint.get(), 52 * 8, hipMemcpyDeviceToHost, c->guard_stream.get()));
    ZK_HIP(c, hipStreamSynchronize(c->guard_stream.get()));
    std::memcpy(h_out, pin, 52 * 8);
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------
// shifted-SRS table: commitments with one bucket set for all windows
// ---------------------------------------------------------------------------------------
extern "C" size_t zkhip_srs_table_bytes(size_t n_points) { return n_points ? ZK_TABLE_HEADER_BYTES + n_points * msm_table_widths(n_points).W * 128 : 0; }

// windows 0 .. n_windows-1 of c bits over n affine points: table entry w * n + i = 2^(c w) * point i (internal 28-bit-limb layout, 128 bytes);
// the context's workspace holds one window in XYZZ and affine form meanwhile
static int build_shift_table(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n, uint32_t width, uint32_t n_windows,
                             uint32_t* table, uint32_t n_wide = ~0u /* windows >= n_wide are width - 1 bits */) {
    // workspace: XYZZ of one window (192 n) | affine (96 n) | infinity flags (n)
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_xyzz = 0, o_aff = al(192 * n), o_inf = o_aff + al(96 * n);
    ZK_TRY(c->reserve_ws(o_inf + al(n)));
    char* ws = (char*)c->ws.ptr;
    const unsigned grid = (unsigned)((n + MSM_BLOCK - 1) / MSM_BLOCK);
    hipLaunchKernelGGL(msm_convert_points_kernel, dim3(std::min<unsigned>(grid, 256 * 8)), dim3(MSM_BLOCK), 0, c->stream, d_points_xy, n, table);
    if (d_points_inf) {   // entries of points at infinity: all-zero coordinates (their scalars are skipped by the sort anyway)
        hipLaunchKernelGGL(msm_clear_inf_kernel, dim3(grid), dim3(MSM_BLOCK), 0, c->stream, d_points_inf, n, table);
    }
    const size_t n_threads = (n + SRS_CHUNK - 1) / SRS_CHUNK;
    for (uint32_t w = 1; w < n_windows; ++w) {
        const uint32_t* prev = table + (size_t)(w - 1) * n * 32;
        uint32_t* cur = table + (size_t)w * n * 32;
        hipLaunchKernelGGL(msm_shift_points_kernel, dim3(grid), dim3(MSM_BLOCK), 0, c->stream, prev, n, w - 1 < n_wide ? width : width - 1,
                           (uint64_t*)(ws + o_xyzz));
        hipLaunchKernelGGL(srs_batch_affine_kernel, dim3((unsigned)((n_threads + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0, c->stream,
                           (const uint64_t*)(ws + o_xyzz), n, (uint64_t*)(ws + o_aff), (uint8_t*)(ws + o_inf));
        hipLaunchKernelGGL(msm_convert_points_kernel, dim3(std::min<unsigned>(grid, 256 * 8)), dim3(MSM_BLOCK), 0, c->stream,
                           (const uint64_t*)(ws + o_aff), n, cur);
    }
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}
extern "C" int zkhip_srs_precompute(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n,
                                    void* d_table) {
    if (!c || !d_points_xy || !d_table) return ZKHIP_ERR_ARG;
    if (n == 0) return ZKHIP_OK;
    const MsmLevelWidths lw = msm_table_widths(n);
    if (n * lw.W >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;   // entry index + sign bit in 32 bits
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;      // before the address is forgotten as a table: a refused rebuild leaves the old one in use
    ZK_TRY(c->activate());
    table_forget(c, d_table);
    ZK_TRY(build_shift_table(c, d_points_xy, d_points_inf, n, lw.hi, lw.W, (uint32_t*)((char*)d_table + ZK_TABLE_HEADER_BYTES), lw.n_hi));
    ZK_HIP(c, hipStreamSynchronize(c->stream));   // the workspace is reused by the next call
    return table_write_header(c, d_table, ZK_TABLE_SHIFTED_SRS, n);      // last: a table whose build failed carries no valid header
}

// LEVEL TABLES: shifted tables of the folded SRS levels MultilinearKZG::open commits against in ONE batch (the levels of at most
// OPEN_BATCH_MAX points), each with the window widths of msm_level_table_widths, end to end in level order (msm_geometry.hpp).
constexpr size_t OPEN_BATCH_MAX_DEFAULT = (size_t)1 << 19;
constexpr size_t MSM_SMALL_MAX = 4096;          // commits / openings of at most this many scalars take the short path (msm_small_batch)
static size_t level_tables_first(size_t n_points, size_t* lvl_off) {   // size of the first (largest) level that has a table; *lvl_off = its offset in the folded array
    size_t h = n_points / 2, off = 0;
    while (h > OPEN_BATCH_MAX_DEFAULT) { off += h; h /= 2; }
    if (lvl_off) *lvl_off = off;
    return h;
}
extern "C" size_t zkhip_srs_level_tables_bytes(size_t n_points) {
    if (n_points < 2 || !is_pow2(n_points)) return 0;
    size_t entries = 0;
    const size_t first = level_tables_first(n_points, nullptr);
    for (size_t h = first; h >= 1; h /= 2) entries += (size_t)msm_level_table_widths(h, 2 * first - 1).W * h;
    return ZK_TABLE_HEADER_BYTES + entries * 128;
}
extern "C" int zkhip_srs_level_tables(zkhip_ctx* c, const uint64_t* d_folded_xy, const uint8_t* d_folded_inf, size_t n_points, void* d_tables_with_header) {
    if (!c || !d_folded_xy || !d_folded_inf || !d_tables_with_header) return ZKHIP_ERR_ARG;
    if (n_points < 2 || !is_pow2(n_points)) return ZKHIP_ERR_SHAPE;
    if (zkhip_srs_level_tables_bytes(n_points) / 128 >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;      // (as zkhip_srs_precompute)
    ZK_TRY(c->activate());
    table_forget(c, d_tables_with_header);
    void* d_tables = (char*)d_tables_with_header + ZK_TABLE_HEADER_BYTES;
    size_t off = 0, entry = 0;
    const size_t first = level_tables_first(n_points, &off);
    if (n_points <= MSM_SMALL_MAX) {
        // a small SRS: every level in one go (msm_small_level_windows_kernel) -- a few ms instead of 0.3-0.4 s, so that a small opening can
        // build its tables on first use
        MsmSmallTabArgs a = {};
        for (size_t h = first; h >= 1; h /= 2) {
            const MsmLevelWidths lw = msm_level_table_widths(h, 2 * first - 1);
            const uint32_t j = a.n_levels++;
            a.h[j] = (uint32_t)h; a.pt_off[j] = a.total_points; a.tab_off[j] = (uint32_t)entry; a.W[j] = lw.W; a.hi[j] = lw.hi; a.n_hi[j] = lw.n_hi;
            a.total_points += (uint32_t)h;
            entry += (size_t)lw.W * h;
        }
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_pts = 0, o_xyzz = al(128 * (size_t)a.total_points), o_aff = o_xyzz + al(192 * entry), o_inf = o_aff + al(96 * entry);
        ZK_TRY(c->reserve_ws(o_inf + al(entry)));
        char* ws = (char*)c->ws.ptr;
        uint32_t* d_pts = (uint32_t*)(ws + o_pts);
        hipLaunchKernelGGL(msm_convert_points_kernel, dim3((a.total_points + MSM_BLOCK - 1) / MSM_BLOCK), dim3(MSM_BLOCK), 0, c->stream, d_folded_xy + 12 * off,
                           (size_t)a.total_points, d_pts);
        hipLaunchKernelGGL(msm_clear_inf_kernel, dim3((a.total_points + MSM_BLOCK - 1) / MSM_BLOCK), dim3(MSM_BLOCK), 0, c->stream, d_folded_inf + off,
                           (size_t)a.total_points, d_pts);
        hipLaunchKernelGGL(msm_small_level_windows_kernel, dim3((a.total_points + 63) / 64), dim3(64), 0, c->stream, a, (const uint32_t*)d_pts, (uint64_t*)(ws + o_xyzz));
        const size_t n_threads = (entry + SRS_CHUNK - 1) / SRS_CHUNK;
        hipLaunchKernelGGL(srs_batch_affine_kernel, dim3((unsigned)((n_threads + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0, c->stream,
                           (const uint64_t*)(ws + o_xyzz), entry, (uint64_t*)(ws + o_aff), (uint8_t*)(ws + o_inf));
        const unsigned grid = (unsigned)((entry + MSM_BLOCK - 1) / MSM_BLOCK);
        hipLaunchKernelGGL(msm_convert_points_kernel, dim3(std::min<unsigned>(grid, 256 * 8)), dim3(MSM_BLOCK), 0, c->stream, (const uint64_t*)(ws + o_aff), entry,
                           (uint32_t*)d_tables);
        hipLaunchKernelGGL(msm_clear_inf_kernel, dim3(grid), dim3(MSM_BLOCK), 0, c->stream, (const uint8_t*)(ws + o_inf), entry, (uint32_t*)d_tables);
        ZK_HIP(c, hipGetLastError());
        ZK_HIP(c, hipStreamSynchronize(c->stream));
        return table_write_header(c, d_tables_with_header, ZK_TABLE_LEVELS, n_points);
    }
    for (size_t h = first; h >= 1; h /= 2) {
        const MsmLevelWidths lw = msm_level_table_widths(h, 2 * first - 1);      // the batch: the levels first, first / 2, ..., 1
        const uint32_t W = lw.W;
        ZK_TRY(build_shift_table(c, d_folded_xy + 12 * off, d_folded_inf + off, h, lw.hi, W, (uint32_t*)d_tables + entry * 32, lw.n_hi));
        off += h;
        entry += (size_t)W * h;
    }
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return table_write_header(c, d_tables_with_header, ZK_TABLE_LEVELS, n_points);
}

// Commits of at most MSM_SMALL_MAX scalars against a shifted-SRS table: the plane sums of msm_kernels.hpp "commits of a few thousand
// points" -- two launches, one copy, a host epilogue of <= 20 doublings.  ZKHIP_MSM_SMALL=0 keeps the bucket pipeline (A/B runs).
// The launches' arguments: a geometry (msm_small_plan.hpp: the problems, the slot rule, the workspace) and the caller's pointers.
static MsmSmallArgs msm_small_args(const MsmSmallGeometry& g, const uint32_t* table, const uint8_t* inf, const uint64_t* scalars, void* partials, void* terms) {
    MsmSmallArgs a = {};
    a.table = table; a.inf = inf; a.scalars = scalars; a.partials = (uint32_t*)partials; a.terms = (uint64_t*)terms;
    a.nprob = g.nprob; a.planes = g.planes; a.total_slots = g.total_slots;
    std::memcpy(a.n, g.n, sizeof a.n); std::memcpy(a.stride, g.stride, sizeof a.stride); std::memcpy(a.W, g.W, sizeof a.W);
    std::memcpy(a.hi, g.hi, sizeof a.hi); std::memcpy(a.n_hi, g.n_hi, sizeof a.n_hi); std::memcpy(a.tab_off, g.tab_off, sizeof a.tab_off);
    std::memcpy(a.sc_off, g.sc_off, sizeof a.sc_off); std::memcpy(a.slot_first, g.slot_first, sizeof a.slot_first);
    return a;
}
// The end of a chunk: ONE copy of its terms (and what lies behind them) into the pinned buffer behind ONE synchronisation ...
static int msm_small_fetch(zkhip_ctx* c, const void* d_terms, size_t bytes) {
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(c->msm_pin[0].ptr, d_terms, bytes, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return ZKHIP_OK;
}
// ... and the host fold of its `count` problems (msm_small_fold.hpp): result k to out_of(k)
template <class OutOf>
static void msm_small_finish(zkhip_ctx* c, const MsmSmallGeometry& g, uint32_t count, uint64_t* h_out_xy, uint8_t* h_out_inf, OutOf out_of) {
    msm_small_fold((const char*)c->msm_pin[0].ptr, g, count, count > 1 ? c->pool() : nullptr, h_out_xy, h_out_inf, out_of);
}
// problem j of pr: results h_out_xy[12 j], h_out_inf[j]
static int msm_small_batch(zkhip_ctx* c, const uint32_t* d_table, const uint8_t* d_inf, const uint64_t* d_scalars, const MsmSmallProblem* pr,
                           uint32_t nprob, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    if (nprob == 0 || nprob > (uint32_t)MSM_SMALL_PROBS) return ZKHIP_ERR_SHAPE;
    const MsmSmallGeometry g = msm_small_plan(pr, nprob, 1);
    const size_t terms_bytes = g.terms_bytes(1);
    const MsmSmallCarve cv = msm_small_carve(g.part_bytes(1), terms_bytes);
    ZK_TRY(c->reserve_ws(cv.ws_bytes));
    ZK_TRY(c->reserve_msm_pin(0, terms_bytes));
    const MsmSmallArgs a = msm_small_args(g, d_table, d_inf, d_scalars, c->ws.ptr, (char*)c->ws.ptr + cv.terms_off);
    {
        ProfScope ps(c, "msm_small", 128.0 * (double)g.total_pairs / std::max<uint32_t>(1, a.W[0]));
        hipLaunchKernelGGL(msm_small_planes_kernel, dim3(a.total_slots, a.planes), dim3(64), 0, c->stream, a);
        hipLaunchKernelGGL(msm_small_reduce_kernel, dim3(a.planes, nprob), dim3(64), 0, c->stream, a);
    }
    ZK_TRY(msm_small_fetch(c, a.terms, terms_bytes));
    msm_small_finish(c, g, nprob, h_out_xy, h_out_inf, [](uint32_t j) { return (size_t)j; });
    return ZKHIP_OK;
}
static int msm_commit_small(zkhip_ctx* c, const uint32_t* d_table, size_t stride, const uint8_t* d_inf, const uint64_t* d_scalars, size_t n,
                            uint64_t* h_out_xy, uint8_t* h_out_inf) {
    const MsmSmallProblem one = {n, stride, 0, 0, msm_table_widths(stride)};
    return msm_small_batch(c, d_table, d_inf, d_scalars, &one, 1, h_out_xy, h_out_inf);
}
static bool msm_small_on() { static const bool on = env::read(env::MSM_SMALL) != 0; return on; }

extern "C" int zkhip_kzg_commit_table(zkhip_ctx* c, const void* d_table_with_header, const uint8_t* d_points_inf, size_t n_points,
                                      const uint64_t* d_scalars, size_t n_scalars, int require_equal_len, uint64_t* h_out_xy,
                                      uint8_t* h_out_inf) {
    if (!c || !h_out_xy || !h_out_inf) return ZKHIP_ERR_ARG;
    if (require_equal_len && n_points != n_scalars) return ZKHIP_ERR_SHAPE;   // multilinear_kzg.rs:36-41
    if (n_scalars > n_points) return ZKHIP_ERR_INDEX;                          // univariate_kzg.rs:53
    const size_t n = n_scalars;
    if (n == 0) { std::memset(h_out_xy, 0, 96); *h_out_inf = 1; return ZKHIP_OK; }
    if (!d_table_with_header || !d_scalars) return ZKHIP_ERR_ARG;
    if (n_points * msm_table_widths(n_points).W >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    int trc = ZKHIP_OK;
    const uint32_t* d_table = table_check(c, d_table_with_header, ZK_TABLE_SHIFTED_SRS, n_points, &trc);     // built for THESE n_points, with the widths used below?
    if (!d_table) return trc;
    if (msm_small_on() && n <= MSM_SMALL_MAX) return msm_commit_small(c, (const uint32_t*)d_table, n_points, d_points_inf, d_scalars, n, h_out_xy, h_out_inf);
    MsmProblems one = {};
    one.n = 1;
    one.off[1] = (uint32_t)n;
    return msm_commit_multi(c, nullptr, d_points_inf, d_scalars, n, one, h_out_xy, h_out_inf, (const uint32_t*)d_table, n_points);
}

extern "C" int zkhip_msm_geometry_info(const size_t* h_offsets, uint32_t n_problems, uint16_t* h_win_first, uint8_t* h_win_bits,
                                       uint32_t* h_totals) {
    if (!h_offsets || !h_win_first || !h_win_bits || !h_totals) return ZKHIP_ERR_ARG;
    if (n_problems == 0 || n_problems > (uint32_t)MSM_MAX_PROBLEMS) return ZKHIP_ERR_SHAPE;
    MsmProblems pr = {};
    pr.n = n_problems;
    for (uint32_t j = 0; j <= n_problems; ++j) {
        if (h_offsets[j] >= ((size_t)1 << 31) || (j && h_offsets[j] < h_offsets[j - 1])) return ZKHIP_ERR_SHAPE;
        pr.off[j] = (uint32_t)(h_offsets[j] - h_offsets[0]);
    }
    MsmGeometry g;
    ZK_TRY(msm_build_geometry(pr, false, 0, g));
    for (uint32_t j = 0; j <= n_problems; ++j) h_win_first[j] = g.win_first[j];
    for (size_t v = 0; v < g.wins.size(); ++v) h_win_bits[v] = (uint8_t)(g.wins[v].bits & 0xffu);
    const uint32_t totals[8] = {g.pl.n_wins, g.pl.n_sets, g.pl.n_buckets, g.pl.n_parts, g.pl.n_terms, g.pl.n_rcwg, g.pl.n_termwg, g.heavy_min};
    std::memcpy(h_totals, totals, sizeof(totals));
    return ZKHIP_OK;
}

extern "C" int zkhip_kzg_commit_batch(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf,
                                      const uint64_t* d_scalars, const size_t* h_offsets, uint32_t n_problems, uint64_t* h_out_xy,
                                      uint8_t* h_out_inf) {
    if (!c || !h_offsets || !h_out_xy || !h_out_inf) return ZKHIP_ERR_ARG;
    if (n_problems == 0) return ZKHIP_OK;
    if (n_problems > (uint32_t)MSM_MAX_PROBLEMS) return ZKHIP_ERR_SHAPE;
    MsmProblems pr = {};
    pr.n = n_problems;
    for (uint32_t j = 0; j <= n_problems; ++j) {
        if (h_offsets[j] >= ((size_t)1 << 31) || (j && h_offsets[j] < h_offsets[j - 1])) return ZKHIP_ERR_SHAPE;
        pr.off[j] = (uint32_t)(h_offsets[j] - h_offsets[0]);
    }
    const size_t n = pr.off[n_problems];
    if (n == 0) {
        for (uint32_t j = 0; j < n_problems; ++j) { std::memset(h_out_xy + 12 * (size_t)j, 0, 96); h_out_inf[j] = 1; }
        return ZKHIP_OK;
    }
    if (!d_points_xy || !d_scalars) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    const size_t o = h_offsets[0];
    return msm_commit_multi(c, d_points_xy + 12 * o, d_points_inf ? d_points_inf + o : nullptr, d_scalars + 4 * o, n, pr, h_out_xy, h_out_inf);
}

// ---------------------------------------------------------------------------------------
// MultilinearKZG::open
// ---------------------------------------------------------------------------------------
// folded SRS levels S_0 .. S_{nv-1} (n - 1 affine points); d_tmp_xyzz: (n - 1) x 192 bytes of scratch
static int fold_srs_levels(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n, uint64_t* d_tmp_xyzz,
                           uint64_t* d_out_xy, uint8_t* d_out_inf) {
    size_t h = n / 2, off = 0;
    hipLaunchKernelGGL(srs_fold_affine_kernel, dim3((unsigned)((h + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0, c->stream,
                       d_points_xy, d_points_inf, h, d_tmp_xyzz);
    while (h > 1) {
        const size_t next = off + h;
        h /= 2;
        hipLaunchKernelGGL(srs_fold_xyzz_kernel, dim3((unsigned)((h + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0, c->stream,
                           d_tmp_xyzz + 24 * off, h, d_tmp_xyzz + 24 * next);
        off = next;
    }
    const size_t total = n - 1, n_threads = (total + SRS_CHUNK - 1) / SRS_CHUNK;
    hipLaunchKernelGGL(srs_batch_affine_kernel, dim3((unsigned)((n_threads + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0, c->stream,
                       d_tmp_xyzz, total, d_out_xy, d_out_inf);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

extern "C" int zkhip_srs_fold_levels(zkhip_ctx* c, const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n_points,
                                     uint64_t* d_out_xy, uint8_t* d_out_inf) {
    if (!c || !d_points_xy || !d_out_xy || !d_out_inf) return ZKHIP_ERR_ARG;
    if (n_points < 2 || !is_pow2(n_points)) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    ZK_TRY(c->reserve_ws((n_points - 1) * 192));
    return fold_srs_levels(c, d_points_xy, d_points_inf, n_points, (uint64_t*)c->ws.ptr, d_out_xy, d_out_inf);
}

extern "C" int zkhip_kzg_open(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_points, size_t n_eval_points,
                              const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n_points,
                              const uint64_t* d_folded_xy, const uint8_t* d_folded_inf, uint64_t* h_evaluation,
                              uint64_t* h_proofs_xy, uint8_t* h_proofs_inf) {
    return zkhip_kzg_open_tables(c, d_evals, n, h_points, n_eval_points, d_points_xy, d_points_inf, n_points, d_folded_xy, d_folded_inf, nullptr,
                                 h_evaluation, h_proofs_xy, h_proofs_inf);
}
static bool open_pipelines_on() { static const bool on = env::read(env::OPEN_PIPELINES) != 0; return on; }
// the shape and argument checks of an opening, shared by zkhip_kzg_open_tables and zkhip_kzg_open_batch (applied once per call, before
// anything is launched); *d_level_tables <- the tables behind their checked header, or nullptr
static int kzg_open_check(zkhip_ctx* c, size_t n, size_t n_eval_points, size_t n_points, const uint64_t* d_folded_xy, const uint8_t* d_folded_inf,
                          const void* d_level_tables_with_header, uint32_t* n_vars_out, const void** d_level_tables) {
    if (d_level_tables_with_header && !d_folded_inf) return ZKHIP_ERR_ARG;      // the tables belong to cached folded levels
    if (!is_pow2(n)) return ZKHIP_ERR_SHAPE;
    const uint32_t n_vars = log2_exact(n);
    if (n_eval_points != n_vars) return ZKHIP_ERR_SHAPE;   // evaluation_form.rs:163-167
    if (n_points != n) return ZKHIP_ERR_SHAPE;             // multilinear_kzg.rs:36-41
    if (n_vars < 2) return ZKHIP_ERR_SHAPE;                // :73 `variable_index - 1` underflows
    if (n >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;
    if ((d_folded_xy == nullptr) != (d_folded_inf == nullptr)) return ZKHIP_ERR_ARG;
    // every round's commit needs the workspace: an opening beside a commit in flight or a split-phase session is refused here, before the
    // quotient area is reserved (which may move it), the quotient chain is launched and the SRS is folded
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;
    ZK_TRY(c->activate());
    *d_level_tables = nullptr;
    if (d_level_tables_with_header) {
        int trc = ZKHIP_OK;
        *d_level_tables = table_check(c, d_level_tables_with_header, ZK_TABLE_LEVELS, n_points, &trc);   // the level tables of an SRS of THIS size, with the widths used below?
        if (!*d_level_tables) return trc;
    }
    *n_vars_out = n_vars;
    return ZKHIP_OK;
}
// one opening behind kzg_open_check (d_level_tables: behind the header)
static int kzg_open_one(zkhip_ctx* c, const uint64_t* d_evals, size_t n, uint32_t n_vars, const uint64_t* h_points,
                        const uint64_t* d_points_xy, const uint8_t* d_points_inf, const uint64_t* d_folded_xy, const uint8_t* d_folded_inf,
                        const void* d_level_tables, uint64_t* h_evaluation, uint64_t* h_proofs_xy, uint8_t* h_proofs_inf) {
    // aux layout: quotients of all rounds (n - 1, laid out like the folded SRS) | remainder ping (n/2) | pong (n/4) |
    // [folded SRS xy, inf]
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_q = 0, o_ping = o_q + al(n * 32), o_pong = o_ping + al(n / 2 * 32);
    const size_t o_fxy = o_pong + al((n / 4 + 1) * 32), o_finf = o_fxy + al((n - 1) * 96);
    const bool own_fold = d_folded_xy == nullptr;
    ZK_TRY(c->reserve_aux(own_fold ? o_finf + al(n - 1) : o_fxy));
    char* aux = (char*)c->aux.ptr;
    if (own_fold) {
        ZK_TRY(c->reserve_ws((n - 1) * 192));
        ProfScope ps(c, "open_fold_srs", 0.0);
        ZK_TRY(fold_srs_levels(c, d_points_xy, d_points_inf, n, (uint64_t*)c->ws.ptr, (uint64_t*)(aux + o_fxy), (uint8_t*)(aux + o_finf)));
        d_folded_xy = (const uint64_t*)(aux + o_fxy);
        d_folded_inf = (const uint8_t*)(aux + o_finf);
    }
    uint64_t* d_q = (uint64_t*)(aux + o_q);
    // All quotients first (a chain of n_vars small kernels on the caller's stream; none of them depends on a commit).  Then the commits:
    // every round with at most 2^19 quotient entries -- all twenty of a 2^20 opening -- as problems of ONE batched commit, each with a
    // window width of its own (msm_build_geometry), on the caller's stream: one pass of every MSM kernel, each filling the chip, one
    // bucket reduction.  Larger rounds (openings above 2^20) are commits of their own, two in flight on side streams beside the batch.
    // (History.  Rounds 1-3: every round above 2^14 as a commit pipeline of its own, five beside each other on three hardware queues, each
    // paying the full reduction of 2^19 buckets and every kernel running at 2-3 x its stand-alone duration beside the others' accumulate
    // passes: 8.5-9.2 ms at 2^20 against 3.2 ms for ONE commit of as many points (profiles/r03/open_trace_pipelines.txt).  Then three
    // batches of one width each (14 / 12 / 10 bits) beside each other, fronts lined up: 6.7 ms -- their sparse top windows needed the
    // heavy-bucket passes (0.6 ms) and the three reductions ended 0.9 ms after the last accumulate pass.  ZKHIP_OPEN_PIPELINES=1 runs the
    // rounds above 2^14 as pipelines again for an A/B.)
    const bool pipelines = open_pipelines_on();
    const size_t OPEN_BATCH_MAX = pipelines ? (size_t)1 << 14 : OPEN_BATCH_MAX_DEFAULT;
    if (pipelines) d_level_tables = nullptr;    // the tables are laid out for the default batch
    // result slot / stream of the single commits (they rotate over the slots); the batch has the last slot
    const int NSLOT = pipelines ? 5 : 2;
    const int sl_batch = zkhip_ctx::MSM_SLOTS - 1;
    const uint64_t* cur = d_evals;
    size_t cn = n, lvl_off = 0;
    MsmProblems batch = {};
    size_t batch_first_off = 0;
    uint32_t batch_first_round = 0;
    struct Large { uint32_t round; size_t off, h; };
    std::vector<Large> large;
    // (a small opening against its tables -- the short path below -- takes all its rounds in ONE launch: a dozen 5 us launches otherwise)
    const bool small_open = d_level_tables && n <= MSM_SMALL_MAX && !pipelines && msm_small_on() && n_vars <= (uint32_t)ZK_MAX_ROUNDS;
    if (small_open) {
        PtsArg zp = {};
        std::memcpy(zp.v, h_points, 32 * (size_t)n_vars);
        hipLaunchKernelGGL(open_steps_small_kernel, dim3(1), dim3(MLE_BLOCK), 0, c->stream, d_evals, (uint32_t)n, zp, n_vars, d_q, (uint64_t*)(aux + o_ping),
                           (uint64_t*)(aux + o_pong));
    }
    for (uint32_t i = 0; i < n_vars; ++i) {
        FrArg z = {};
        std::memcpy(z.v, h_points + 4 * (size_t)i, 32);
        uint64_t* rem = (uint64_t*)(aux + ((i & 1) ? o_pong : o_ping));
        if (!small_open)
            hipLaunchKernelGGL(open_step_kernel, dim3(mle_grid_stream(cn / 2)), dim3(MLE_BLOCK), 0, c->stream, cur, cn, z, d_q + 4 * lvl_off, rem);
        const size_t h = cn / 2;   // |q_i| = |S_i|
        if (h > OPEN_BATCH_MAX) {
            large.push_back({i, lvl_off, h});
        } else {                   // the batched rounds follow each other, so the problems lie end to end
            if (batch.n == 0) { batch_first_off = lvl_off; batch_first_round = i; }
            batch.off[batch.n] = (uint32_t)(lvl_off - batch_first_off);
            batch.off[++batch.n] = (uint32_t)(lvl_off + h - batch_first_off);
        }
        lvl_off += h;
        cur = rem;
        cn = h;
    }
    ZK_HIP(c, hipGetLastError());
    if (small_open && large.empty() && batch.n && batch.n <= (uint32_t)MSM_SMALL_PROBS) {
        // a small opening against its level tables: every round's quotient commit is a plain sum per digit bit (msm_small_batch) --
        // two launches for all rounds instead of the bucket pipeline's seventeen (0.96 -> 0.6x ms at 2^12)
        MsmSmallProblem sp[MSM_SMALL_PROBS];
        const size_t total = batch.off[batch.n];
        size_t entry = 0;
        for (uint32_t j = 0; j < batch.n; ++j) {
            const size_t h = batch.off[j + 1] - batch.off[j];
            const MsmLevelWidths lw = msm_level_table_widths(h, total);          // as zkhip_srs_level_tables laid the level out
            sp[j] = {h, h, entry, batch_first_off + batch.off[j], lw};
            entry += (size_t)lw.W * h;
        }
        ZK_TRY(msm_small_batch(c, (const uint32_t*)d_level_tables, d_folded_inf, d_q, sp, batch.n, h_proofs_xy + 12 * (size_t)batch_first_round,
                               h_proofs_inf + batch_first_round));
        ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), cur, 32, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipStreamSynchronize(c->stream));
        std::memcpy(h_evaluation, c->pinned_u64(ZK_PIN_RES), 32);
        return ZKHIP_OK;
    }
    // workspace: region k (k < NSLOT) is sized for the k-th single commit and reused by the commits k + NSLOT, k + 2 NSLOT, ... (each
    // half the size of its predecessor in the region or less); the batch has a region of its own.  Reserved once, up front: a
    // commit that grew the workspace later would move it under the commits in flight.
    size_t region_off[zkhip_ctx::MSM_SLOTS + 1] = {};
    for (int k = 0; k < NSLOT; ++k) {
        size_t used = 0;
        if ((size_t)k < large.size()) {
            MsmProblems one = {};
            one.n = 1;
            one.off[1] = (uint32_t)large[k].h;
            ZK_TRY(msm_enqueue(c, nullptr, nullptr, nullptr, large[k].h, one, nullptr, 0, 0, 0, nullptr, &used));
        }
        region_off[k + 1] = region_off[k] + ((used + 4095) & ~(size_t)4095);
    }
    {
        size_t used = 0;
        if (batch.n) ZK_TRY(msm_enqueue(c, nullptr, nullptr, nullptr, lvl_off - batch_first_off, batch, (const uint32_t*)d_level_tables, 0, 0, 0, nullptr, &used));
        ZK_TRY(c->reserve_ws(region_off[NSLOT] + used));
    }
    ZK_TRY(c->ensure_side_streams());
    ZK_HIP(c, hipEventRecord(c->fork_ev.get(), c->stream));
    MsmPending pend[zkhip_ctx::MSM_SLOTS];
    int pend_round[zkhip_ctx::MSM_SLOTS];
    for (int k = 0; k < zkhip_ctx::MSM_SLOTS; ++k) pend_round[k] = -1;
    auto finish_slot = [&](int sl) -> int {
        if (pend_round[sl] < 0) return ZKHIP_OK;
        const int r = pend_round[sl];
        pend_round[sl] = -1;
        return msm_finish(c, pend[sl], h_proofs_xy + 12 * (size_t)r, h_proofs_inf + r);
    };
    hipStream_t const main_stream = c->stream;
    int rc = ZKHIP_OK;
    if (batch.n) {
        // on the caller's stream (nothing else runs there meanwhile); pipelines: on a side stream, and FIRST -- its chain of passes is the longest
        hipStream_t on = pipelines ? c->side[sl_batch].get() : main_stream;
        if (on != main_stream && hipStreamWaitEvent(on, c->fork_ev.get(), 0) != hipSuccess) rc = ZKHIP_ERR_HIP;
        if (rc == ZKHIP_OK) {
            c->stream = on;                                // msm_enqueue launches on the context's stream
            rc = msm_enqueue(c, d_folded_xy + 12 * batch_first_off, d_folded_inf + batch_first_off, d_q + 4 * batch_first_off,
                             lvl_off - batch_first_off, batch, (const uint32_t*)d_level_tables, 0, region_off[NSLOT], sl_batch, &pend[sl_batch], nullptr);
            c->stream = main_stream;
            if (rc == ZKHIP_OK) pend_round[sl_batch] = (int)batch_first_round;
        }
    }
    for (size_t j = 0; j < large.size() && rc == ZKHIP_OK; ++j) {
        const int sl = (int)(j % NSLOT);
        if ((rc = finish_slot(sl)) != ZKHIP_OK) break;     // commit j - NSLOT used this region, stream and result slot
        MsmProblems one = {};
        one.n = 1;
        one.off[1] = (uint32_t)large[j].h;
        if (hipStreamWaitEvent(c->side[sl].get(), c->fork_ev.get(), 0) != hipSuccess) { rc = ZKHIP_ERR_HIP; break; }
        c->stream = c->side[sl].get();
        rc = msm_enqueue(c, d_folded_xy + 12 * large[j].off, d_folded_inf + large[j].off, d_q + 4 * large[j].off, large[j].h, one, nullptr, 0,
                         region_off[sl], sl, &pend[sl], nullptr);
        c->stream = main_stream;
        if (rc == ZKHIP_OK) pend_round[sl] = (int)large[j].round;
    }
    // the remaining epilogues, each as soon as its commit's results have landed; every slot is drained even after an error, so that
    // nothing is left running on a side stream
    for (;;) {
        int left = 0, ready = -1;
        for (int k = 0; k < zkhip_ctx::MSM_SLOTS; ++k) {
            if (pend_round[k] < 0) continue;
            ++left;
            if (ready < 0 && hipEventQuery(c->msm_ev[k].get()) != hipErrorNotReady) ready = k;
        }
        if (!left) break;
        if (ready < 0) { std::this_thread::yield(); continue; }
        const int r2 = finish_slot(ready);
        if (rc == ZKHIP_OK) rc = r2;
    }
    if (rc != ZKHIP_OK) {
        for (int k = 0; k < zkhip_ctx::MSM_SLOTS; ++k) hipStreamSynchronize(c->side[k].get());
        return rc;
    }
    // the last remainder is poly(z): `evaluation`, and what the reference checks it against (:84-86)
    ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), cur, 32, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_evaluation, c->pinned_u64(ZK_PIN_RES), 32);
    return ZKHIP_OK;
}

extern "C" int zkhip_kzg_open_tables(zkhip_ctx* c, const uint64_t* d_evals, size_t n, const uint64_t* h_points, size_t n_eval_points,
                                     const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n_points,
                                     const uint64_t* d_folded_xy, const uint8_t* d_folded_inf, const void* d_level_tables_with_header,
                                     uint64_t* h_evaluation, uint64_t* h_proofs_xy, uint8_t* h_proofs_inf) {
    if (!c || !d_evals || !h_points || !d_points_xy || !h_evaluation || !h_proofs_xy || !h_proofs_inf) return ZKHIP_ERR_ARG;
    uint32_t n_vars = 0;
    const void* d_level_tables = nullptr;
    ZK_TRY(kzg_open_check(c, n, n_eval_points, n_points, d_folded_xy, d_folded_inf, d_level_tables_with_header, &n_vars, &d_level_tables));
    return kzg_open_one(c, d_evals, n, n_vars, h_points, d_points_xy, d_points_inf, d_folded_xy, d_folded_inf, d_level_tables, h_evaluation,
                        h_proofs_xy, h_proofs_inf);
}

// ---------------------------------------------------------------------------------------
// MultilinearKZG::open of a BATCH of (polynomial, point) pairs against one SRS
// ---------------------------------------------------------------------------------------
// A small opening (the short path above) is latency: one single-workgroup quotient launch and two launches of a few dozen waves, a copy,
// a synchronisation and a serial host fold, on an empty chip.  Round i of EVERY opening of one SRS commits against the same level table
// with the same widths, so B openings are n_vars table regions read by B scalar vectors each: three launches (quotients, plane sums,
// reduction) with the batch index as a grid dimension, one copy of the terms and the B evaluations, one synchronisation, and the host
// fold of B n_vars problems on the context's host threads.  The group elements are those of the single call, so are the affine proofs.
// A batch is cut into chunks of at most OPEN_BATCH_CHUNK openings: at 2^12 entries a chunk holds 14 MiB of quotients and remainders
// (224 KiB each), <= 3 MiB of terms in device and pinned memory (n_vars x <= 14 planes x 192 B each) and its partial sums -- the buffers
// stay of the size a few dozen single openings' worth, whatever B a caller passes; 64 openings are >= 512 (opening, round) problems
// of <= 14 planes each, several waves for every SIMD of the chip, so a larger chunk has nothing left to fill.
constexpr uint32_t OPEN_BATCH_CHUNK = 64;
static int kzg_open_small_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_eval_ptrs, size_t n, uint32_t n_vars, const uint64_t* h_points,
                                const uint8_t* d_folded_inf, const uint32_t* d_level_tables, uint64_t* h_evaluations, uint64_t* h_proofs_xy,
                                uint8_t* h_proofs_inf, uint32_t chunk_max) {
    if (n_vars > (uint32_t)MSM_SMALL_PROBS || chunk_max == 0) return ZKHIP_ERR_SHAPE;
    const uint32_t bc_max = std::min(batch, chunk_max);
    // the rounds, once for the whole batch: round j commits n >> (j + 1) quotients against level j as zkhip_srs_level_tables laid it out;
    // the slots are dealt over the WHOLE chunk (msm_small_plan.hpp)
    MsmSmallProblem sp[MSM_SMALL_PROBS];
    size_t entry = 0, lvl_off = 0;
    for (uint32_t j = 0; j < n_vars; ++j) {
        const size_t h = n >> (j + 1);
        sp[j] = {h, h, entry, lvl_off, msm_level_table_widths(h, n - 1)};
        entry += (size_t)sp[j].lw.W * h;
        lvl_off += h;
    }
    const MsmSmallGeometry g = msm_small_plan(sp, n_vars, bc_max);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // staging (pinned -> aux): the chunk's table pointers, then its points
    const size_t o_pts = al((size_t)bc_max * 8), stage_bytes = o_pts + al((size_t)bc_max * n_vars * 32);
    const size_t q_stride = n, ping_stride = n / 2, pong_stride = n / 4;             // scalars per opening
    const size_t o_q = stage_bytes, o_ping = o_q + al(bc_max * q_stride * 32), o_pong = o_ping + al(bc_max * ping_stride * 32);
    ZK_TRY(c->reserve_aux(o_pong + al(bc_max * pong_stride * 32)));
    const size_t out_bytes = al(g.terms_bytes(bc_max) + (size_t)bc_max * 32);    // terms | evaluations: ONE copy
    const MsmSmallCarve cv = msm_small_carve(g.part_bytes(bc_max), out_bytes);
    ZK_TRY(c->reserve_ws(cv.ws_bytes));
    ZK_TRY(c->reserve_msm_pin(0, out_bytes + stage_bytes));
    char* aux = (char*)c->aux.ptr;
    char* pin = (char*)c->msm_pin[0].ptr;
    const MsmSmallArgs a = msm_small_args(g, d_level_tables, d_folded_inf, (const uint64_t*)(aux + o_q), c->ws.ptr, (char*)c->ws.ptr + cv.terms_off);
    for (uint32_t b0 = 0; b0 < batch; b0 += bc_max) {
        const uint32_t bc = std::min(bc_max, batch - b0);
        const size_t terms_bytes = g.terms_bytes(bc);
        uint64_t* d_evals_out = a.terms + terms_bytes / 8;
        // (the previous chunk's upload has ended: every chunk ends in a synchronisation)
        std::memcpy(pin + out_bytes, h_eval_ptrs + b0, (size_t)bc * 8);
        std::memcpy(pin + out_bytes + o_pts, h_points + 4 * (size_t)n_vars * b0, (size_t)bc * n_vars * 32);
        ZK_HIP(c, hipMemcpyAsync(aux, pin + out_bytes, o_pts + (size_t)bc * n_vars * 32, hipMemcpyHostToDevice, c->stream));
        {
            ProfScope ps(c, "open_batch_steps", 96.0 * (double)n * bc);
            hipLaunchKernelGGL(open_steps_small_batch_kernel, dim3(bc), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t* const*)aux, (uint32_t)n,
                               (const uint64_t*)(aux + o_pts), n_vars, (uint64_t*)(aux + o_q), q_stride, (uint64_t*)(aux + o_ping), ping_stride,
                               (uint64_t*)(aux + o_pong), pong_stride, d_evals_out);
        }
        {
            ProfScope ps(c, "open_batch_planes", 128.0 * (double)g.total_pairs * bc);
            hipLaunchKernelGGL(msm_small_batch_planes_kernel, dim3(a.total_slots, a.planes, bc), dim3(64), 0, c->stream, a, q_stride);
        }
        {
            ProfScope ps(c, "open_batch_reduce", 0.0);
            hipLaunchKernelGGL(msm_small_batch_reduce_kernel, dim3(a.planes, n_vars, bc), dim3(64), 0, c->stream, a);
        }
        ZK_TRY(msm_small_fetch(c, a.terms, terms_bytes + (size_t)bc * 32));
        // the host fold per (opening, round); with the profile on, events on the now idle stream bracket it: their distance is the host time
        ProfScope ps(c, "open_batch_fold", 0.0);
        msm_small_finish(c, g, bc * n_vars, h_proofs_xy, h_proofs_inf, [&](uint32_t k) { return (size_t)b0 * n_vars + k; });
        std::memcpy(h_evaluations + 4 * (size_t)b0, pin + terms_bytes, (size_t)bc * 32);
    }
    return ZKHIP_OK;
}
// The commits of one round of a CHUNK of PLONK proofs (zkhip_plonk_prove_batch, ctx.hpp): m <= 3 polynomials per proof, polynomial j of
// proof b being lens[j] scalars from d_scalars + 4 (b q_stride + sc_off[j]) on, all against the one shifted-SRS table.  ONE launch of the
// plane sums with the proof as grid.z, one of the reduce, one copy, one synchronisation -- which also completes whatever the caller
// enqueued before -- and the host folds on the context's pool.  Result (b, j) goes to h_out_xy + 12 (b out_stride + j),
// h_out_inf[b out_stride + j].  The group elements are those of any other commit path, so are the affine points.
bool zk_msm_commit_batch_serves(size_t n_points, size_t longest) {
    return msm_small_on() && longest <= MSM_SMALL_MAX && n_points * msm_table_widths(n_points).W < ((size_t)1 << 31);
}
int zk_msm_commit_batch(zkhip_ctx* c, const void* d_table_with_header, const uint8_t* d_points_inf, size_t n_points, const uint64_t* d_scalars,
                        size_t q_stride, uint32_t batch, uint32_t m, const size_t* sc_off, const size_t* lens, uint64_t* h_out_xy,
                        uint8_t* h_out_inf, size_t out_stride) {
    if (!c || !d_table_with_header || !d_scalars || !sc_off || !lens || !h_out_xy || !h_out_inf) return ZKHIP_ERR_ARG;
    if (m == 0 || m > 3 || batch == 0 || batch > 65535) return ZKHIP_ERR_SHAPE;
    size_t longest = 0;
    for (uint32_t j = 0; j < m; ++j) {
        longest = std::max(longest, lens[j]);
        if (lens[j] == 0 || sc_off[j] + lens[j] > q_stride || q_stride >= ((size_t)1 << 32)) return ZKHIP_ERR_SHAPE;
    }
    if (longest > n_points) return ZKHIP_ERR_INDEX;
    if (!zk_msm_commit_batch_serves(n_points, longest)) return ZKHIP_ERR_SHAPE;
    int trc = ZKHIP_OK;
    const uint32_t* d_table = table_check(c, d_table_with_header, ZK_TABLE_SHIFTED_SRS, n_points, &trc);
    if (!d_table) return trc;
    const MsmLevelWidths lw = msm_table_widths(n_points);
    MsmSmallProblem sp[3];
    for (uint32_t j = 0; j < m; ++j) sp[j] = {lens[j], n_points, 0, sc_off[j], lw};
    const MsmSmallGeometry g = msm_small_plan(sp, m, batch);            // the slots: dealt over the whole chunk of proofs
    const size_t terms_bytes = g.terms_bytes(batch);
    const MsmSmallCarve cv = msm_small_carve(g.part_bytes(batch), terms_bytes);
    ZK_TRY(c->reserve_ws(cv.ws_bytes));
    ZK_TRY(c->reserve_msm_pin(0, terms_bytes));
    const MsmSmallArgs a = msm_small_args(g, d_table, d_points_inf, d_scalars, c->ws.ptr, (char*)c->ws.ptr + cv.terms_off);
    {
        ProfScope ps(c, "plonk_batch_commit_planes", 128.0 * (double)g.total_pairs * batch / std::max<uint32_t>(1, lw.W));
        hipLaunchKernelGGL(msm_small_commit_batch_planes_kernel, dim3(a.total_slots, a.planes, batch), dim3(64), 0, c->stream, a, q_stride);
    }
    {
        ProfScope ps(c, "plonk_batch_commit_reduce", 0.0);
        hipLaunchKernelGGL(msm_small_batch_reduce_kernel, dim3(a.planes, m, batch), dim3(64), 0, c->stream, a);
    }
    ZK_TRY(msm_small_fetch(c, a.terms, terms_bytes));
    msm_small_finish(c, g, batch * m, h_out_xy, h_out_inf, [&](uint32_t k) { return (size_t)(k / m) * out_stride + k % m; });      // k = b m + j
    return ZKHIP_OK;
}

// ---------------------------------------------------------------------------------------
// zkhip_kzg_commit_polys: a BATCH of polynomials against one SRS
// ---------------------------------------------------------------------------------------
// A lone commit of 2^13 .. 2^16 scalars is ~1 ms of latency on a mostly idle chip -- seventeen launches, reduction passes that are chains
// of point additions, a host epilogue --, whatever the chip could do beside.  B polynomials against ONE SRS share all of it: their
// (point, window) pairs fill ONE pass of every kernel of the bucket pipeline (the geometry mode "one set of points": every problem its
// own windows and bucket sets, the point base in the windows' entry_off, the scalars read in place through a pointer table), and their
// host epilogues run side by side on the context's pool.  What serves a batch, and how it is cut into chunks, is decided by
// commit_polys_plan.hpp; the routes are below.  Every route delivers the group elements of the single commits, so their affine points.
static_assert(CPP_SMALL_MAX == MSM_SMALL_MAX, "commit_polys_plan.hpp routes by the short path's limit");
static int commit_polys_plan(size_t n_points, const size_t* len, uint32_t batch, bool table, std::shared_ptr<const CppPlan>* out) {
    // the plans of the last few shapes (a plan builds its chunks' geometries: ~0.1 ms of host time per distinct chunk shape)
    struct Entry { size_t n_points; bool table; std::vector<size_t> len; std::shared_ptr<const CppPlan> plan; };
    static std::mutex mu;
    static std::vector<Entry> cache;
    std::lock_guard<std::mutex> lk(mu);
    for (const Entry& e : cache)
        if (e.n_points == n_points && e.table == table && e.len.size() == batch && std::equal(e.len.begin(), e.len.end(), len)) {
            *out = e.plan;
            return e.plan->status;
        }
    auto p = std::make_shared<CppPlan>(cpp_plan(n_points, len, batch, table, msm_small_on()));
    if (cache.size() >= 4) cache.erase(cache.begin());
    cache.push_back({n_points, table, std::vector<size_t>(len, len + batch), p});
    *out = p;
    return p->status;
}
// one polynomial on the single call's path, behind its checks (d_table: behind the checked header)
static int commit_polys_one(zkhip_ctx* c, const uint64_t* d_points_xy, const uint32_t* d_table, const uint8_t* d_points_inf, size_t n_points,
                            const uint64_t* d_scalars, size_t n, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    if (!d_table) return msm_commit(c, d_points_xy, d_points_inf, d_scalars, n, h_out_xy, h_out_inf);
    if (msm_small_on() && n <= MSM_SMALL_MAX) return msm_commit_small(c, d_table, n_points, d_points_inf, d_scalars, n, h_out_xy, h_out_inf);
    MsmProblems one = {};
    one.n = 1;
    one.off[1] = (uint32_t)n;
    return msm_commit_multi(c, nullptr, d_points_inf, d_scalars, n, one, h_out_xy, h_out_inf, d_table, n_points);
}
// SHORT route: a chunk's polynomials in the order of their lengths; every run of one length (a CLASS) is one launch of the plane sums
// with the polynomial as grid.z and one of the reduce, all classes of the chunk in front of ONE copy and ONE synchronisation; then the
// weighted sums on the pool (zk_msm_commit_batch does the same for PLONK's fixed-stride layout).
// ptrs / len / where: the non-empty polynomials, their lengths and their places in the outputs.
static int commit_polys_short(zkhip_ctx* c, const uint32_t* d_table, const uint8_t* d_points_inf, size_t n_points, const CppPlan& plan,
                              const uint64_t* const* ptrs, const size_t* len, const uint32_t* where, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    const MsmLevelWidths lw = msm_table_widths(n_points);
    for (const CppChunk& ch : plan.chunks) {
        static_assert(CPP_SMALL_CHUNK <= (uint32_t)MSM_MAX_PROBLEMS, "a chunk's pointers are one MsmPtrTable");
        uint32_t order[CPP_SMALL_CHUNK];
        for (uint32_t k = 0; k < ch.count; ++k) order[k] = ch.first + k;
        std::stable_sort(order, order + ch.count, [&](uint32_t x, uint32_t y) { return len[x] < len[y]; });
        MsmPtrTable pt = {};
        for (uint32_t k = 0; k < ch.count; ++k) pt.p[k] = ptrs[order[k]];
        struct Class { uint32_t first, count; size_t part_off; MsmSmallGeometry g; };
        std::vector<Class> classes;
        size_t part_bytes = 0;
        for (uint32_t k = 0; k < ch.count;) {
            uint32_t e = k + 1;
            while (e < ch.count && len[order[e]] == len[order[k]]) ++e;
            const MsmSmallProblem one = {len[order[k]], n_points, 0, 0, lw};
            classes.push_back({k, e - k, part_bytes, msm_small_plan(&one, 1, ch.count)});      // the slots: dealt over the whole chunk
            part_bytes += classes.back().g.part_bytes(e - k);
            k = e;
        }
        const size_t terms_bytes = (size_t)ch.count * lw.hi * 192;
        const MsmSmallCarve cv = msm_small_carve(part_bytes, terms_bytes);
        ZK_TRY(c->reserve_ws(cv.ws_bytes));
        ZK_TRY(c->reserve_msm_pin(0, terms_bytes));
        uint64_t* d_terms = (uint64_t*)((char*)c->ws.ptr + cv.terms_off);
        for (const Class& cl : classes) {
            const MsmSmallArgs a = msm_small_args(cl.g, d_table, d_points_inf, nullptr, (char*)c->ws.ptr + cl.part_off, d_terms + 24 * (size_t)cl.first * lw.hi);
            {
                ProfScope ps(c, "commit_polys_planes", 128.0 * (double)a.n[0] * cl.count);
                hipLaunchKernelGGL(msm_small_commit_polys_planes_kernel, dim3(a.total_slots, lw.hi, cl.count), dim3(64), 0, c->stream, a, pt, cl.first);
            }
            {
                ProfScope ps(c, "commit_polys_reduce", 0.0);
                hipLaunchKernelGGL(msm_small_batch_reduce_kernel, dim3(lw.hi, 1, cl.count), dim3(64), 0, c->stream, a);
            }
        }
        ZK_TRY(msm_small_fetch(c, d_terms, terms_bytes));
        // (every class has one problem of lw.hi planes: any of their geometries describes the chunk's terms)
        msm_small_finish(c, classes[0].g, ch.count, h_out_xy, h_out_inf, [&](uint32_t k) { return (size_t)where[order[k]]; });
    }
    return ZKHIP_OK;
}
// BUCKET route: chunk after chunk as one pass of the bucket pipeline each, all on the caller's stream, TWO in flight -- a region of the
// workspace, a result slot and a device copy of the geometry tables each -- so that the host epilogues of a chunk (one weighted sum per
// problem, on the pool) run beside the passes of the next.
static int commit_polys_bucket(zkhip_ctx* c, const uint64_t* d_points_xy, const uint32_t* d_table, const uint8_t* d_points_inf, size_t n_points,
                               const CppPlan& plan, const uint64_t* const* ptrs, const uint32_t* where, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    size_t region = 0;
    for (const CppChunk& ch : plan.chunks) region = std::max(region, (ch.ws_bytes + 4095) & ~(size_t)4095);
    const size_t n_chunks = plan.chunks.size();
    ZK_TRY(c->reserve_ws(region * std::min<size_t>(2, n_chunks)));      // once, up front: growing it later would move it under the chunk in flight
    MsmPending pend[2];
    int pend_chunk[2] = {-1, -1};
    uint64_t xy[12 * MSM_MAX_PROBLEMS];
    uint8_t inf[MSM_MAX_PROBLEMS];
    auto finish_slot = [&](int sl) -> int {
        if (pend_chunk[sl] < 0) return ZKHIP_OK;
        const CppChunk& ch = plan.chunks[pend_chunk[sl]];
        pend_chunk[sl] = -1;
        ZK_TRY(msm_finish(c, pend[sl], xy, inf));
        for (uint32_t j = 0; j < ch.count; ++j) {                        // (empty polynomials may lie between a chunk's: the outputs are not one run)
            const size_t o = where[ch.first + j];
            std::memcpy(h_out_xy + 12 * o, xy + 12 * j, 96);
            h_out_inf[o] = inf[j];
        }
        return ZKHIP_OK;
    };
    int rc = ZKHIP_OK;
    for (size_t k = 0; k < n_chunks && rc == ZKHIP_OK; ++k) {
        const CppChunk& ch = plan.chunks[k];
        const int sl = (int)(k & 1);
        if ((rc = finish_slot(sl)) != ZKHIP_OK) break;                   // chunk k - 2 used this region, result slot and table copy
        MsmPolys polys = {};
        for (uint32_t j = 0; j < ch.count; ++j) polys.ptrs.p[j] = ptrs[ch.first + j];
        polys.n_conv = ch.n_conv;
        polys.geo = ch.geo;
        size_t used = 0;
        rc = msm_enqueue(c, nullptr, nullptr, nullptr, ch.n_total, ch.pr, d_table, n_points, 0, 0, nullptr, &used, &polys);
        if (rc == ZKHIP_OK && used > region) rc = ZKHIP_ERR_SHAPE;       // (the planner's carve-up is msm_enqueue's: never)
        if (rc == ZKHIP_OK)
            rc = msm_enqueue(c, d_points_xy, d_points_inf, nullptr, ch.n_total, ch.pr, d_table, n_points, (size_t)sl * region, sl, &pend[sl], nullptr, &polys);
        if (rc == ZKHIP_OK) pend_chunk[sl] = (int)k;
    }
    // the chunks still in flight, the older first; both are drained even after an error
    for (int q = 0; q < 2; ++q) {
        const int sl = (int)((n_chunks + q) & 1);
        const int r2 = finish_slot(sl);
        if (rc == ZKHIP_OK) rc = r2;
    }
    if (rc != ZKHIP_OK) hipStreamSynchronize(c->stream);
    return rc;
}
// SINGLE route: the shapes a batched route does not serve faster (commit_polys_plan.hpp) run as the single commits a caller could issue
// himself, the way that serves him best -- the short commits against a table one after another (zkhip_kzg_commit_table's short path:
// a commit in flight always takes the bucket pipeline), everything else three in flight (zkhip_kzg_commit_begin / _end), which takes
// and returns the workspace loan inside the call.  One polynomial is the single call's path.
static int commit_polys_single(zkhip_ctx* c, const uint64_t* d_points_xy, const void* d_table_with_header, const uint32_t* d_table,
                               const uint8_t* d_points_inf, size_t n_points, uint32_t m, const uint64_t* const* ptrs, const size_t* len,
                               const uint32_t* where, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    std::vector<uint32_t> rest;
    for (uint32_t k = 0; k < m; ++k) {
        if (m > 1 && !(d_table && msm_small_on() && len[k] <= MSM_SMALL_MAX)) { rest.push_back(k); continue; }
        ZK_TRY(commit_polys_one(c, d_points_xy, d_table, d_points_inf, n_points, ptrs[k], len[k], h_out_xy + 12 * (size_t)where[k], h_out_inf + where[k]));
    }
    if (rest.size() == 1) {
        const uint32_t k = rest[0];
        return commit_polys_one(c, d_points_xy, d_table, d_points_inf, n_points, ptrs[k], len[k], h_out_xy + 12 * (size_t)where[k], h_out_inf + where[k]);
    }
    struct InFlight { uint32_t k, ticket; };
    InFlight pend[zkhip_ctx::ASYNC_SLOTS];
    int n_pend = 0, rc = ZKHIP_OK;
    auto end_oldest = [&](bool deliver) -> int {
        const InFlight f = pend[0];
        for (int q = 1; q < n_pend; ++q) pend[q - 1] = pend[q];
        --n_pend;
        return zkhip_kzg_commit_end(c, f.ticket, deliver ? h_out_xy + 12 * (size_t)where[f.k] : nullptr, deliver ? h_out_inf + where[f.k] : nullptr);
    };
    for (size_t q = 0; q < rest.size() && rc == ZKHIP_OK; ++q) {
        const uint32_t k = rest[q];
        uint32_t ticket = 0;
        for (;;) {
            if (n_pend == zkhip_ctx::ASYNC_SLOTS && (rc = end_oldest(true)) != ZKHIP_OK) break;
            rc = zkhip_kzg_commit_begin(c, d_points_xy, d_table_with_header, d_points_inf, n_points, ptrs[k], len[k], 0, &ticket);
            if (rc != ZKHIP_ERR_BUSY || n_pend == 0) break;
            if ((rc = end_oldest(true)) != ZKHIP_OK) break;              // a larger commit than the ones in flight: those end first
        }
        if (rc == ZKHIP_OK) pend[n_pend++] = InFlight{k, ticket};
    }
    while (n_pend) {                                                     // the rest; after an error they are drained, not delivered
        const int r2 = end_oldest(rc == ZKHIP_OK);
        if (rc == ZKHIP_OK) rc = r2;
    }
    return rc;
}
// the checks on the lengths, shared by the call and its diagnostic
static int commit_polys_check_lengths(size_t n_points, const size_t* h_n_scalars, uint32_t batch, int require_equal_len) {
    if (require_equal_len) {
        for (uint32_t b = 0; b < batch; ++b) if (h_n_scalars[b] != n_points) return ZKHIP_ERR_SHAPE;     // multilinear_kzg.rs:36-41
    }
    for (uint32_t b = 0; b < batch; ++b) if (h_n_scalars[b] > n_points) return ZKHIP_ERR_INDEX;         // univariate_kzg.rs:53
    return ZKHIP_OK;
}
// The call behind its argument checks, in two steps that zkhip_univariate_kzg_open_batch shares (its quotients are the polynomials):
// ADMIT -- the plan of the m >= 1 non-empty polynomials, the refusal beside a lent workspace, the table's header; nothing is launched,
// reserved or written -- and the ROUTES, which deliver polynomial k at where[k] of the outputs.
static int commit_polys_admit(zkhip_ctx* c, const void* d_table_with_header, size_t n_points, const size_t* len, uint32_t m,
                              std::shared_ptr<const CppPlan>* plan, const uint32_t** d_table) {
    ZK_TRY(commit_polys_plan(n_points, len, m, d_table_with_header != nullptr, plan));
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;
    ZK_TRY(c->activate());
    *d_table = nullptr;
    if (d_table_with_header) {
        int trc = ZKHIP_OK;
        *d_table = table_check(c, d_table_with_header, ZK_TABLE_SHIFTED_SRS, n_points, &trc);       // built for THESE n_points, with the widths used below?
        if (!*d_table) return trc;
    }
    return ZKHIP_OK;
}
static int commit_polys_routes(zkhip_ctx* c, const uint64_t* d_points_xy, const void* d_table_with_header, const uint32_t* d_table,
                               const uint8_t* d_points_inf, size_t n_points, const CppPlan& plan, uint32_t m, const uint64_t* const* ptrs,
                               const size_t* len, const uint32_t* where, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    if (plan.route == CPP_SHORT) return commit_polys_short(c, d_table, d_points_inf, n_points, plan, ptrs, len, where, h_out_xy, h_out_inf);
    if (plan.route == CPP_BUCKET) return commit_polys_bucket(c, d_points_xy, d_table, d_points_inf, n_points, plan, ptrs, where, h_out_xy, h_out_inf);
    return commit_polys_single(c, d_points_xy, d_table_with_header, d_table, d_points_inf, n_points, m, ptrs, len, where, h_out_xy, h_out_inf);
}
extern "C" int zkhip_kzg_commit_polys(zkhip_ctx* c, const uint64_t* d_points_xy, const void* d_table_with_header, const uint8_t* d_points_inf,
                                      size_t n_points, uint32_t batch, const uint64_t* const* h_scalar_ptrs, const size_t* h_n_scalars,
                                      int require_equal_len, uint64_t* h_out_xy, uint8_t* h_out_inf) {
    if (!c) return ZKHIP_ERR_ARG;
    if (batch == 0) return ZKHIP_OK;
    if (!h_scalar_ptrs || !h_n_scalars || !h_out_xy || !h_out_inf || (!d_points_xy == !d_table_with_header)) return ZKHIP_ERR_ARG;
    ZK_TRY(commit_polys_check_lengths(n_points, h_n_scalars, batch, require_equal_len));
    // the non-empty polynomials and their places in the outputs
    std::vector<const uint64_t*> ptrs;
    std::vector<size_t> len;
    std::vector<uint32_t> where;
    for (uint32_t b = 0; b < batch; ++b) {
        if (h_n_scalars[b] == 0) continue;
        if (!h_scalar_ptrs[b]) return ZKHIP_ERR_ARG;
        ptrs.push_back(h_scalar_ptrs[b]); len.push_back(h_n_scalars[b]); where.push_back(b);
    }
    const uint32_t m = (uint32_t)ptrs.size();
    const uint32_t* d_table = nullptr;
    std::shared_ptr<const CppPlan> plan;
    if (m) ZK_TRY(commit_polys_admit(c, d_table_with_header, n_points, len.data(), m, &plan, &d_table));
    for (uint32_t b = 0; b < batch; ++b)
        if (h_n_scalars[b] == 0) { std::memset(h_out_xy + 12 * (size_t)b, 0, 96); h_out_inf[b] = 1; }       // P::G1::default()
    if (!m) return ZKHIP_OK;
    return commit_polys_routes(c, d_points_xy, d_table_with_header, d_table, d_points_inf, n_points, *plan, m, ptrs.data(), len.data(), where.data(),
                               h_out_xy, h_out_inf);
}
extern "C" int zkhip_commit_polys_plan_info(size_t n_points, const size_t* h_n_scalars, uint32_t batch, int with_table, uint32_t* h_route,
                                            uint32_t* h_n_chunks, uint32_t* h_chunk_counts, size_t* h_chunk_ws) {
    if (!h_n_scalars || !h_route || !h_n_chunks) return ZKHIP_ERR_ARG;
    ZK_TRY(commit_polys_check_lengths(n_points, h_n_scalars, batch, 0));
    std::vector<size_t> len;
    for (uint32_t b = 0; b < batch; ++b) if (h_n_scalars[b]) len.push_back(h_n_scalars[b]);
    const CppPlan plan = cpp_plan(n_points, len.data(), (uint32_t)len.size(), with_table != 0, msm_small_on());
    ZK_TRY(plan.status);
    *h_route = (uint32_t)plan.route;
    *h_n_chunks = (uint32_t)plan.chunks.size();
    for (size_t k = 0; k < plan.chunks.size(); ++k) {
        if (h_chunk_counts) h_chunk_counts[k] = plan.chunks[k].count;
        if (h_chunk_ws) h_chunk_ws[k] = plan.chunks[k].ws_bytes;
    }
    return ZKHIP_OK;
}

static int kzg_open_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_eval_ptrs, size_t n, const uint64_t* h_points, size_t n_eval_points,
                          const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n_points, const uint64_t* d_folded_xy,
                          const uint8_t* d_folded_inf, const void* d_level_tables_with_header, uint64_t* h_evaluations, uint64_t* h_proofs_xy,
                          uint8_t* h_proofs_inf, uint32_t chunk_max) {
    if (!c) return ZKHIP_ERR_ARG;
    if (batch == 0) return ZKHIP_OK;
    if (!h_eval_ptrs || !h_points || !d_points_xy || !h_evaluations || !h_proofs_xy || !h_proofs_inf) return ZKHIP_ERR_ARG;
    for (uint32_t b = 0; b < batch; ++b) if (!h_eval_ptrs[b]) return ZKHIP_ERR_ARG;
    uint32_t n_vars = 0;
    const void* d_level_tables = nullptr;
    ZK_TRY(kzg_open_check(c, n, n_eval_points, n_points, d_folded_xy, d_folded_inf, d_level_tables_with_header, &n_vars, &d_level_tables));
    if (d_level_tables && n <= MSM_SMALL_MAX && !open_pipelines_on() && msm_small_on())
        return kzg_open_small_batch(c, batch, h_eval_ptrs, n, n_vars, h_points, d_folded_inf, (const uint32_t*)d_level_tables, h_evaluations,
                                    h_proofs_xy, h_proofs_inf, chunk_max);
    // every other size and configuration: one after another through the single opening (several openings in ONE bucket-pipeline commit
    // need a point base per problem in msm_enqueue's sort keys: zkhip_kzg_commit_polys has it now; the openings do not go through it yet)
    for (uint32_t b = 0; b < batch; ++b)
        ZK_TRY(kzg_open_one(c, h_eval_ptrs[b], n, n_vars, h_points + 4 * (size_t)n_vars * b, d_points_xy, d_points_inf, d_folded_xy, d_folded_inf,
                            d_level_tables, h_evaluations + 4 * (size_t)b, h_proofs_xy + 12 * (size_t)n_vars * b, h_proofs_inf + (size_t)n_vars * b));
    return ZKHIP_OK;
}
extern "C" int zkhip_kzg_open_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_eval_ptrs, size_t n, const uint64_t* h_points,
                                    size_t n_eval_points, const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n_points,
                                    const uint64_t* d_folded_xy, const uint8_t* d_folded_inf, const void* d_level_tables_with_header,
                                    uint64_t* h_evaluations, uint64_t* h_proofs_xy, uint8_t* h_proofs_inf) {
    return kzg_open_batch(c, batch, h_eval_ptrs, n, h_points, n_eval_points, d_points_xy, d_points_inf, n_points, d_folded_xy, d_folded_inf,
                          d_level_tables_with_header, h_evaluations, h_proofs_xy, h_proofs_inf, OPEN_BATCH_CHUNK);
}

// ---------------------------------------------------------------------------------------
// UnivariateKZG::open
// ---------------------------------------------------------------------------------------
extern "C" int zkhip_univariate_kzg_open(zkhip_ctx* c, const uint64_t* d_coeffs, size_t n, const uint64_t* h_z,
                                         const uint64_t* d_points_xy, const uint8_t* d_points_inf, size_t n_points,
                                         uint64_t* h_evaluation, uint64_t* h_proof_xy, uint8_t* h_proof_inf) {
    if (!c || !h_z || !h_evaluation || !h_proof_xy || !h_proof_inf || (n && !d_coeffs)) return ZKHIP_ERR_ARG;
    if (n == 0) {                                   // the zero polynomial: evaluate() = 0; numerator [z] has degree 0 < 1 -> quotient zero
        std::memset(h_proof_xy, 0, 96);
        std::memset(h_evaluation, 0, 32);
        *h_proof_inf = 1;
        return ZKHIP_OK;
    }
    if (n - 1 > n_points) return ZKHIP_ERR_INDEX;  // srs.powers_of_tau_in_g1[i] out of bounds (univariate_kzg.rs:75)
    if (n >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;
    if (n > 1 && !d_points_xy) return ZKHIP_ERR_ARG;
    // the quotient's commit needs the workspace: refused before the scan is launched and before an output is written (the evaluation
    // used to be delivered, and the proof cleared, in front of the commit's ZKHIP_ERR_BUSY)
    if (n > 1 && c->ws_loans.lent()) return ZKHIP_ERR_BUSY;
    std::memset(h_proof_xy, 0, 96);
    ZK_TRY(c->activate());
    const size_t per_block = (size_t)HS_T * HS_L;
    const uint32_t n_blocks = (uint32_t)((n + per_block - 1) / per_block);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_q = 0, o_vals = al(32 * n), o_carry = o_vals + al(32 * (size_t)n_blocks), o_eval = o_carry + al(32 * (size_t)n_blocks);
    ZK_TRY(c->reserve_aux(o_eval + 256));
    char* aux = (char*)c->aux.ptr;
    uint64_t* d_q = (uint64_t*)(aux + o_q);
    uint64_t* d_vals = (uint64_t*)(aux + o_vals);
    uint64_t* d_carry = (uint64_t*)(aux + o_carry);
    uint64_t* d_eval = (uint64_t*)(aux + o_eval);
    FrArg z = {};
    std::memcpy(z.v, h_z, 32);
    {
        ProfScope ps(c, "horner_scan", 96.0 * (double)n);
        hipLaunchKernelGGL(horner_scan_kernel<false>, dim3(n_blocks), dim3(HS_T), 0, c->stream, d_coeffs, n, z, d_vals, nullptr, nullptr, nullptr);
        hipLaunchKernelGGL(horner_top_kernel, dim3(1), dim3(1024), 0, c->stream, d_vals, n_blocks, z, d_carry, (uint64_t*)nullptr);
        hipLaunchKernelGGL(horner_scan_kernel<true>, dim3(n_blocks), dim3(HS_T), 0, c->stream, d_coeffs, n, z, nullptr, d_carry, d_q, d_eval);
    }
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_eval, 32, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_evaluation, c->pinned_u64(ZK_PIN_RES), 32);
    if (n == 1) { *h_proof_inf = 1; return ZKHIP_OK; }          // degree 0 < 1: quotient zero, proof = G1::default()
    return msm_commit(c, d_points_xy, d_points_inf, d_q, n - 1, h_proof_xy, h_proof_inf);
}

// ---------------------------------------------------------------------------------------
// zkhip_univariate_kzg_open_batch: a BATCH of openings against one SRS
// ---------------------------------------------------------------------------------------
// A lone opening is three scan launches, a synchronisation for the evaluation and a whole commit of the quotient -- the bucket pipeline's
// ~0.7 ms of latency even for 2^8 coefficients.  A batch shares both halves: the scans of a chunk of jobs run as one launch (short jobs)
// or three (long jobs) over a job table in device memory (horner_jobs_kernels.hpp), and the chunk's quotients are the polynomials of
// zkhip_kzg_commit_polys's routes, read in place.  univariate_open_plan.hpp cuts the batch into chunks and bounds a chunk's scratch.
//
// WHERE THE QUOTIENTS LIVE.  In the `aux` arena, like the single call's quotient across msm_commit, reserved ONCE for the largest chunk
// before the first launch.  That is safe because no route of the commit touches that arena: commit_polys_short, commit_polys_bucket and
// msm_enqueue carve the WORKSPACE (reserve_ws) and the pinned result slots (reserve_msm_pin); commit_polys_single goes through
// msm_commit / msm_commit_small / zkhip_kzg_commit_begin, which reserve the workspace and side streams; reserve_aux is called by the
// multilinear openings (kzg_open_one, kzg_open_small_batch), by this call and its single form, and by zkhip_dense_evaluate only -- none
// of them runs inside a commit.  The commits in flight of the single route read the quotients from side streams that wait for an event
// recorded on the caller's stream behind the scans, and are ended before the route returns, so the next chunk's scans overwrite nothing
// that is still read.
static_assert(UOP_BLOCK == (size_t)HS_T * HS_L, "univariate_open_plan.hpp classes a job by the scan's workgroup");
// No shape runs as a loop of the single call (the rule and its measurements: univariate_open_plan.hpp): the scans of a chunk are never
// more launches than one opening's, and where commit_polys_plan.hpp finds no shared pass worth it, its own single route (three commits in
// flight) already is the loop, minus a synchronisation per opening.
extern "C" int zkhip_univariate_kzg_open_batch(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_coeff_ptrs, const size_t* h_n_coeffs,
                                               const uint64_t* h_z, const uint64_t* d_points_xy, const void* d_table_with_header,
                                               const uint8_t* d_points_inf, size_t n_points, uint64_t* h_evaluations, uint64_t* h_proofs_xy,
                                               uint8_t* h_proofs_inf) {
    if (!c) return ZKHIP_ERR_ARG;
    if (batch == 0) return ZKHIP_OK;
    if (!h_coeff_ptrs || !h_n_coeffs || !h_z || !h_evaluations || !h_proofs_xy || !h_proofs_inf) return ZKHIP_ERR_ARG;
    bool any_quotient = false;
    for (uint32_t b = 0; b < batch; ++b) {
        if (h_n_coeffs[b] && !h_coeff_ptrs[b]) return ZKHIP_ERR_ARG;
        any_quotient = any_quotient || h_n_coeffs[b] > 1;
    }
    const UopPlan plan = uop_plan(n_points, h_n_coeffs, batch);                 // ZKHIP_ERR_INDEX, ZKHIP_ERR_SHAPE: the single call's
    ZK_TRY(plan.status);
    const bool table = d_table_with_header != nullptr;
    if (any_quotient && (!d_points_xy == !d_table_with_header)) return ZKHIP_ERR_ARG;
    if (any_quotient && table && n_points * msm_table_widths(n_points).W >= ((size_t)1 << 31)) return ZKHIP_ERR_SHAPE;   // (as the commit against a table)
    if (any_quotient && c->ws_loans.lent()) return ZKHIP_ERR_BUSY;              // the quotients' commits need the workspace
    if (batch == 1 && (d_points_xy || !any_quotient))                           // one opening: the single call's path
        return zkhip_univariate_kzg_open(c, h_coeff_ptrs[0], h_n_coeffs[0], h_z, d_points_xy, d_points_inf, n_points, h_evaluations, h_proofs_xy, h_proofs_inf);
    ZK_TRY(c->activate());
    const uint32_t* d_table = nullptr;
    if (any_quotient && table) {
        int trc = ZKHIP_OK;
        d_table = table_check(c, d_table_with_header, ZK_TABLE_SHIFTED_SRS, n_points, &trc);
        if (!d_table) return trc;
    }
    // the arena: [ job table | evaluations | the chunk's scratch ], for the largest chunk, once
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    uint32_t max_jobs = 0;
    for (const UopChunk& ch : plan.chunks) max_jobs = std::max(max_jobs, ch.count);
    const size_t o_evals = al(sizeof(HornerJobsHead) + (size_t)max_jobs * (sizeof(HornerJob) + 4)), o_scratch = o_evals + al(32 * (size_t)max_jobs);
    if (!plan.chunks.empty()) ZK_TRY(c->reserve_aux(o_scratch + plan.scratch_max + 256));
    // the openings that need no device: the zero polynomial (evaluation 0, the identity)
    for (uint32_t b = 0; b < batch; ++b)
        if (h_n_coeffs[b] == 0) {
            std::memset(h_evaluations + 4 * (size_t)b, 0, 32);
            std::memset(h_proofs_xy + 12 * (size_t)b, 0, 96);
            h_proofs_inf[b] = 1;
        }
    std::vector<char> h_table;
    std::vector<uint64_t> h_ev;
    std::vector<const uint64_t*> q_ptrs;
    std::vector<size_t> q_len;
    std::vector<uint32_t> q_where;
    for (const UopChunk& ch : plan.chunks) {
        char* const aux = (char*)c->aux.ptr;
        const HornerJobsHead* d_head = (const HornerJobsHead*)aux;
        const HornerJob* d_jobs = (const HornerJob*)(aux + sizeof(HornerJobsHead));
        const uint32_t* d_order = (const uint32_t*)(aux + sizeof(HornerJobsHead) + (size_t)ch.count * sizeof(HornerJob));
        uint64_t* d_evals = (uint64_t*)(aux + o_evals);
        uint64_t* d_scratch = (uint64_t*)(aux + o_scratch);
        // 1. the job table: short jobs first in `order`, then the long ones
        const size_t table_bytes = sizeof(HornerJobsHead) + (size_t)ch.count * (sizeof(HornerJob) + 4);
        h_table.assign(table_bytes, 0);
        HornerJob* hj = (HornerJob*)(h_table.data() + sizeof(HornerJobsHead));
        uint32_t* order = (uint32_t*)(h_table.data() + sizeof(HornerJobsHead) + (size_t)ch.count * sizeof(HornerJob));
        uint32_t n_s = 0, n_l = 0;
        q_ptrs.clear(); q_len.clear(); q_where.clear();
        for (uint32_t k = 0; k < ch.count; ++k) {
            const UopJob& j = plan.jobs[ch.first + k];
            hj[k].coeffs = h_coeff_ptrs[j.index];
            hj[k].n = j.n;
            std::memcpy(hj[k].z, h_z + 4 * (size_t)j.index, 32);
            hj[k].q_off = j.q_off;
            hj[k].row_off = j.row_off;
            if (uop_short(j.n)) order[n_s++] = k;
            else order[ch.n_short + n_l++] = k;
            if (j.n >= 2) {
                q_ptrs.push_back(d_scratch + 4 * j.q_off); q_len.push_back(j.n - 1); q_where.push_back(j.index);
            } else {
                std::memset(h_proofs_xy + 12 * (size_t)j.index, 0, 96);         // degree 0 < 1: quotient zero, proof = G1::default()
                h_proofs_inf[j.index] = 1;
            }
        }
        // (from here to the chunk's synchronisation nothing returns: the copy reads h_table, the scans write the arena)
        hipError_t he = hipMemcpyAsync(aux, h_table.data(), table_bytes, hipMemcpyHostToDevice, c->stream);
        // 2. the scans
        if (he == hipSuccess) {
            ProfScope ps(c, "horner_jobs", 0.0);
            if (ch.n_short)
                hipLaunchKernelGGL(horner_jobs_short_kernel, dim3(1, ch.n_short), dim3(HS_T), 0, c->stream, d_head, d_jobs, d_order, d_scratch, d_evals);
            if (ch.n_long) {
                hipLaunchKernelGGL(horner_jobs_scan_kernel<false>, dim3(ch.max_blocks, ch.n_long), dim3(HS_T), 0, c->stream, d_jobs, d_order, ch.n_short, d_scratch, d_evals);
                hipLaunchKernelGGL(horner_jobs_top_kernel, dim3(ch.n_long), dim3(1024), 0, c->stream, d_jobs, d_order, ch.n_short, d_scratch);
                hipLaunchKernelGGL(horner_jobs_scan_kernel<true>, dim3(ch.max_blocks, ch.n_long), dim3(HS_T), 0, c->stream, d_jobs, d_order, ch.n_short, d_scratch, d_evals);
            }
        }
        if (he == hipSuccess) he = hipGetLastError();
        // 3. the quotients' commits: zkhip_kzg_commit_polys behind its checks
        int rc = ZKHIP_OK;
        if (he == hipSuccess && !q_ptrs.empty()) {
            std::shared_ptr<const CppPlan> cplan;
            rc = commit_polys_plan(n_points, q_len.data(), (uint32_t)q_len.size(), table, &cplan);
            if (rc == ZKHIP_OK)
                rc = commit_polys_routes(c, d_points_xy, d_table_with_header, d_table, d_points_inf, n_points, *cplan, (uint32_t)q_ptrs.size(), q_ptrs.data(),
                                         q_len.data(), q_where.data(), h_proofs_xy, h_proofs_inf);
        }
        // 4. the evaluations: one copy and one synchronisation per chunk (the synchronisation also after an error: h_table and the
        // arena are in use until the stream is idle)
        h_ev.resize(4 * (size_t)ch.count);
        if (he == hipSuccess && rc == ZKHIP_OK) he = hipMemcpyAsync(h_ev.data(), d_evals, 32 * (size_t)ch.count, hipMemcpyDeviceToHost, c->stream);
        const hipError_t se = hipStreamSynchronize(c->stream);
        ZK_TRY(rc);
        ZK_HIP(c, he);
        ZK_HIP(c, se);
        for (uint32_t k = 0; k < ch.count; ++k) std::memcpy(h_evaluations + 4 * (size_t)plan.jobs[ch.first + k].index, h_ev.data() + 4 * (size_t)k, 32);
    }
    return ZKHIP_OK;
}

// DenseUnivariatePolynomial::evaluate (dense_univariate.rs:184-196) and ::degree (:199-207) on a device coefficient vector
extern "C" int zkhip_dense_evaluate(zkhip_ctx* c, const uint64_t* d_coeffs, size_t n, const uint64_t* h_z, uint64_t* h_out) {
    if (!c || !h_z || !h_out || (n && !d_coeffs)) return ZKHIP_ERR_ARG;
    if (n == 0) { std::memset(h_out, 0, 32); return ZKHIP_OK; }
    ZK_TRY(c->activate());
    const size_t per_block = (size_t)HS_T * HS_L;
    const uint32_t n_blocks = (uint32_t)((n + per_block - 1) / per_block);
    ZK_TRY(c->reserve_aux(64 * (size_t)n_blocks + 512));
    uint64_t* d_vals = (uint64_t*)c->aux.ptr;
    uint64_t* d_carry = d_vals + 4 * (size_t)n_blocks;
    uint64_t* d_eval = d_carry + 4 * (size_t)n_blocks;
    FrArg z = {};
    std::memcpy(z.v, h_z, 32);
    hipLaunchKernelGGL(horner_scan_kernel<false>, dim3(n_blocks), dim3(HS_T), 0, c->stream, d_coeffs, n, z, d_vals, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(horner_top_kernel, dim3(1), dim3(1024), 0, c->stream, d_vals, n_blocks, z, d_carry, d_eval);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_eval, 32, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_out, c->pinned_u64(ZK_PIN_RES), 32);
    return ZKHIP_OK;
}
extern "C" int zkhip_dense_degree(zkhip_ctx* c, const uint64_t* d_coeffs, size_t n, size_t* h_degree) {
    if (!c || !h_degree || (n && !d_coeffs)) return ZKHIP_ERR_ARG;
    *h_degree = 0;
    if (n == 0) return ZKHIP_OK;
    ZK_TRY(c->activate());
    unsigned long long* d_out = (unsigned long long*)c->small_u64(ZK_SMALL_RES);
    ZK_HIP(c, hipMemsetAsync(d_out, 0, 8, c->stream));
    hipLaunchKernelGGL(dense_degree_kernel, dim3(mle_grid(n)), dim3(MLE_BLOCK), 0, c->stream, d_coeffs, n, d_out);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(c->pinned_u64(ZK_PIN_RES), d_out, 8, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    *h_degree = (size_t)c->pinned_u64(ZK_PIN_RES)[0];
    return ZKHIP_OK;
}

// the generator's window table of this context (built once: 32 chains of 255 additions, ~10 ms)
static int srs_gen_table(zkhip_ctx* c, const uint64_t** table_xy) {
    const size_t n_tab = (size_t)SRS_WINDOWS * SRS_DIGITS;
    if (!c->d_gen_table) {
        DevMem owner;
        if (dev_alloc(owner, n_tab * 97 + 256 + n_tab * 192) != hipSuccess) return ZKHIP_ERR_NOMEM;
        void* const mem = owner.get();
        uint64_t* xy = (uint64_t*)mem;
        uint8_t* inf = (uint8_t*)mem + n_tab * 96;                 // never set: no multiple d * 2^(8w) * G with d < 256 is the identity
        uint64_t* xyzz = (uint64_t*)((char*)mem + ((n_tab * 97 + 255) & ~(size_t)255));
        hipLaunchKernelGGL(srs_gen_table_kernel, dim3(1), dim3(64), 0, c->stream, xyzz);
        const size_t n_threads = (n_tab + SRS_CHUNK - 1) / SRS_CHUNK;
        hipLaunchKernelGGL(srs_batch_affine_kernel, dim3((unsigned)((n_threads + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0,
                           c->stream, xyzz, n_tab, xy, inf);
        if (hipGetLastError() != hipSuccess) return ZKHIP_ERR_HIP;
        c->d_gen_table = std::move(owner);
    }
    *table_xy = (const uint64_t*)c->d_gen_table.get();
    return ZKHIP_OK;
}

// scalars (device, n x 4) -> affine SRS points
static int srs_from_scalars(zkhip_ctx* c, const uint64_t* d_scalars, size_t n, uint64_t* d_out_xy, uint8_t* d_out_inf) {
    // workspace layout: [scalars n*32 (owned by caller region)] ... we only need n*192 for XYZZ here
    uint64_t* xyzz = (uint64_t*)((char*)c->ws.ptr + ((n * 32 + 255) & ~(size_t)255));
    const uint64_t* table = nullptr;
    ZK_TRY(srs_gen_table(c, &table));
    hipLaunchKernelGGL(srs_fixed_base_window_kernel, dim3((unsigned)((n + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0, c->stream,
                       d_scalars, n, table, xyzz);
    const size_t n_threads = (n + SRS_CHUNK - 1) / SRS_CHUNK;
    hipLaunchKernelGGL(srs_batch_affine_kernel, dim3((unsigned)((n_threads + SRS_BLOCK - 1) / SRS_BLOCK)), dim3(SRS_BLOCK), 0,
                       c->stream, xyzz, n, d_out_xy, d_out_inf);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

extern "C" int zkhip_srs_multilinear_g1(zkhip_ctx* c, const uint64_t* h_tau, uint32_t n_vars, uint64_t* d_out_xy,
                                        uint8_t* d_out_inf) {
    if (!c || !d_out_xy || !d_out_inf || (n_vars && !h_tau)) return ZKHIP_ERR_ARG;
    if (n_vars > 30 || n_vars > ZK_MAX_ROUNDS) return ZKHIP_ERR_SHAPE;
    ZK_TRY(c->activate());
    const size_t n = (size_t)1 << n_vars;
    ZK_TRY(c->reserve_ws(((n * 32 + 255) & ~(size_t)255) + n * 192));
    PtsArg tau = {};
    if (n_vars) std::memcpy(tau.v, h_tau, 32 * (size_t)n_vars);
    uint64_t* d_scalars = (uint64_t*)c->ws.ptr;
    hipLaunchKernelGGL(srs_eq_scalars_kernel, dim3(mle_grid(n)), dim3(SRS_BLOCK), 0, c->stream, tau, n_vars, d_scalars);
    return srs_from_scalars(c, d_scalars, n, d_out_xy, d_out_inf);
}

extern "C" int zkhip_srs_univariate_g1(zkhip_ctx* c, const uint64_t* h_tau, size_t max_degree, uint64_t* d_out_xy,
                                       uint8_t* d_out_inf) {
    if (!c || !d_out_xy || !d_out_inf || !h_tau) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    const size_t n = max_degree + 1;
    ZK_TRY(c->reserve_ws(((n * 32 + 255) & ~(size_t)255) + n * 192));
    FrArg tau = {};
    std::memcpy(tau.v, h_tau, 32);
    uint64_t* d_scalars = (uint64_t*)c->ws.ptr;
    hipLaunchKernelGGL(srs_power_scalars_kernel, dim3(mle_grid(n)), dim3(SRS_BLOCK), 0, c->stream, tau, n, d_scalars);
    return srs_from_scalars(c, d_scalars, n, d_out_xy, d_out_inf);
}

extern "C" int zkhip_g1_sum_affine(const uint64_t* h_points_xy, const uint8_t* h_points_inf, size_t n,
                                   uint64_t* h_out_xy, uint8_t* h_out_inf) {
    if ((n && !h_points_xy) || !h_out_xy || !h_out_inf) return ZKHIP_ERR_ARG;
    zkhost::Xyzz acc = zkhost::xyzz_identity();
    for (size_t i = 0; i < n; ++i)
        acc = zkhost::xyzz_add(acc, zkhost::xyzz_from_affine(h_points_xy + 12 * i, h_points_inf && h_points_inf[i]));
    *h_out_inf = zkhost::xyzz_to_affine(acc, h_out_xy) ? 0 : 1;
    return ZKHIP_OK;
}

