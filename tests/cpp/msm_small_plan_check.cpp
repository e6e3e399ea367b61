// msm_small_plan_check.cpp -- the slot rule and the workspace carve-up of the MSM's short path (csrc/msm_small_plan.hpp) without a GPU:
// built with g++ under the host sanitizers by tests/test_msm_small_plan_cpu.py.  The header has no HIP in it.
// The four drivers of msm.hip each carried the rule; their formulas stand below as they stood there (old_single, old_open_batch,
// old_plonk, old_short), and msm_small_plan must give their slot_first[], total_slots, planes and per-problem arrays over
//   1. single commits: n_points 1 .. 299, the powers of two up to 4096 and 4095; n 1 .. n_points (n_points < 300 or a power of two) or
//      {1, n_points / 2, n_points - 1, n_points} -- at the default widths and at every window size 8 .. 20;
//   2. one opening: n_vars 2 .. 12 at the default level widths, at every uniform window size 8 .. 20 and at every ZKHIP_LEVEL_TABLE_DELTA
//      -- against the single driver's rule, which had no lane cap (so these runs decide that the rule needs no cap parameter), and
//      against the batched rule at one opening;
//   3. batched openings: n_vars 2 .. 12 x chunks of {1, 2, 3, 16, 17, 63, 64};
//   4. PLONK: m 1 .. 3 lengths from {1, 6, 64, 70, 1030, 4096} <= n_points in {64, 1024, 4096}, batch {1, 2, 3, 16, 64, 1000, 65535};
//   5. short-route classes: lengths {1, 17, 64, 300, 1000, 2000, 4096} <= n_points in {256, 4096}, chunks of 1 .. 64 polynomials.
// Every plan: slot_first strictly increasing from 0, a problem's slots <= ceil(pairs / 64), no lane walks more than OPEN_BATCH_LANE_PAIRS
// pairs, and the carve-up holds batch x planes x total_slots partials and batch x nprob x planes terms.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zk-cryptography_amd/csrc/msm_small_plan.hpp"

using namespace zk;

static long n_checked = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        ++n_checked;                                                             \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);      \
            std::printf(__VA_ARGS__);                                            \
            std::printf("\n");                                                   \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

// what a driver filled by hand: the per-problem arrays, planes and its slot split
struct Old {
    uint32_t nprob = 0, planes = 0, total_slots = 0;
    uint32_t n[MSM_SMALL_PROBS] = {}, stride[MSM_SMALL_PROBS] = {}, W[MSM_SMALL_PROBS] = {}, hi[MSM_SMALL_PROBS] = {}, n_hi[MSM_SMALL_PROBS] = {};
    uint32_t tab_off[MSM_SMALL_PROBS] = {}, sc_off[MSM_SMALL_PROBS] = {}, slot_first[MSM_SMALL_PROBS + 1] = {};
};

// ---- the four rules as they stood in msm.hip -------------------------------------------------------------------------------------------
static Old old_single(const MsmSmallProblem* pr, uint32_t nprob) {                       // msm_small_batch
    Old a;
    a.nprob = nprob;
    size_t total_pairs = 0;
    for (uint32_t j = 0; j < nprob; ++j) {
        a.n[j] = (uint32_t)pr[j].n; a.stride[j] = (uint32_t)pr[j].stride; a.W[j] = pr[j].lw.W; a.hi[j] = pr[j].lw.hi; a.n_hi[j] = pr[j].lw.n_hi;
        a.tab_off[j] = (uint32_t)pr[j].tab_off; a.sc_off[j] = (uint32_t)pr[j].sc_off;
        a.planes = std::max(a.planes, pr[j].lw.hi);
        total_pairs += pr[j].n * pr[j].lw.W;
    }
    const size_t budget = std::max<size_t>(1, 2048 / a.planes);
    for (uint32_t j = 0; j < nprob; ++j) {
        const size_t pairs = pr[j].n * pr[j].lw.W, chunks = (pairs + 63) / 64;
        const size_t share = total_pairs ? (budget * pairs + total_pairs - 1) / total_pairs : 1;
        a.slot_first[j + 1] = a.slot_first[j] + (uint32_t)std::max<size_t>(1, std::min(chunks, share));
    }
    a.total_slots = a.slot_first[nprob];
    return a;
}
static Old old_open_batch(size_t n, uint32_t n_vars, uint32_t bc_max, const MsmLevelWidths* widths) {      // kzg_open_small_batch
    Old a;
    a.nprob = n_vars;
    size_t entry = 0, lvl_off = 0, total_pairs = 0;
    for (uint32_t j = 0; j < n_vars; ++j) {
        const size_t h = n >> (j + 1);
        const MsmLevelWidths lw = widths[j];
        a.n[j] = (uint32_t)h; a.stride[j] = (uint32_t)h; a.W[j] = lw.W; a.hi[j] = lw.hi; a.n_hi[j] = lw.n_hi;
        a.tab_off[j] = (uint32_t)entry; a.sc_off[j] = (uint32_t)lvl_off;
        a.planes = std::max(a.planes, lw.hi);
        total_pairs += h * lw.W;
        entry += (size_t)lw.W * h;
        lvl_off += h;
    }
    const size_t budget = std::max<size_t>(1, 2048 / a.planes / bc_max);
    for (uint32_t j = 0; j < n_vars; ++j) {
        const size_t pairs = (size_t)a.n[j] * a.W[j], chunks = (pairs + 63) / 64;
        const size_t share = (budget * pairs + total_pairs - 1) / total_pairs, capped = (chunks + OPEN_BATCH_LANE_PAIRS - 1) / OPEN_BATCH_LANE_PAIRS;
        a.slot_first[j + 1] = a.slot_first[j] + (uint32_t)std::max<size_t>(1, std::min(chunks, std::max(share, capped)));
    }
    a.total_slots = a.slot_first[n_vars];
    return a;
}
static Old old_plonk(size_t n_points, uint32_t batch, uint32_t m, const size_t* sc_off, const size_t* lens) {      // zk_msm_commit_batch
    const MsmLevelWidths lw = msm_table_widths(n_points);
    Old a;
    a.nprob = m; a.planes = lw.hi;
    size_t total_pairs = 0;
    for (uint32_t j = 0; j < m; ++j) {
        a.n[j] = (uint32_t)lens[j]; a.stride[j] = (uint32_t)n_points; a.W[j] = lw.W; a.hi[j] = lw.hi; a.n_hi[j] = lw.n_hi;
        a.tab_off[j] = 0; a.sc_off[j] = (uint32_t)sc_off[j];
        total_pairs += lens[j] * lw.W;
    }
    const size_t budget = std::max<size_t>(1, 2048 / a.planes / batch);
    for (uint32_t j = 0; j < m; ++j) {
        const size_t pairs = lens[j] * lw.W, chunks = (pairs + 63) / 64;
        const size_t share = (budget * pairs + total_pairs - 1) / total_pairs, capped = (chunks + OPEN_BATCH_LANE_PAIRS - 1) / OPEN_BATCH_LANE_PAIRS;
        a.slot_first[j + 1] = a.slot_first[j] + (uint32_t)std::max<size_t>(1, std::min(chunks, std::max(share, capped)));
    }
    a.total_slots = a.slot_first[m];
    return a;
}
static Old old_short(size_t n_points, size_t len, uint32_t count) {       // commit_polys_short: a class of one length in a chunk of `count`
    const MsmLevelWidths lw = msm_table_widths(n_points);
    const size_t budget = std::max<size_t>(1, 2048 / lw.hi / count);
    const size_t pairs = len * lw.W, chunks = (pairs + 63) / 64, capped = (chunks + OPEN_BATCH_LANE_PAIRS - 1) / OPEN_BATCH_LANE_PAIRS;
    const uint32_t slots = (uint32_t)std::max<size_t>(1, std::min(chunks, std::max(budget, capped)));
    Old a;
    a.nprob = 1; a.planes = lw.hi; a.total_slots = slots;
    a.n[0] = (uint32_t)len; a.stride[0] = (uint32_t)n_points; a.W[0] = lw.W; a.hi[0] = lw.hi; a.n_hi[0] = lw.n_hi;
    a.slot_first[1] = slots;
    return a;
}

// ---- the plan against a rule, and what holds for every plan -----------------------------------------------------------------------------
static void check_plan(const char* what, const MsmSmallProblem* pr, uint32_t nprob, uint32_t batch, const Old& o) {
    const MsmSmallGeometry g = msm_small_plan(pr, nprob, batch);
    CHECK(g.nprob == o.nprob && g.planes == o.planes && g.total_slots == o.total_slots, "%s: nprob %u / %u, planes %u / %u, slots %u / %u (batch %u, n[0] %zu)",
          what, g.nprob, o.nprob, g.planes, o.planes, g.total_slots, o.total_slots, batch, pr[0].n);
    size_t total_pairs = 0;
    CHECK(g.slot_first[0] == 0, "%s: slot_first[0]", what);
    for (uint32_t j = 0; j < nprob; ++j) {
        CHECK(g.n[j] == o.n[j] && g.stride[j] == o.stride[j] && g.W[j] == o.W[j] && g.hi[j] == o.hi[j] && g.n_hi[j] == o.n_hi[j] &&
              g.tab_off[j] == o.tab_off[j] && g.sc_off[j] == o.sc_off[j], "%s: the arrays of problem %u", what, j);
        CHECK(g.slot_first[j + 1] == o.slot_first[j + 1], "%s: slot_first[%u] %u, the driver's rule %u (batch %u, n %u, W %u, hi %u)", what, j + 1,
              g.slot_first[j + 1], o.slot_first[j + 1], batch, g.n[j], g.W[j], g.hi[j]);
        const size_t pairs = (size_t)g.n[j] * g.W[j], slots = g.slot_first[j + 1] - g.slot_first[j];
        CHECK(g.slot_first[j + 1] > g.slot_first[j] && slots <= (pairs + 63) / 64, "%s: problem %u has %zu slots for %zu pairs", what, j, slots, pairs);
        CHECK(64 * OPEN_BATCH_LANE_PAIRS * slots >= pairs, "%s: a lane of problem %u walks more than %zu of %zu pairs in %zu slots", what, j,
              OPEN_BATCH_LANE_PAIRS, pairs, slots);
        total_pairs += pairs;
    }
    for (uint32_t j = nprob; j < (uint32_t)MSM_SMALL_PROBS; ++j) CHECK(g.n[j] == 0 && g.W[j] == 0 && g.slot_first[j + 1] == 0, "%s: problem %u is none", what, j);
    CHECK(g.total_pairs == total_pairs, "%s: total_pairs", what);
    // the bytes: partials [b][plane][slot] of 256, terms [b][problem][plane] of 192, a tail behind the terms
    for (size_t tail : {(size_t)0, (size_t)32 * batch}) {
        const MsmSmallCarve cv = msm_small_carve(g.part_bytes(batch), g.terms_bytes(batch) + tail);
        CHECK(g.part_bytes(batch) >= (size_t)batch * g.planes * g.total_slots * 256 && g.terms_bytes(batch) >= (size_t)batch * nprob * g.planes * 192, "%s: sizes", what);
        CHECK(cv.terms_off % 256 == 0 && cv.terms_off >= g.part_bytes(batch) && cv.ws_bytes >= cv.terms_off + g.terms_bytes(batch) + tail &&
              cv.ws_bytes < cv.terms_off + g.terms_bytes(batch) + tail + 256, "%s: carve-up", what);
    }
}

static MsmLevelWidths widths_of(uint32_t c) {        // msm_level_table_widths' layout for windows of at most c bits
    MsmLevelWidths lw;
    lw.W = (256 + c - 1) / c;
    lw.hi = (256 + lw.W - 1) / lw.W;
    lw.n_hi = 256 - lw.W * (lw.hi - 1);
    return lw;
}
static bool is_pow2(size_t n) { return n && !(n & (n - 1)); }

static void single_commits() {
    std::vector<size_t> sizes;
    for (size_t p = 1; p < 300; ++p) sizes.push_back(p);
    for (size_t p = 512; p <= 4096; p *= 2) sizes.push_back(p);
    sizes.push_back(4095);
    long shapes = 0;
    for (size_t n_points : sizes) {
        std::vector<size_t> ns;
        if (n_points < 300 || is_pow2(n_points)) for (size_t n = 1; n <= n_points; ++n) ns.push_back(n);
        else ns = {1, n_points / 2, n_points - 1, n_points};
        for (size_t n : ns) {
            ++shapes;
            std::vector<MsmLevelWidths> widths = {msm_table_widths(n_points)};
            for (uint32_t c = 8; c <= 20; ++c) widths.push_back(widths_of(c));
            for (const MsmLevelWidths& lw : widths) {
                const MsmSmallProblem one = {n, n_points, 0, 0, lw};
                check_plan("single commit", &one, 1, 1, old_single(&one, 1));
            }
        }
    }
    std::printf("single commits: %ld shapes x (the default widths, 8 .. 20 bits)\n", shapes);
}

// an opening of 2^n_vars entries whose level j has the widths lw[j], single and in chunks
static void opening(uint32_t n_vars, const MsmLevelWidths* lw, bool chunks) {
    const size_t n = (size_t)1 << n_vars;
    MsmSmallProblem sp[MSM_SMALL_PROBS];
    size_t entry = 0, lvl_off = 0;
    for (uint32_t j = 0; j < n_vars; ++j) {
        const size_t h = n >> (j + 1);
        sp[j] = {h, h, entry, lvl_off, lw[j]};
        entry += (size_t)lw[j].W * h;
        lvl_off += h;
    }
    check_plan("one opening, the single driver's rule", sp, n_vars, 1, old_single(sp, n_vars));
    check_plan("one opening, the batched rule", sp, n_vars, 1, old_open_batch(n, n_vars, 1, lw));
    if (!chunks) return;
    for (uint32_t bc : {1u, 2u, 3u, 16u, 17u, 63u, 64u}) check_plan("batched openings", sp, n_vars, bc, old_open_batch(n, n_vars, bc, lw));
}
static void openings() {
    for (uint32_t n_vars = 2; n_vars <= 12; ++n_vars) {
        const size_t n = (size_t)1 << n_vars;
        MsmLevelWidths lw[MSM_SMALL_PROBS];
        for (uint32_t j = 0; j < n_vars; ++j) lw[j] = msm_level_table_widths(n >> (j + 1), n - 1);
        opening(n_vars, lw, true);
        for (uint32_t c = 8; c <= 20; ++c) {                                       // every window size, all levels alike
            for (uint32_t j = 0; j < n_vars; ++j) lw[j] = widths_of(c);
            opening(n_vars, lw, true);
        }
        for (int delta = -20; delta <= 12; ++delta) {                              // every ZKHIP_LEVEL_TABLE_DELTA: log2(level) - delta bits, within 8 .. 20
            for (uint32_t j = 0; j < n_vars; ++j) lw[j] = widths_of((uint32_t)std::min(20, std::max(8, (int)(n_vars - 1 - j) - delta)));
            opening(n_vars, lw, true);
        }
    }
}

static void plonk() {
    static const size_t LENS[] = {1, 6, 64, 70, 1030, 4096};
    for (size_t n_points : {(size_t)64, (size_t)1024, (size_t)4096})
        for (uint32_t m = 1; m <= 3; ++m)
            for (int code = 0; code < 6 * 6 * 6; ++code) {                         // every m-tuple of the lengths
                if ((m < 3 && code / 36) || (m < 2 && code / 6)) continue;
                const size_t lens[3] = {LENS[code % 6], LENS[code / 6 % 6], LENS[code / 36]};
                size_t sc_off[3] = {0, 0, 0};
                bool fits = true;
                for (uint32_t j = 0; j < m; ++j) { fits = fits && lens[j] <= n_points; sc_off[j] = j * n_points + 3 * j; }
                if (!fits) continue;
                const MsmLevelWidths lw = msm_table_widths(n_points);
                MsmSmallProblem sp[3];
                for (uint32_t j = 0; j < m; ++j) sp[j] = {lens[j], n_points, 0, sc_off[j], lw};
                for (uint32_t batch : {1u, 2u, 3u, 16u, 64u, 1000u, 65535u}) check_plan("PLONK", sp, m, batch, old_plonk(n_points, batch, m, sc_off, lens));
            }
}

static void short_classes() {
    for (size_t n_points : {(size_t)256, (size_t)4096})
        for (size_t len : {(size_t)1, (size_t)17, (size_t)64, (size_t)300, (size_t)1000, (size_t)2000, (size_t)4096}) {
            if (len > n_points) continue;
            const MsmSmallProblem one = {len, n_points, 0, 0, msm_table_widths(n_points)};
            for (uint32_t count = 1; count <= 64; ++count) check_plan("short-route class", &one, 1, count, old_short(n_points, len, count));
        }
}

int main() {
    single_commits();
    openings();
    plonk();
    short_classes();
    std::printf("checked %ld conditions\n", n_checked);
    return 0;
}
