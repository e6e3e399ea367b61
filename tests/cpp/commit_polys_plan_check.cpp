// commit_polys_plan_check.cpp -- the chunk planner of zkhip_kzg_commit_polys (csrc/commit_polys_plan.hpp) and the geometry mode it plans
// for (csrc/msm_geometry.hpp, "one set of points"), without a GPU: built with g++ under the host sanitizers by
// tests/test_commit_polys_plan_cpu.py.  Neither header has HIP in it.
//   1. plans: B in 1 .. 200, lengths from {1, 17, 4096, 4097, 2^13, 2^14, 2^16, 2^17, 2^20}, uniform and mixed, n_points >= the longest,
//      with and without a table -- the chunks cover every polynomial once and in order, every chunk's geometry builds, its partitions,
//      windows, scalars and pairs are within the sort's limits, every sort item lands on the problem's own points, the workspace bound holds;
//   2. the geometries of the modes that existed before (one problem, several disjoint problems, one table, level tables) are what they
//      were: a digest over every field, recorded from the header as it stood before the new mode.
#include <cstdio>
#include <cstdlib>
#include <vector>

#ifdef CPP_CHECK_PARENT_HEADER
#include "msm_geometry.hpp"      // (found with -I: the header of another revision, to record its digests with `commit_polys_plan_check print`)
#else
#include "../../zk-cryptography_amd/csrc/commit_polys_plan.hpp"
#endif

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

static const size_t LENGTHS[] = {1, 17, 4096, 4097, (size_t)1 << 13, (size_t)1 << 14, (size_t)1 << 16, (size_t)1 << 17, (size_t)1 << 20};
static const int N_LENGTHS = (int)(sizeof(LENGTHS) / sizeof(LENGTHS[0]));

#ifndef CPP_CHECK_PARENT_HEADER
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rng() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static void check_plan(size_t n_points, const std::vector<size_t>& len, bool table) {
    const uint32_t batch = (uint32_t)len.size();
    const CppPlan p = cpp_plan(n_points, len.data(), batch, table);
    size_t longest = 0;
    for (size_t l : len) longest = std::max(longest, l);
    CHECK(p.status == ZKHIP_OK, "n_points %zu batch %u table %d: status %d", n_points, batch, (int)table, p.status);
    // the chunks cover every polynomial exactly once, in order
    uint32_t next = 0;
    for (const CppChunk& ch : p.chunks) {
        CHECK(ch.first == next && ch.count >= 1, "chunk at %u, expected %u", ch.first, next);
        next += ch.count;
    }
    CHECK(next == batch, "covered %u of %u", next, batch);
    if (batch == 1) CHECK(p.route == CPP_SINGLE, "one polynomial is the single call's");
    if (p.route == CPP_SHORT) {
        size_t sum_short = 0;
        for (size_t l : len) sum_short += l;
        CHECK(table && longest <= CPP_SMALL_MAX && sum_short <= CPP_SHORT_TOTAL_MAX, "short route without a table or above its limits");
        for (const CppChunk& ch : p.chunks) CHECK(ch.count <= CPP_SMALL_CHUNK, "short chunk of %u", ch.count);
        return;
    }
    size_t sum = 0;
    for (size_t l : len) sum += l;
    if (batch > 1) CHECK(!(table && longest <= CPP_SMALL_MAX && sum <= CPP_SHORT_TOTAL_MAX), "the short route serves this batch");
    if (p.route == CPP_SINGLE) {
        for (const CppChunk& ch : p.chunks) CHECK(ch.count == 1, "single commits in a chunk of %u", ch.count);
        return;
    }
    // the bucket route: only where it was measured to gain
    CHECK(p.route == CPP_BUCKET && longest <= (table ? CPP_TABLE_MAX : CPP_PLAIN_MAX) && (!table || batch >= CPP_TABLE_MIN_BATCH), "bucket route");
    bool any_multi = false;
    for (const CppChunk& ch : p.chunks) any_multi = any_multi || ch.count > 1;
    CHECK(any_multi, "a bucket route of single commits");
    for (const CppChunk& ch : p.chunks) {
        CHECK(ch.count <= (uint32_t)MSM_MAX_PROBLEMS && ch.pr.n == ch.count, "chunk of %u", ch.count);
        size_t total = 0, conv = 0;
        for (uint32_t j = 0; j < ch.count; ++j) {
            CHECK(ch.pr.off[j] == total, "off[%u]", j);
            total += len[ch.first + j];
            conv = std::max(conv, len[ch.first + j]);
        }
        CHECK(ch.pr.off[ch.count] == total && ch.n_total == total && total < ((size_t)1 << 31), "total %zu", total);
        CHECK(ch.n_conv == (table ? 0 : conv), "n_conv %zu", ch.n_conv);
        // its geometry builds, and is the one the plan carries
        MsmGeometry g;
        const int rc = msm_build_geometry(ch.pr, table, table ? n_points : 0, g, true);
        CHECK(rc == ZKHIP_OK, "geometry of chunk at %u (%u problems): %d", ch.first, ch.count, rc);
        CHECK(ch.geo && ch.geo->wins.size() == g.wins.size() && ch.geo->pl.n_buckets == g.pl.n_buckets && ch.geo->items == g.items, "the plan's geometry");
        CHECK(g.pl.n_parts <= (uint32_t)SORT_MAX_PARTS && g.wins.size() <= (size_t)MSM_MAX_WINS && g.pl.n_wins == g.wins.size(), "parts %u wins %zu",
              g.pl.n_parts, g.wins.size());
        CHECK(g.items < ((size_t)1 << 31), "items %zu", g.items);
        CHECK(g.prob_set_first.size() == (size_t)ch.count + 1 && g.prob_set_first[ch.count] == g.pl.n_sets, "sets per problem");
        const size_t stride = table ? n_points : 0;
        size_t items = 0;
        for (uint32_t j = 0; j < ch.count; ++j) {
            const size_t nj = len[ch.first + j];
            CHECK(g.win_first[j] == ch.pr.win_first[j] && g.win_first[j + 1] > g.win_first[j], "win_first[%u]", j);
            uint32_t bits = 0;
            for (uint32_t v = g.win_first[j]; v < g.win_first[j + 1]; ++v) {
                const uint32_t w = v - g.win_first[j];
                bits += g.wins[v].bits & 0xffu;
                // every item index of the problem: entry_off + i (mod 2^32), i in [off[j], off[j+1]) -- affine in i, so the ends decide
                const uint32_t lo = g.wins[v].entry_off + ch.pr.off[j], hi = g.wins[v].entry_off + (ch.pr.off[j + 1] - 1);
                CHECK((size_t)lo == (size_t)w * stride && (size_t)hi == (size_t)w * stride + nj - 1 && hi < 0x80000000u,
                      "problem %u window %u: items [%u, %u], points from %zu, %zu of them", j, w, lo, hi, (size_t)w * stride, nj);
                // its partitions belong to a set of the problem
                const uint32_t set_of = g.part_set[g.wins[v].part_base];
                CHECK(set_of >= g.prob_set_first[j] && set_of < g.prob_set_first[j + 1], "window %u of problem %u sorts into set %u", w, j, set_of);
            }
            CHECK(bits >= 256 && bits < 256 + 16, "problem %u: %u bits", j, bits);      // (a pass of one problem has uniform windows: the top one may be short)
            items += nj * (g.win_first[j + 1] - g.win_first[j]);
        }
        CHECK(items == g.items, "items %zu / %zu", items, g.items);
        // the workspace: msm_enqueue's carve-up, within the bound unless the chunk is a single commit
        CHECK(ch.ws_bytes == cpp_ws_bytes(g, total, ch.n_conv), "ws_bytes");
        CHECK(ch.count == 1 || ch.ws_bytes <= CPP_WS_MAX, "chunk of %u at %u: %zu bytes", ch.count, ch.first, ch.ws_bytes);
    }
}

#endif

// ---- the modes that existed before ----------------------------------------------------------------------------------------------------
static uint64_t fnv(uint64_t h, uint64_t v) {
    for (int b = 0; b < 8; ++b) { h ^= (v >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    return h;
}
static uint64_t geometry_digest(const MsmProblems& pr, bool shared, size_t stride) {
    MsmGeometry g;
    const int rc = msm_build_geometry(pr, shared, stride, g);
    uint64_t h = fnv(14695981039346656037ull, (uint64_t)(int64_t)rc);
    if (rc != ZKHIP_OK) return h;
    const MsmPlan& pl = g.pl;
    for (uint64_t v : {(uint64_t)pl.n_sets, (uint64_t)pl.n_buckets, (uint64_t)pl.n_parts, (uint64_t)pl.n_terms, (uint64_t)pl.n_rc, (uint64_t)pl.n_rcwg,
                       (uint64_t)pl.n_termwg, (uint64_t)pl.n_wins, (uint64_t)pl.shared, (uint64_t)g.items, (uint64_t)g.heavy_min})
        h = fnv(h, v);
    for (const MsmWin& w : g.wins) for (uint64_t v : {(uint64_t)w.part_base, (uint64_t)w.entry_off, (uint64_t)w.bits, (uint64_t)w.pad}) h = fnv(h, v);
    for (const MsmSet& s : g.sets)
        for (uint64_t v : {(uint64_t)s.bucket_base, (uint64_t)s.part_base, (uint64_t)s.bits, (uint64_t)s.term_base, (uint64_t)s.rc_base, (uint64_t)s.rcwg_base,
                           (uint64_t)s.termwg_base})
            h = fnv(h, v);
    for (uint16_t v : g.part_set) h = fnv(h, v);
    for (uint16_t v : g.rcwg_set) h = fnv(h, v);
    for (uint16_t v : g.termwg_set) h = fnv(h, v);
    for (uint32_t v : g.set_exp) h = fnv(h, v);
    for (uint32_t v : g.prob_set_first) h = fnv(h, v);
    for (uint32_t j = 0; j <= pr.n; ++j) h = fnv(h, g.win_first[j]);
    return h;
}
struct OldCase { const char* name; bool shared; size_t stride; std::vector<size_t> len; uint64_t digest; };
static std::vector<OldCase> old_cases() {
    std::vector<size_t> rounds20, rounds12, odd;
    for (size_t h = (size_t)1 << 19; h >= 1; h /= 2) rounds20.push_back(h);
    for (size_t h = (size_t)1 << 11; h >= 1; h /= 2) rounds12.push_back(h);
    for (size_t k = 0; k < 64; ++k) odd.push_back(1 + 977 * k);
    return {
        {"one problem, 1 scalar", false, 0, {1}, 0x7c74b17df435f04aull},
        {"one problem, 300 scalars", false, 0, {300}, 0x9f1ab9658000bac9ull},
        {"one problem, 2^12 scalars", false, 0, {4096}, 0x5323bfbd5acc9a52ull},
        {"one problem, 2^13 scalars", false, 0, {8192}, 0xa065d8cbdaed125full},
        {"one problem, 2^20 scalars", false, 0, {(size_t)1 << 20}, 0xeee0689e1aac9176ull},
        {"several: the rounds of an opening at 2^20", false, 0, rounds20, 0x5303dea0044d6502ull},
        {"several: the rounds of an opening at 2^12", false, 0, rounds12, 0x201e08c813f870a4ull},
        {"several: 64 problems of odd sizes", false, 0, odd, 0xb2aff336e6adf340ull},
        {"several: 5 and 2^16", false, 0, {5, 65536}, 0xab23988cda248b60ull},
        {"several: 64 problems of 100000 scalars", false, 0, std::vector<size_t>(64, 100000), 0xf84fa99992ca8011ull},
        {"one table of 2^20 points", true, (size_t)1 << 20, {(size_t)1 << 20}, 0xe612629d3fbcfddcull},
        {"one table of 2^12 points", true, 4096, {4096}, 0xd8aa615837b07203ull},
        {"one table of 2^16 points, 1000 scalars", true, 65536, {1000}, 0x2d4d2f74fadeac2eull},
        {"level tables at 2^20", true, 0, rounds20, 0x0561b1ffa56e2babull},
        {"level tables at 2^12", true, 0, rounds12, 0xcdca65a07f0e1b68ull},
    };
}
static void check_old_modes(bool print) {
    for (const OldCase& oc : old_cases()) {
        MsmProblems pr = {};
        pr.n = (uint32_t)oc.len.size();
        for (uint32_t j = 0; j < pr.n; ++j) pr.off[j + 1] = pr.off[j] + (uint32_t)oc.len[j];
        const uint64_t d = geometry_digest(pr, oc.shared, oc.stride);
        if (print) { std::printf("%s 0x%016llxull\n", oc.name, (unsigned long long)d); continue; }
        CHECK(d == oc.digest, "%s: digest 0x%016llx, recorded 0x%016llx", oc.name, (unsigned long long)d, (unsigned long long)oc.digest);
#ifndef CPP_CHECK_PARENT_HEADER
        MsmGeometry a, b;       // the flag's default is the old behaviour
        CHECK(msm_build_geometry(pr, oc.shared, oc.stride, a) == msm_build_geometry(pr, oc.shared, oc.stride, b, false) && a.wins.size() == b.wins.size() &&
              a.pl.n_buckets == b.pl.n_buckets, "%s: the default flag", oc.name);
#endif
    }
}

int main(int argc, char** argv) {      // any argument: print the digests of the old modes instead of checking them
    (void)argv;
    check_old_modes(argc > 1);
    if (argc > 1) return 0;
#ifndef CPP_CHECK_PARENT_HEADER
    static const uint32_t BATCHES[] = {1, 2, 3, 4, 5, 8, 13, 31, 32, 33, 51, 52, 53, 63, 64, 65, 100, 128, 129, 200};
    for (int table = 0; table < 2; ++table) {
        // uniform
        for (int li = 0; li < N_LENGTHS; ++li)
            for (uint32_t batch : BATCHES) {
                const size_t L = LENGTHS[li];
                size_t pow2 = 1;
                while (pow2 < L) pow2 *= 2;
                for (size_t n_points : {L, pow2, (size_t)1 << 20})
                    if (n_points >= L) check_plan(n_points, std::vector<size_t>(batch, L), table != 0);
            }
        // every B in 1 .. 200 at the sizes where a lone commit is latency
        for (uint32_t batch = 1; batch <= 200; ++batch)
            for (size_t L : {(size_t)1 << 13, (size_t)1 << 14, (size_t)4097}) check_plan((size_t)1 << 14, std::vector<size_t>(batch, L), table != 0);
        // mixed
        for (int rep = 0; rep < 60; ++rep) {
            const uint32_t batch = 1 + rng() % 200;
            const int top = 1 + (int)(rng() % N_LENGTHS);       // lengths from the first `top` of the list
            std::vector<size_t> len(batch);
            size_t longest = 0;
            for (size_t& l : len) { l = LENGTHS[rng() % top]; longest = std::max(longest, l); }
            check_plan(longest, len, table != 0);
            check_plan((size_t)1 << 20, len, table != 0);
        }
        // the geometry mode itself at the sizes the planner leaves to single commits: two and three problems of 2^17 / 2^20 scalars
        for (size_t L : {(size_t)1 << 17, (size_t)1 << 20})
            for (uint32_t count : {2u, 3u}) {
                MsmProblems pr = {};
                pr.n = count;
                for (uint32_t j = 0; j < count; ++j) pr.off[j + 1] = pr.off[j] + (uint32_t)(L - j);
                MsmGeometry g;
                const int rc = msm_build_geometry(pr, table != 0, table ? L : 0, g, true);
                if (table && count * (1u << (msm_table_widths(L).hi - 1 - 8)) > (uint32_t)SORT_MAX_PARTS) {
                    CHECK(rc == ZKHIP_ERR_SHAPE, "more bucket sets than the sort has partitions for: %d", rc);
                    continue;
                }
                CHECK(rc == ZKHIP_OK && g.pl.n_parts <= (uint32_t)SORT_MAX_PARTS && g.wins.size() <= (size_t)MSM_MAX_WINS, "2^17 / 2^20: %d", rc);
                for (uint32_t j = 0; j < count; ++j)
                    for (uint32_t v = g.win_first[j]; v < g.win_first[j + 1]; ++v) {
                        const size_t base = table ? (size_t)(v - g.win_first[j]) * L : 0;
                        const uint32_t lo = g.wins[v].entry_off + pr.off[j], hi = g.wins[v].entry_off + (pr.off[j + 1] - 1);
                        CHECK((size_t)lo == base && (size_t)hi == base + (L - j) - 1 && hi < 0x80000000u, "problem %u window %u", j, v);
                    }
            }
        // the mixed batch of the GPU test, both ways
        check_plan((size_t)1 << 14, {1, 5, 300, 4096, 4097, 9000, 16384}, table != 0);
        check_plan((size_t)1 << 14, {16384, 9000, 4097, 4096, 300, 5, 1}, table != 0);
    }
#endif
    std::printf("checked %ld conditions\n", n_checked);
    return 0;
}
