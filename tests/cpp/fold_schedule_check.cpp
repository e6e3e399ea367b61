// fold_schedule_check.cpp -- stand-alone program around csrc/fold_schedule.hpp for tests/test_fold_rounds_schedule_cpu.py (g++, no HIP).
// For every T in 1 .. max_tiles and F in 1 .. max_wgs: the regular and the leftover assignments cover every tile exactly once, q = 0 is
// one tile per wave, no workgroup gets more than ceil(rem / F) leftovers, leftover i belongs to the workgroup that lists it.
// Prints one line per violation (at most 20) and "checked <pairs>"; exit status 1 on a violation.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zk-cryptography_amd/csrc/fold_schedule.hpp"

using namespace zk;

// the figures the prover runs at, at compile time: 2^18 outputs on a part of 256 CUs
static_assert(fold_schedule_workgroups(4096, 256) == 255, "one resident workgroup per CU beside the serial one");
static_assert(fold_schedule(4096, 255).q == 2 && fold_schedule(4096, 255).rem == 16, "F = 255: q = 2, rem = 16");
static_assert(fold_schedule_workgroups(132, 256) == 17 && fold_schedule(132, 17).q == 0, "a small fold keeps one tile per wave");
static_assert(fold_schedule_workgroups(4096, 1) == 1 && fold_schedule_workgroups(1, 256) == 1, "never no fold workgroup");

static int bad = 0;
static void fail(size_t T, unsigned F, const char* what, size_t a, size_t b) {
    if (bad++ < 20) std::printf("T=%zu F=%u: %s (%zu, %zu)\n", T, F, what, a, b);
}

int main(int argc, char** argv) {
    const size_t max_tiles = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4200;
    const unsigned max_wgs = argc > 2 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 300;
    size_t pairs = 0;
    std::vector<unsigned char> seen;
    for (size_t T = 1; T <= max_tiles; ++T)
        for (unsigned F = 1; F <= max_wgs; ++F, ++pairs) {
            const FoldSchedule s = fold_schedule(T, F);
            seen.assign(T, 0);
            if (s.waves != (size_t)FOLD_WG_WAVES * F || s.q * s.waves + s.rem != T || s.rem >= s.waves) fail(T, F, "q, rem", s.q, s.rem);
            const size_t g_end = s.waves < T + FOLD_WG_WAVES ? s.waves : T + FOLD_WG_WAVES;   // (and the first waves without a tile)
            for (size_t g = 0; g < g_end; ++g) {
                const size_t cnt = fold_wave_tiles(s, g);
                if (s.q == 0 && cnt != (g < T ? 1u : 0u)) fail(T, F, "q = 0 is one tile per wave", g, cnt);
                if (s.q != 0 && cnt != s.q) fail(T, F, "every wave has q regular tiles", g, cnt);
                for (size_t j = 0; j < cnt; ++j) {
                    const size_t t = fold_wave_tile(s, g, j);
                    if (s.q == 0 && t != g) fail(T, F, "q = 0: wave g takes tile g", g, t);
                    if (t >= T) fail(T, F, "regular tile out of range", g, t); else ++seen[t];
                }
            }
            const size_t left = fold_leftovers(s), most = (left + F - 1) / F;
            if (left != (s.q ? s.rem : 0)) fail(T, F, "leftovers", left, s.rem);
            size_t dealt = 0;
            for (unsigned wg = 0; wg < F; ++wg) {
                const size_t cnt = fold_wg_leftovers(s, wg);
                if (cnt > most) fail(T, F, "more than ceil(rem / F) leftovers", wg, cnt);
                dealt += cnt;
                for (size_t j = 0; j < cnt; ++j) {
                    const size_t t = fold_wg_leftover_tile(s, wg, j);
                    if (t < s.q * s.waves || t >= T) { fail(T, F, "leftover tile out of range", wg, t); continue; }
                    ++seen[t];
                    if (fold_leftover_owner(s, t - s.q * s.waves) != wg) fail(T, F, "leftover's owner", wg, t);
                }
            }
            if (dealt != left) fail(T, F, "leftovers dealt", dealt, left);
            for (size_t t = 0; t < T; ++t) if (seen[t] != 1) fail(T, F, "tile not covered exactly once", t, (size_t)seen[t]);
        }
    std::printf("checked %zu\n", pairs);
    return bad ? 1 : 0;
}
