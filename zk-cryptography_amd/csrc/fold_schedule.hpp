// fold_schedule.hpp -- which wave of fold_rounds_kernel (fold_rounds.hpp) folds which tile of 64 outputs.  A function of the grid
// alone: the kernel, the host that picks the grid and tests/test_fold_rounds_schedule_cpu.py share this one definition.  No HIP in here.
//
// F fold workgroups of FOLD_WG_WAVES waves, W = FOLD_WG_WAVES * F waves, T tiles, q = T / W, rem = T % W.
//   regular tiles   wave g = FOLD_WG_WAVES * workgroup + wave takes tiles g, g + W, .., g + (q - 1) W: neighbouring waves keep
//                   neighbouring tiles, and every wave of the launch has the same number of them;
//   leftover tiles  q W + i, i < rem, go round-robin to the workgroups, i to workgroup i % F, and each is folded by its whole workgroup;
//   q = 0           (a grid of at least T / FOLD_WG_WAVES fold workgroups) nothing is cooperative: wave g takes tile g, and a wave
//                   past the last tile has none.
// The assignment is static: no workgroup learns anything from another.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define ZK_SCHED_HD __host__ __device__ constexpr
#else
#define ZK_SCHED_HD constexpr
#endif

namespace zk {

constexpr uint32_t FOLD_WG_WAVES = 8;        // waves of a fold workgroup (= FOLD_ROUNDS_WAVES, fold_rounds.hpp)

struct FoldSchedule {
    size_t tiles;        // T
    uint32_t wgs;        // F >= 1
    size_t waves;        // W
    size_t q;            // regular tiles per wave
    size_t rem;          // leftover tiles when q > 0; T itself when q = 0
};
ZK_SCHED_HD FoldSchedule fold_schedule(size_t tiles, uint32_t wgs) {
    return FoldSchedule{tiles, wgs, (size_t)FOLD_WG_WAVES * wgs, tiles / ((size_t)FOLD_WG_WAVES * wgs), tiles % ((size_t)FOLD_WG_WAVES * wgs)};
}
// tiles the waves of a workgroup take one each, in turn (q, or -- q = 0 -- the one tile of the waves that have one)
ZK_SCHED_HD size_t fold_wave_tiles(const FoldSchedule& s, size_t g) { return s.q ? s.q : (g < s.tiles ? 1 : 0); }
ZK_SCHED_HD size_t fold_wave_tile(const FoldSchedule& s, size_t g, size_t j) { return g + j * s.waves; }
// leftover tiles, folded by a whole workgroup each
ZK_SCHED_HD size_t fold_leftovers(const FoldSchedule& s) { return s.q ? s.rem : 0; }
ZK_SCHED_HD uint32_t fold_leftover_owner(const FoldSchedule& s, size_t i) { return (uint32_t)(i % s.wgs); }
ZK_SCHED_HD size_t fold_wg_leftovers(const FoldSchedule& s, uint32_t wg) {
    return fold_leftovers(s) > wg ? (fold_leftovers(s) - wg + s.wgs - 1) / s.wgs : 0;
}
ZK_SCHED_HD size_t fold_wg_leftover_tile(const FoldSchedule& s, uint32_t wg, size_t j) { return s.q * s.waves + wg + j * s.wgs; }

// fold workgroups the host launches on a device of `cus` compute units: one tile per wave while the workgroups fit beside the
// serial workgroup's CU, else one resident workgroup on every other CU
ZK_SCHED_HD uint32_t fold_schedule_workgroups(size_t tiles, uint32_t cus) {
    const size_t one_each = (tiles + FOLD_WG_WAVES - 1) / FOLD_WG_WAVES, resident = cus > 1 ? cus - 1 : 1;
    return (uint32_t)(one_each < resident ? one_each : resident);
}

}  // namespace zk
