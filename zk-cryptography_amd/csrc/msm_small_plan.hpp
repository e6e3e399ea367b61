// msm_small_plan.hpp -- what the MSM's short path (msm.hip; msm_kernels.hpp, "commits of a few thousand points") decides on the host before
// its two launches: which waves sum which problem's (point, window) pairs, and where partial sums and terms lie in the workspace.
// Functions of (the problems, how many instances share the chip) alone; the four drivers of msm.hip and
// tests/cpp/msm_small_plan_check.cpp share this one definition.  No HIP in here.
//
// A launch takes up to MSM_SMALL_PROBS PROBLEMS (the rounds of an opening, the polynomials of a PLONK round, one polynomial length) and
// `batch` instances of them as grid.z (the openings / proofs of a chunk, the polynomials of that length).  A SLOT is a wave per plane;
// the slots of a problem walk its pairs with a stride of all their lanes.
//
// THE SLOT RULE.  ~2 waves per SIMD (2048) over the WHOLE launch: 2048 / planes / batch slots per instance, dealt to the problems by their
// share of the pairs, at least one slot each and at most a wave per 64 pairs.  From a dozen instances on the minimum alone is more than the
// budget: one wave per (instance, problem, plane), and the chip is full of them.  But no lane walks more than OPEN_BATCH_LANE_PAIRS pairs:
// a full chip is as fast as its longest wave lets it be, and with one slot per round the first round of a 2^12 opening is ONE wave of 608
// pairs per lane beside waves of a handful -- measured at B = 64: 32 ms in the plane sums, no faster per opening than the loop, against
// 0.31 ms per opening at B = 16, whose share still split the round five ways (profiles/open_batch/NOTES.md).  At batch 1 the share alone
// is 8-17 pairs per lane and the cap changes no split, at any window width ZKHIP_LEVEL_TABLE_DELTA can produce (msm_small_plan_check.cpp
// compares with the rule without it), so the single commit and the single opening are this rule at batch 1: it has no cap parameter.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "msm_geometry.hpp"

namespace zk {

constexpr int MSM_SMALL_PROBS = 16;
constexpr size_t OPEN_BATCH_LANE_PAIRS = 32;      // most (point, window) pairs a lane of the plane sums walks

// n scalars from sc_off on against the table at tab_off (entries) of `stride` points with the widths lw
struct MsmSmallProblem { size_t n, stride, tab_off, sc_off; MsmLevelWidths lw; };

struct MsmSmallGeometry {
    uint32_t nprob, planes, total_slots;            // planes: the widest digit of the problems; problem j owns the slots [slot_first[j], slot_first[j + 1])
    uint32_t n[MSM_SMALL_PROBS], stride[MSM_SMALL_PROBS], W[MSM_SMALL_PROBS], hi[MSM_SMALL_PROBS], n_hi[MSM_SMALL_PROBS];
    uint32_t tab_off[MSM_SMALL_PROBS], sc_off[MSM_SMALL_PROBS], slot_first[MSM_SMALL_PROBS + 1];
    size_t total_pairs;                             // of one instance
    // `batch` instances: partials [b][plane][slot] of 256 bytes, terms [b][problem][plane] of 192 bytes
    size_t part_bytes(size_t batch) const { return batch * planes * total_slots * 256; }
    size_t terms_bytes(size_t batch) const { return batch * nprob * planes * 192; }
};

inline MsmSmallGeometry msm_small_plan(const MsmSmallProblem* pr, uint32_t nprob, uint32_t batch) {
    MsmSmallGeometry g = {};
    g.nprob = nprob;
    for (uint32_t j = 0; j < nprob; ++j) {
        g.n[j] = (uint32_t)pr[j].n; g.stride[j] = (uint32_t)pr[j].stride; g.W[j] = pr[j].lw.W; g.hi[j] = pr[j].lw.hi; g.n_hi[j] = pr[j].lw.n_hi;
        g.tab_off[j] = (uint32_t)pr[j].tab_off; g.sc_off[j] = (uint32_t)pr[j].sc_off;
        g.planes = std::max(g.planes, pr[j].lw.hi);
        g.total_pairs += pr[j].n * pr[j].lw.W;
    }
    const size_t budget = std::max<size_t>(1, 2048 / g.planes / batch);
    for (uint32_t j = 0; j < nprob; ++j) {
        const size_t pairs = pr[j].n * pr[j].lw.W, chunks = (pairs + 63) / 64;
        const size_t share = g.total_pairs ? (budget * pairs + g.total_pairs - 1) / g.total_pairs : 1;
        const size_t capped = (chunks + OPEN_BATCH_LANE_PAIRS - 1) / OPEN_BATCH_LANE_PAIRS;
        g.slot_first[j + 1] = g.slot_first[j] + (uint32_t)std::max<size_t>(1, std::min(chunks, std::max(share, capped)));
    }
    g.total_slots = g.slot_first[nprob];
    return g;
}

// The workspace of a chunk: partials | terms | tail, 256-byte aligned.  part_bytes: of every launch in front of the chunk's one copy;
// out_bytes: the terms and what the caller keeps right behind them for that copy to fetch too (the evaluations of a chunk of openings).
struct MsmSmallCarve { size_t terms_off, ws_bytes; };
inline MsmSmallCarve msm_small_carve(size_t part_bytes, size_t out_bytes) {
    const size_t terms_off = (part_bytes + 255) & ~(size_t)255;
    return {terms_off, terms_off + ((out_bytes + 255) & ~(size_t)255)};
}

}  // namespace zk
