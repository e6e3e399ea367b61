// fold_rounds.hpp -- the overlapped plan's big fold and the serial rounds that run beside it, as ONE launch (gfx950).
//
// The synchronous prover used to put the streaming k1-variable fold of the table on a second queue, behind an event, next to the
// serial kernel of rounds k1 .. g-1 (zkhip.hip, proof_overlapped): a cross-queue fork in front of the proof's longest kernel and a
// join behind it.  Here both are workgroups of one grid on one queue:
//   workgroup 0       is sumcheck_small_kernel's body (multifold_kernels.hpp), unchanged: the transcript wave, its priority, its
//                     barriers and its stamps are that workgroup's alone;
//   workgroups 1 .. F are multifold_mfma_kernel's tile loop (mfma_fold.hpp), one tile of 64 outputs per wave, tile index from
//                     (workgroup - 1, wave); same term order, rotation and loads.  The per-tile sums the stand-alone kernel leaves
//                     for the stage plan are neither reduced nor stored: this plan folds the result itself (blockfold_kernel).
// Both bodies are TEXT shared with the stand-alone kernels (sumcheck_small_body.hpp, mfma_fold_tile_body.hpp), not functions: those
// kernels run in every proof in flight and must stay the code they were, instruction for instruction (see there).
// A launch has one workgroup shape, the serial kernel's: SMALL_BLOCK lanes and FOLD_ROUNDS_LDS bytes of dynamic LDS -- the serial kernel's request at 2^10
// entries with weights is 148 KiB anyway -- so a CU holds exactly one workgroup and the transcript wave shares its CU with nobody,
// as before.  Workgroup 0 is dispatched first, so the serial rounds never wait for a CU behind the fold.
// There is no communication between the workgroups: the fold reads the table and the weights of the launch BEFORE, the serial
// workgroup reads the partial tables of the launch before, and what both write is read by the launch after.
#pragma once
#include "multifold_kernels.hpp"
#include "mfma_fold.hpp"

namespace zk {

// eight waves: 512 fold workgroups at 2^24.  (Twelve -- a second generation that still fills the memory system -- leave the fold 168
// registers of the 190 it needs: spills, step 0.304 against 0.281 ms; ten have the same limit: profiles/fold_rounds/NOTES.md.)
constexpr int FOLD_ROUNDS_WAVES = SMALL_BLOCK / 64;
constexpr int FOLD_ROUNDS_DEPTH = 4;             // terms per register set, as multifold_mfma_kernel<4, 4>
constexpr size_t FOLD_ROUNDS_LDS = 156 * 1024;   // + ~0.5 KiB of the fold's static LDS: one workgroup per CU (160 KiB)

// fold workgroups of a fold to m outputs (m a multiple of 64): the last one may have waves without a tile
__host__ __device__ constexpr uint32_t fold_rounds_workgroups(size_t m) { return (uint32_t)((m / 64 + FOLD_ROUNDS_WAVES - 1) / FOLD_ROUNDS_WAVES); }
// what the matrix-core fold form asks of its shape (launch_multifold's condition) and the fused launch of its LDS
__host__ __device__ constexpr bool fold_rounds_serves(size_t m, uint32_t k, size_t small_lds) {
    return m >= 8192 && (m & (m - 1)) == 0 && k >= 4 && k <= (uint32_t)MF_CAP_LOGK && small_lds <= FOLD_ROUNDS_LDS &&
           mfm_lds_bytes((1u << k) < (uint32_t)MFM_CHUNK ? (1u << k) : (uint32_t)MFM_CHUNK) <= FOLD_ROUNDS_LDS;
}

// grid 1 + fold_rounds_workgroups(m), SMALL_BLOCK lanes, FOLD_ROUNDS_LDS bytes of dynamic LDS.
// a, st, round_polys, challenges: sumcheck_small_kernel's arguments; in .. rot: multifold_mfma_kernel's (no per-tile sums)
static __global__ __launch_bounds__(SMALL_BLOCK) void fold_rounds_kernel(SmallArgs a, SumcheckDev* st, uint64_t* __restrict__ round_polys,
                                                                         uint64_t* __restrict__ challenges,
                                                                         const uint64_t* __restrict__ in, size_t m, uint32_t k,
                                                                         const uint64_t* __restrict__ weights, uint64_t* __restrict__ out,
                                                                         uint32_t rot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];   // the serial body's trees / the fold's digit strings
    if (blockIdx.x == 0) {
#include "sumcheck_small_body.hpp"
        return;
    }
    // ---- a fold workgroup: multifold_mfma_kernel<WAVES, DEPTH>'s preamble with the tile index of this launch, its tile, its store
    constexpr int WAVES = FOLD_ROUNDS_WAVES, DEPTH = FOLD_ROUNDS_DEPTH;
    uint32_t* qd = reinterpret_cast<uint32_t*>(zk_dyn_lds);
    const unsigned char* q_lds = zk_dyn_lds;                        // plane 0 = the unshifted strings
    __shared__ int32_t d_lds[32];        // digit sums of the current chunk
    __shared__ int32_t kc_lds[64];       // 128 * sum_{b,i} d[b][c - i], all chunks
    __shared__ long long kv_lds[16];     // the same per 32-bit limb: sum_t kc[4 g + t] << 8 t
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = lane & 31, h = lane >> 5;
    const uint32_t n_terms = 1u << k;
    const size_t own_tile = (size_t)(blockIdx.x - 1) * WAVES + wave, n_tiles = m / 64;
    const bool stores = own_tile < n_tiles;                          // a wave past the last tile repeats the last one (the barriers and the
    const size_t tile = stores ? own_tile : n_tiles - 1;             // strings need every wave) and stores nothing
#include "mfma_fold_tile_body.hpp"
    const Fr o = wide_redc(x);
    if (stores) store_fr(out, tile * 64 + lane, o);
}

}  // namespace zk
