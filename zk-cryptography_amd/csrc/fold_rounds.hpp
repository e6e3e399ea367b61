// fold_rounds.hpp -- the overlapped plan's big fold and the serial rounds that run beside it, as ONE launch (gfx950).
//
// The synchronous prover used to put the streaming k1-variable fold of the table on a second queue, behind an event, next to the
// serial kernel of rounds k1 .. g-1 (zkhip.hip, proof_overlapped): a cross-queue fork in front of the proof's longest kernel and a
// join behind it.  Here both are workgroups of one grid on one queue:
//   workgroup 0       is sumcheck_small_kernel's body (multifold_kernels.hpp), unchanged: the transcript wave, its priority, its
//                     barriers and its stamps are that workgroup's alone;
//   workgroups 1 .. F are multifold_mfma_kernel's fold (mfma_fold.hpp) -- same term order, rotation, loads, matrix-core products and
//                     epilogue arithmetic, so the same bits -- as RESIDENT workgroups: the host launches one per CU beside the serial
//                     workgroup's (F = min(tiles / 8, CUs - 1): 255 from 2^22 entries on) and every wave folds several tiles of 64
//                     outputs, by the schedule of fold_schedule.hpp, which depends on the grid alone:
//                       * the digit strings of the weights and the column constants are built once per workgroup where the terms
//                         fit one chunk (k <= 7), not once per tile;
//                       * a wave's q regular tiles are one stream of loads: the last loads of a tile are the first of the next,
//                         in flight during the epilogue;
//                       * the T % 8F leftover tiles (16 at F = 255) are folded FIRST, under full load, each by the eight waves of one
//                         workgroup: a wave takes an eighth of the terms, the partial limb values (integers below 2^56) are added in
//                         LDS and wave 0 finishes the tile.  One tile per wave for them measured slower than the launch this replaces.
//                     One tile per wave on 512 workgroups was two generations on 255 CUs and two workgroups more, which ran alone on
//                     an empty chip: 90.9 us against 82.9 now (profiles/fold_resident/NOTES.md).  At a grid of tiles / 8 workgroups
//                     or more (q <= 1) the schedule IS one tile per wave, a wave past the last tile repeats it and stores nothing.
//                     The kernel is correct at every grid of two or more workgroups (tests/test_gpu_fold_rounds_grid.py).
//                     The per-tile sums the stand-alone kernel leaves for the stage plan are neither reduced nor stored: this plan
//                     folds the result itself (blockfold_kernel).
// The serial body is TEXT shared with the stand-alone kernel (sumcheck_small_body.hpp), not a function: that kernel runs in every
// proof in flight and must stay the code it was, instruction for instruction (see there).  For the same reason the fold workgroups
// do not share code with multifold_mfma_kernel, whose tile stays in mfma_fold_tile_body.hpp untouched: the loop here wraps the
// middle of that tile, and its pieces (strings, terms, limb values, finish) are lambdas of this kernel alone.
// A launch has one workgroup shape, the serial kernel's: SMALL_BLOCK lanes and FOLD_ROUNDS_LDS bytes of dynamic LDS -- the serial kernel's request at 2^10
// entries with weights is 148 KiB anyway -- so a CU holds exactly one workgroup and the transcript wave shares its CU with nobody,
// as before.  Workgroup 0 is dispatched first, so the serial rounds never wait for a CU behind the fold.
// There is no communication between the workgroups: the fold reads the table and the weights of the launch BEFORE, the serial
// workgroup reads the partial tables of the launch before, and what both write is read by the launch after.
#pragma once
#include "multifold_kernels.hpp"
#include "mfma_fold.hpp"
#include "fold_schedule.hpp"

namespace zk {

// eight waves.  (Twelve leave the fold 168 registers of the 190 it needed with one tile per wave: spills, step 0.304 against 0.281 ms;
// ten have the same limit: profiles/fold_rounds/NOTES.md.  The resident loop has 216 of the 256 that eight waves allow.)
constexpr int FOLD_ROUNDS_WAVES = SMALL_BLOCK / 64;
constexpr int FOLD_ROUNDS_DEPTH = 4;             // terms per register set, as multifold_mfma_kernel<4, 4>
constexpr size_t FOLD_ROUNDS_LDS = 156 * 1024;   // + ~0.5 KiB of the fold's static LDS: one workgroup per CU (160 KiB)
// a leftover tile's exchange: 16 limb values of 64 bits per lane and wave, behind the digit strings (48.25 KiB at most)
constexpr size_t FOLD_ROUNDS_XCH = (size_t)FOLD_ROUNDS_WAVES * 16 * 64 * sizeof(long long);
static_assert(FOLD_ROUNDS_WAVES == (int)FOLD_WG_WAVES, "fold_schedule.hpp counts the waves of this workgroup");
static_assert(mfm_lds_bytes(MFM_CHUNK) % 16 == 0 && mfm_lds_bytes(MFM_CHUNK) + FOLD_ROUNDS_XCH <= FOLD_ROUNDS_LDS, "strings + exchange fit the launch's LDS");

// fold workgroups of a fold to m outputs (m a multiple of 64) at one tile per wave: the last one may have waves without a tile.
// The largest grid that is of use; the host launches fold_schedule_workgroups(m / 64, CUs)
__host__ __device__ constexpr uint32_t fold_rounds_workgroups(size_t m) { return (uint32_t)((m / 64 + FOLD_ROUNDS_WAVES - 1) / FOLD_ROUNDS_WAVES); }
// what the matrix-core fold form asks of its shape (launch_multifold's condition) and the fused launch of its LDS
__host__ __device__ constexpr bool fold_rounds_serves(size_t m, uint32_t k, size_t small_lds) {
    return m >= 8192 && (m & (m - 1)) == 0 && k >= 4 && k <= (uint32_t)MF_CAP_LOGK && small_lds <= FOLD_ROUNDS_LDS &&
           mfm_lds_bytes((1u << k) < (uint32_t)MFM_CHUNK ? (1u << k) : (uint32_t)MFM_CHUNK) <= FOLD_ROUNDS_LDS;
}

// grid 1 + F with any F >= 1, SMALL_BLOCK lanes, FOLD_ROUNDS_LDS bytes of dynamic LDS.
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
    // ---- a fold workgroup: resident, its tiles from the schedule of this grid (fold_schedule.hpp)
    constexpr int WAVES = FOLD_ROUNDS_WAVES, DEPTH = FOLD_ROUNDS_DEPTH;
    uint32_t* qd = reinterpret_cast<uint32_t*>(zk_dyn_lds);
    const unsigned char* q_lds = zk_dyn_lds;                        // plane 0 = the unshifted strings
    __shared__ int32_t d_lds[32];        // digit sums of the current chunk
    __shared__ int32_t kc_lds[64];       // 128 * sum_{b,i} d[b][c - i], all chunks
    __shared__ long long kv_lds[16];     // the same per 32-bit limb: sum_t kc[4 g + t] << 8 t
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = lane & 31, h = lane >> 5;
    const uint32_t n_terms = 1u << k;
    const FoldSchedule sched = fold_schedule(m / 64, gridDim.x - 1);
    const uint32_t wg = blockIdx.x - 1;
    const size_t g_wave = (size_t)wg * WAVES + wave;
    const size_t row = 32 * m;                                       // bytes between consecutive terms of one output
    const unsigned char* base = reinterpret_cast<const unsigned char*>(in) + 32 * n + 16 * h;
    const uint32_t chunk = n_terms < (uint32_t)MFM_CHUNK ? n_terms : (uint32_t)MFM_CHUNK;   // terms per chunk, a power of two
    const uint32_t plane = mfm_plane_dwords(chunk);
    const bool once = n_terms == chunk;                              // one chunk: its strings serve every tile of the workgroup
    const uint32_t* qa = qd + ((31 - n + 16 * h) & 3) * plane + ((31 - n + 16 * h) >> 2);   // this lane's window (mfma_fold_tile_body.hpp)
    long long* xch = reinterpret_cast<long long*>(zk_dyn_lds + mfm_lds_bytes(chunk));       // [wave][limb][lane], behind the strings
    mf_v4i da[DEPTH][2], db[DEPTH][2];
    mf_v16i acc00, acc01, acc10, acc11;                              // acc[jh][mh]

    // the strings of chunk t0 / chunk and its share of the column constants: the stand-alone kernel's code, barriers included
    auto build_chunk = [&](uint32_t t0) {
        __syncthreads();                                             // the previous chunk's strings are no longer read
        for (uint32_t idx = tid; idx < 4 * chunk; idx += 64 * WAVES) {
            const uint32_t t = idx >> 2, a = idx & 3;
            const Fr w = load_fr(weights, t0 + t);
            uint32_t qs[25];
            uint64_t c = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) { qs[i] = 0; qs[16 + i] = 0; }
            qs[24] = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) { c += (uint64_t)w.l[i] + 0x80808080u; qs[15 - i] = __builtin_bswap32((uint32_t)c ^ 0x80808080u); c >>= 32; }
            uint32_t* q = qd + a * plane + t * 24;
#pragma unroll
            for (int d = 0; d < 24; ++d) q[d] = (uint32_t)((((uint64_t)qs[d + 1] << 32) | qs[d]) >> (8 * a));
        }
        __syncthreads();
        if (tid < 32) {
            int32_t dsum = 0;
            for (uint32_t t = 0; t < chunk; ++t) dsum += (int32_t)(signed char)q_lds[t * MFM_QSTRIDE + 63 - tid];
            d_lds[tid] = dsum;
        }
        __syncthreads();
        if (tid < 64) {
            int32_t s = 0;
            const int lo = (int)tid - 31 < 0 ? 0 : (int)tid - 31, hi = tid < 31 ? (int)tid : 31;
            for (int x = lo; x <= hi; ++x) s += d_lds[x];
            kc_lds[tid] += 128 * s;
        }
    };
    auto limb_constants = [&]() {                                    // kc of all chunks -> kv, between two barriers
        __syncthreads();
        if (tid < 16) {
            long long v = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) v += (long long)kc_lds[4 * tid + t] << (8 * t);
            kv_lds[tid] = v;
        }
        __syncthreads();
    };
    // term `term` of the current chunk from register set d
    auto mfma_term = [&](const mf_v4i (&d)[2], uint32_t term) {
        const uint32_t* qt = qa + term * 24;
        const mf_v4i a0 = {(int)qt[8], (int)qt[9], (int)qt[10], (int)qt[11]}, a1 = {(int)qt[0], (int)qt[1], (int)qt[2], (int)qt[3]};
        const mf_v4i b0 = mfm_signed(d[0]), b1 = mfm_signed(d[1]);
        acc00 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc11, 0, 0, 0);
    };
    // lane (n, h) takes output 32 h + n (the swap of mfma_fold_tile_body.hpp); v[g] = this wave's columns 4 g .. 4 g + 3 as one value
    auto limb_sums = [&](long long (&v)[16]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            auto s0 = __builtin_amdgcn_permlane32_swap((unsigned)acc00[r], (unsigned)acc10[r], false, false);
            acc00[r] = (int)s0[0]; acc10[r] = (int)s0[1];
            auto s1 = __builtin_amdgcn_permlane32_swap((unsigned)acc01[r], (unsigned)acc11[r], false, false);
            acc01[r] = (int)s1[0]; acc11[r] = (int)s1[1];
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {                               // limb g = (mh, q, h') = (g / 8, (g / 2) % 4, g % 2)
            const int mh = g >> 3, q = (g >> 1) & 3, hp = g & 1;
            long long s = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int r = 4 * q + t;
                const int col = hp ? (mh ? acc11[r] : acc10[r]) : (mh ? acc01[r] : acc00[r]);
                s += (long long)col << (8 * t);
            }
            v[g] = s;
        }
    };
    // the tile's entry of this lane from the limb values of all its terms: constants, carries, reduction, store
    auto finish = [&](const long long (&v)[16], size_t tile) {
        uint32_t x[18];
        long long carry = 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const long long s = carry + kv_lds[g] + v[g];
            x[g] = (uint32_t)s;
            carry = s >> 32;
        }
        x[16] = (uint32_t)carry;
        x[17] = 0;
        store_fr(out, tile * 64 + lane, wide_redc(x));
    };

    if (tid < 64) kc_lds[tid] = 0;
    const size_t n_left = fold_wg_leftovers(sched, wg), n_own = sched.q ? sched.q : 1;
    // this wave's regular tiles as one stream of steps: step S is term S % n_terms (in the tile's rotated order) of its tile
    // S / n_terms; a wave without a tile (q = 0, past the last one) repeats the last tile and stores nothing.  Steps past the end are
    // clamped to the last one and never used.
    const bool stores = sched.q != 0 || g_wave < sched.tiles;
    const size_t tile0 = stores ? g_wave : sched.tiles - 1;
    const size_t last_step = n_own * n_terms - 1;
    auto step_ptr = [&](size_t S) -> const unsigned char* {
        S = S < last_step ? S : last_step;
        const size_t tile = fold_wave_tile(sched, tile0, S >> k);
        const uint32_t s = (uint32_t)S & (n_terms - 1), start = (uint32_t)(tile * rot) & (chunk - 1);
        const uint32_t term = (s & ~(chunk - 1)) | ((s + start) & (chunk - 1));
        return base + 2048 * tile + (size_t)term * row;
    };
    auto load_first = [&]() {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) { const unsigned char* pt = step_ptr(u); da[u][0] = mfm_load_nt(pt); da[u][1] = mfm_load_nt(pt + 1024); }
    };
    if (n_left == 0) load_first();                                   // in flight while the strings are built
    if (once) { build_chunk(0); limb_constants(); }

    // ---- leftover tiles first, under full load: each wave takes chunk / WAVES consecutive terms of every chunk, the limb values of the
    // eight waves are added in LDS (integers below 2^56: exact) and wave 0 finishes the tile
    for (size_t j = 0; j < n_left; ++j) {
        const size_t tile = fold_wg_leftover_tile(sched, wg, j);
        const unsigned char* p = base + 2048 * tile;
        const uint32_t start = (uint32_t)(tile * rot) & (chunk - 1), share = chunk / WAVES, u0 = wave * share;   // share = 2 .. 16
        acc00 = {0}; acc01 = {0}; acc10 = {0}; acc11 = {0};
        if (!once && tid < 64) kc_lds[tid] = 0;
        for (uint32_t t0 = 0; t0 < n_terms; t0 += chunk) {
            if (!once) build_chunk(t0);
            for (uint32_t t = 0; t < share; t += 2 * DEPTH) {
#pragma unroll
                for (int u = 0; u < DEPTH; ++u) {
                    const uint32_t ua = t + u < share ? t + u : share - 1, ub = t + DEPTH + u < share ? t + DEPTH + u : share - 1;
                    const unsigned char* pa = p + (size_t)(t0 | ((u0 + ua + start) & (chunk - 1))) * row;
                    const unsigned char* pb = p + (size_t)(t0 | ((u0 + ub + start) & (chunk - 1))) * row;
                    da[u][0] = mfm_load_nt(pa); da[u][1] = mfm_load_nt(pa + 1024);
                    db[u][0] = mfm_load_nt(pb); db[u][1] = mfm_load_nt(pb + 1024);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < DEPTH; ++u) if (t + u < share) mfma_term(da[u], (u0 + t + u + start) & (chunk - 1));
#pragma unroll
                for (int u = 0; u < DEPTH; ++u) if (t + DEPTH + u < share) mfma_term(db[u], (u0 + t + DEPTH + u + start) & (chunk - 1));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (!once) limb_constants();
        long long v[16];
        limb_sums(v);
#pragma unroll
        for (int g = 0; g < 16; ++g) xch[(wave * 16 + g) * 64 + lane] = v[g];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {                                // limbs 2 wave, 2 wave + 1 of every output: only this lane touches them
            const uint32_t g = 2 * wave + e;
            long long s = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += xch[(w * 16 + g) * 64 + lane];
            xch[g * 64 + lane] = s;
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int g = 0; g < 16; ++g) v[g] = xch[g * 64 + lane];
            finish(v, tile);
        }
    }
    if (n_left != 0) load_first();

    // ---- the regular tiles: two register sets of DEPTH terms in flight; the last loads of a tile are the first of the next
    for (size_t j = 0; j < n_own; ++j) {
        const size_t tile = fold_wave_tile(sched, tile0, j), S0 = j * n_terms;
        const uint32_t start = (uint32_t)(tile * rot) & (chunk - 1);
        acc00 = {0}; acc01 = {0}; acc10 = {0}; acc11 = {0};
        if (!once && tid < 64) kc_lds[tid] = 0;
        for (uint32_t t0 = 0; t0 < n_terms; t0 += chunk) {
            if (!once) build_chunk(t0);
            for (uint32_t t = 0; t < chunk; t += 2 * DEPTH) {
                const size_t S = S0 + t0 + t;                        // step of da[0]
#pragma unroll
                for (int u = 0; u < DEPTH; ++u) { const unsigned char* pt = step_ptr(S + DEPTH + u); db[u][0] = mfm_load_nt(pt); db[u][1] = mfm_load_nt(pt + 1024); }
                __builtin_amdgcn_sched_barrier(0);                   // keep the issue order (mfma_fold_tile_body.hpp)
#pragma unroll
                for (int u = 0; u < DEPTH; ++u) mfma_term(da[u], (t + u + start) & (chunk - 1));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < DEPTH; ++u) { const unsigned char* pt = step_ptr(S + 2 * DEPTH + u); da[u][0] = mfm_load_nt(pt); da[u][1] = mfm_load_nt(pt + 1024); }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < DEPTH; ++u) mfma_term(db[u], (t + DEPTH + u + start) & (chunk - 1));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (!once) limb_constants();
        long long v[16];
        limb_sums(v);
        if (stores) finish(v, tile);
    }
}

}  // namespace zk
