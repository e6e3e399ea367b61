// multi_composed_batch_kernels.hpp -- B independent multi-composed sumcheck proofs in one launch, one workgroup per proof, for gfx950.
//
// MultiComposedSumcheckProver::prove_internal (sumcheck/src/composed/multi_composed_sumcheck.rs:64-121) of a small claim is a serial
// chain -- sums, interpolation, SHA-256, challenge, fold, and the next round needs that challenge.  B claims of one shape are B
// independent chains, so workgroup b walks ALL rounds of claim b, as sumcheck_batch_kernel does for the two sibling provers: the
// tables in LDS, the transcript in LDS (Sha256State, where close_round keeps it), nothing shared with another workgroup (no flags, no
// spinning, no assumption about which workgroups are resident together, no outer-transcript hasher).
//
// A round is composed_tail_kernel's round, from the same device functions (composed_kernels.hpp): tail_late_evals / tail_round_evals
// for the terms' sums, close_round for interpolation, zero drop, merge-add, absorb and challenge, TailShadow / tail_fold for the fold.
// What this kernel adds is the start of a proof and the rounds before the tables fit the LDS:
//   - the transcript starts fresh (first = 1: prove_partial, the claimed sum absorbed in round one) or from a state the host prepared
//     per proof (first = 2: prove, every table's bytes hashed first); the context's ComposedDev is read for the interpolation
//     matrices only (close_round<.., false>), so a continuation of a single proof or session never notices a batch call;
//   - T * n > CMP_TAIL_ENTRIES (T tables): the first rounds read the caller's tables (tail_round_evals over PointedTables) and fold
//     them into a per-proof slab of T * n / 2 entries, in place from the second such round on, until the folded tables fit -- the
//     caller's tables are only read, and pointers may repeat within and across proofs (every table has a slab of its own).
#pragma once
#include "composed_kernels.hpp"

namespace zk {

// Lanes per proof.  512 (the tail's: a record of up to 8 sums takes the wave-per-evaluation rounds; 255 VGPRs, so one workgroup per
// CU) against 256 (two workgroups per CU, records above 4 sums lose those rounds) is a measurement: profiles/multi_composed_batch/
// NOTES.md, "Block size".  -DZK_MCB_BLOCK=256 builds the other side of that comparison.
#ifndef ZK_MCB_BLOCK
#define ZK_MCB_BLOCK CMP_TAIL_BLOCK
#endif
constexpr int MCB_BLOCK = ZK_MCB_BLOCK;
static_assert(MCB_BLOCK == 256 || MCB_BLOCK == 512, "close_round needs the 144 interpolation lanes and a wave beside the hash");
constexpr uint32_t MCB_MAX_ENTRIES = 1u << 16;        // T * n above this: the entry point runs the single prover proof after proof
constexpr uint32_t MCB_ROUND_WORDS = 64;              // u64 per recorded round, close_round's layout: [0] #monomials, (coeff, pow) pairs from [8]

struct MultiComposedBatchArgs {
    CloseArgs ca;                    // meta, st (interpolation matrices), first (1 or 2); sum_dev = [proofs][4] claimed sums;
                                     // round_out = [proofs][n_vars][MCB_ROUND_WORDS], challenges = [proofs][n_vars][4]
    const uint64_t* const* tables;   // [proofs][T] device pointers, term after term
    const Sha256State* init;         // [proofs] transcript states (first = 2), or NULL
    uint64_t* slab;                  // [proofs][T][n / 2] (not touched when the proof is resident from the first round)
    uint32_t total;                  // T
    uint32_t n, n_vars;              // entries per table, a power of two >= 2
    uint32_t m;                      // entries per table in LDS: min(n, composed_tail_len(T))
};

// canonical big-endian bytes of the chunk's tables, table after table (composed_poly_to_bytes of every proof in a row): grid (x, tables)
static __global__ __launch_bounds__(MLE_BLOCK) void to_bytes_tables_kernel(const uint64_t* const* __restrict__ tables, uint32_t n,
                                                                    uint32_t* __restrict__ out_words) {
    const uint64_t* in = tables[blockIdx.y];
    uint32_t* out = out_words + 8 * (size_t)blockIdx.y * n;
    for (uint32_t q = blockIdx.x * MLE_BLOCK + threadIdx.x; q < n; q += gridDim.x * MLE_BLOCK) store_be_bytes(out, q, load_fr(in, q));
}

static __global__ __launch_bounds__(MCB_BLOCK) void multi_composed_batch_kernel(MultiComposedBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];
    uint32_t* tab = reinterpret_cast<uint32_t*>(zk_dyn_lds);   // T tables x m elements
    __shared__ CloseShared sh;
    __shared__ Fr wave_part[MCB_BLOCK / 64][CMP_MAX_REC];
    __shared__ Sha256State trs;
    __shared__ const uint64_t* src[CMP_MAX_TERMS * CMP_MAX_K];   // the current tables while they are in global memory
    const uint32_t b = blockIdx.x, tid = threadIdx.x, total = a.total, m = a.m;
    const ComposedMeta& meta = a.ca.meta;
    if (tid < total) src[tid] = a.tables[(size_t)b * total + tid];
    if (a.init && tid < sizeof(Sha256State) / 4)
        reinterpret_cast<uint32_t*>(&trs)[tid] = reinterpret_cast<const uint32_t*>(a.init + b)[tid];
    close_preload(sh, meta, a.ca.st);
    __syncthreads();
    uint32_t cn = a.n, first = a.ca.first;
    uint32_t round = b * a.n_vars;                   // close_round records at round_out + 64 * round and challenges + 4 * round
    // ---- rounds from global memory: sums over the caller's tables or the slab, folded into the slab or, once it fits, into LDS
    while (cn > m) {
        tail_round_evals<MCB_BLOCK>(PointedTables{src}, nullptr, meta, cn, sh, wave_part);
        close_round<NoShadow, false>(sh, a.ca, &trs, round, first, NoShadow(), b);
        first = 0;
        const uint32_t half = cn >> 1;
        const bool fits = half <= m;
        const Fr r = fr_to_mont_outlined(sh.challenge_canon);
        // lane (q, j) reads (j, j + half) of table q and writes j of its slab: in place there, no other lane touches index j this round
        for (uint32_t idx = tid; idx < total * half; idx += MCB_BLOCK) {
            const uint32_t q = idx / half, j = idx % half;
            const Fr v = fold_pair(load_fr(src[q], j), load_fr(src[q], (size_t)j + half), r);
            if (fits) lds_store_fr(tab, q * m + j, v);
            else store_fr(a.slab + 4 * ((size_t)b * total + q) * (a.n >> 1), j, v);
        }
        __syncthreads();   // (within the workgroup also for the slab: what a lane stored is what the next round's lanes read)
        if (tid < total) src[tid] = a.slab + 4 * ((size_t)b * total + tid) * (a.n >> 1);
        __syncthreads();
        cn = half;
        ++round;
    }
    if (cn == a.n) {       // resident from the first round
        for (uint32_t idx = tid; idx < total * m; idx += MCB_BLOCK) lds_store_fr(tab, idx, load_fr(src[idx / m], idx % m));
        __syncthreads();
    }
    // ---- resident rounds: composed_tail_kernel's
    for (;; ++round) {
        if (tail_late_round<MCB_BLOCK>(meta, cn)) tail_late_evals(tab, meta, m, cn, sh);
        else tail_round_evals<MCB_BLOCK>(LdsTables{tab, m}, tab, meta, cn, sh, wave_part);
        const uint32_t half = cn >> 1;
        close_round<TailShadow, false>(sh, a.ca, &trs, round, first, TailShadow{tab, total, m, cn == 2 ? 0u : half}, b);
        first = 0;
        if (cn == 2) break;   // the fold after the last round has no consumer
        tail_fold<MCB_BLOCK>(tab, total, m, half, sh.challenge_canon);
        __syncthreads();
        cn = half;
    }
}

}  // namespace zk
