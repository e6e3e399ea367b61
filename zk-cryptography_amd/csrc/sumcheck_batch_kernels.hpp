// sumcheck_batch_kernels.hpp -- B independent sumcheck proofs in one launch, one workgroup per proof, for gfx950.
//
// Sumcheck::prove (sumcheck/src/sumcheck.rs:29-61) and ComposedSumcheck::prove (sumcheck/src/composed/composed_sumcheck.rs:32-67)
// of a small table are serial by construction: SHA-256, challenge, fold, and the next round needs that challenge.  B such proofs
// are B independent chains, so workgroup b walks ALL rounds of proof b: its tables in LDS, its transcript in wave 0's registers.
// The workgroups never talk to each other (no flags, no spinning, no assumption about which of them are resident together).
//
// The two provers differ in two places only:
//   ABSORB_SUM = true  (basic, K = 1): the claimed sum is absorbed first (32 bytes), then per round (lo, hi);
//   ABSORB_SUM = false (composed, K tables): nothing first, per round the K + 1 values sum_x prod_k f_k(t, x), t = 0..K.
// vec_to_bytes and Multilinear::to_bytes are the same encoding, so a K = 1 composed round polynomial IS (lo, hi).
#pragma once
#include "mle_kernels.hpp"

namespace zk {

constexpr int SCB_BLOCK = 256;                        // lanes per proof ...
constexpr int SCB_WAVE_BLOCK = 64;                    // ... one wave for proofs of at most SCB_WAVE_ENTRIES entries (K * n), as measured:
constexpr uint32_t SCB_WAVE_ENTRIES = 1024;           //     profiles/sumcheck_batch/NOTES.md, "One wave or four"
constexpr uint32_t SCB_LDS_ENTRIES = TAIL_N;          // K * len <= 2^12 entries (128 KiB) are resident in LDS
constexpr uint32_t SCB_MAX_ENTRIES = 1u << 16;        // K * n above this: the entry points run the single provers one after another
constexpr uint32_t SCB_CHUNK = 1024;                  // proofs per launch
constexpr uint32_t SCB_MIN_CHUNK = 256;               // ... never fewer (one workgroup per CU), whatever the slabs take
constexpr size_t SCB_SLAB_BYTES = (size_t)256 << 20;  // most global scratch a chunk asks of the workspace (256 proofs of 2^16 entries)
// proofs per launch of every batched sumcheck prover, from the global scratch one proof needs (slab, staging; 0: resident)
inline uint32_t scb_chunk(size_t scratch_per_proof) {
    if (!scratch_per_proof) return SCB_CHUNK;
    const size_t fit = SCB_SLAB_BYTES / scratch_per_proof;
    return (uint32_t)(fit < SCB_MIN_CHUNK ? SCB_MIN_CHUNK : fit > SCB_CHUNK ? SCB_CHUNK : fit);
}

// Fewest proofs from which on the batch kernel measured faster per proof than the better thing a caller could do without it
// (profiles/sumcheck_batch/NOTES.md, "Where the kernel starts to pay"): for the basic prover eight proofs in flight through
// zkhip_sumcheck_prove_begin / _end, for the composed prover a loop of zkhip_composed_prove.  A proof on this kernel takes 1.5 - 2 x
// the single provers' time (one plain SHA-256 compression per round beside the wave-wide one); B of them take hardly longer.
inline uint32_t scb_min_batch(bool basic, uint32_t k, size_t n) {
    if (basic) return n <= 64 ? 3 : n <= 4096 ? 4 : n <= 16384 ? 6 : 16;
    if (k * n > 32768) return 6;        // not measured for the composed prover: the basic prover's bound against its loop at 2^16
    return k == 2 ? 2 : 3;              // K = 2 and 5 measured; 1, 3 and 4 take the larger bound
}
// entries per table from which on a proof is resident: the first of n, n/2, ... with K * len <= SCB_LDS_ENTRIES
inline uint32_t scb_resident_len(uint32_t k, size_t n) {
    size_t len = n;
    while (k * len > SCB_LDS_ENTRIES) len >>= 1;
    return (uint32_t)len;
}
inline int scb_block(uint32_t k, size_t n) { return k * n <= SCB_WAVE_ENTRIES ? SCB_WAVE_BLOCK : SCB_BLOCK; }
// LDS scratch behind the tables: the block reductions' 2 * waves slots, the K + 2 values the round absorbs, the challenge
inline size_t scb_lds_bytes(uint32_t k, uint32_t resident_len) {
    return ((size_t)k * resident_len + 2 * (SCB_BLOCK / 64) + (k + 2) + 1) * sizeof(Fr);
}
constexpr size_t SCB_MAX_LDS_BYTES = ((size_t)SCB_LDS_ENTRIES + 2 * (SCB_BLOCK / 64) + (5 + 2) + 1) * sizeof(Fr);   // the family's largest request
// words of one proof's results: [absorbed sum (ABSORB_SUM)] [round values: n_vars x (K + 1)] [challenges: n_vars]
inline uint32_t scb_out_words(uint32_t k, uint32_t n_vars, bool absorb_sum) { return 4 * ((absorb_sum ? 1 : 0) + n_vars * (k + 2)); }

struct SumcheckBatchArgs {
    const uint64_t* const* tables;   // [proofs][K] device pointers (they may repeat: the tables are only read)
    const uint64_t* claimed;         // [proofs][4] sums to absorb as given, or NULL: every proof absorbs lo + hi of its first round
    uint64_t* slab;                  // [proofs][K][n / 2] scratch of the rounds too large for LDS (not touched when the proof is resident)
    uint64_t* out;                   // [proofs][out_words]
    uint32_t n;                      // entries per table, a power of two >= 2
    uint32_t resident_len;           // scb_resident_len(K, n)
    uint32_t out_words;              // scb_out_words(K, log2 n, ABSORB_SUM)
};

// acc[t] += prod_k (lo_k + t (hi_k - lo_k)), t = 0..K, for one index pair
template <int K>
__device__ __forceinline__ void scb_accumulate(Fr (&acc)[K + 1], const Fr (&lo)[K], const Fr (&hi)[K]) {
    if (K == 1) {   // v(1) = hi itself
        acc[0] = acc[0] + lo[0];
        acc[1] = acc[1] + hi[0];
        return;
    }
    Fr d[K], v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { d[k] = hi[k] - lo[k]; v[k] = lo[k]; }
#pragma unroll
    for (int t = 0; t <= K; ++t) {
        if (t) {
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = v[k] + d[k];
        }
        Fr p = v[0];
#pragma unroll
        for (int k = 1; k < K; ++k) p = p * v[k];
        acc[t] = acc[t] + p;
    }
}

template <int K, bool ABSORB_SUM>
static __global__ __launch_bounds__(SCB_BLOCK) void sumcheck_batch_kernel(SumcheckBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t RL = a.resident_len;
    Fr* tab = reinterpret_cast<Fr*>(zk_dyn_lds);   // K tables of RL entries
    Fr* red = tab + (size_t)K * RL;                // 2 * SCB_BLOCK / 64
    Fr* conv = red + 2 * (SCB_BLOCK / 64);         // K + 2: [sum] [the round's K + 1 values]
    Fr* r_sh = conv + (K + 2);                     // 1
    const uint64_t* src[K];                        // the current tables while they are in global memory
    uint64_t* slab[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        src[k] = a.tables[(size_t)b * K + k];
        slab[k] = a.slab + 4 * ((size_t)b * K + k) * (a.n >> 1);
    }
    uint64_t* out = a.out + (size_t)b * a.out_words;
    uint64_t* out_rp = out + (ABSORB_SUM ? 4 : 0);
    uint32_t n_vars = 0;
    while ((1u << n_vars) < a.n) ++n_vars;
    uint64_t* out_ch = out_rp + 4 * (size_t)n_vars * (K + 1);

    uint32_t cur = a.n, round = 0;
    bool resident = cur <= RL;
    if (resident) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            for (uint32_t j = tid; j < cur; j += nt) tab[k * RL + j] = load_fr(src[k], j);
        __syncthreads();
    }
    Transcript tr;
    tr.init();                                     // (only wave 0's copy is ever used)
    while (cur > 1) {
        const uint32_t half = cur >> 1;
        Fr acc[K + 1];
#pragma unroll
        for (int t = 0; t <= K; ++t) acc[t] = Fr::zero();
        for (uint32_t j = tid; j < half; j += nt) {
            Fr lo[K], hi[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (resident) { lo[k] = tab[k * RL + j]; hi[k] = tab[k * RL + j + half]; }
                else { lo[k] = load_fr(src[k], j); hi[k] = load_fr(src[k], (size_t)j + half); }
            }
            scb_accumulate<K>(acc, lo, hi);
        }
        // K + 1 block sums, two at a time; valid in thread 0
#pragma unroll
        for (int t = 0; t + 1 <= K; t += 2) block_reduce_fr2(acc[t], acc[t + 1], red);
        if ((K + 1) & 1) acc[K] = block_reduce_fr(acc[K], red);
        if (tid == 0) {
#pragma unroll
            for (int t = 0; t <= K; ++t) conv[1 + t] = acc[t];
            if (ABSORB_SUM && round == 0) conv[0] = a.claimed ? load_fr(a.claimed, b) : acc[0] + acc[1];
        }
        __syncthreads();
        if (tid < 64) {   // wave 0, uniform: close the round as transcript_round does
            const bool with_sum = ABSORB_SUM && round == 0;
            // the values leave Montgomery form side by side in lanes 0 .. K + 1: one product's latency for all of them
            const Fr mine = conv[tid < (uint32_t)(K + 2) ? tid : (uint32_t)(K + 1)];
            const Fr canon = fr_from_mont_outlined(mine);
            if (with_sum) tr.commit_canonical(shfl_fr(canon, 0));
#pragma unroll
            for (int t = 0; t <= K; ++t) tr.commit_canonical(shfl_fr(canon, 1 + t));
            // challenge_fr by the whole wave (the schedule on sixteen lanes, the state rounds on six); its 64 words of scratch are the
            // reduction's slots, idle until the next round
            static_assert(2 * (SCB_BLOCK / 64) * sizeof(Fr) >= 64 * sizeof(uint32_t), "challenge_fr_wave's scratch");
            const Fr r = tr.challenge_fr_wave(reinterpret_cast<uint32_t*>(red));
            if (tid == 0) {
                *r_sh = r;
                if (with_sum) store_fr(out, 0, conv[0]);
#pragma unroll
                for (int t = 0; t <= K; ++t) store_fr(out_rp, (size_t)round * (K + 1) + t, conv[1 + t]);
                store_fr(out_ch, round, r);
            }
        }
        __syncthreads();
        const Fr r = *r_sh;
        if (resident) {
            // in place: lane j reads (j, j + half) and writes j; no other lane touches index j this round
            for (uint32_t j = tid; j < half; j += nt) {
#pragma unroll
                for (int k = 0; k < K; ++k) tab[k * RL + j] = fold_pair(tab[k * RL + j], tab[k * RL + j + half], r);
            }
        } else {
            // from the caller's tables (first round) or the slab, into the slab -- in place there, by the same rule -- or, the first
            // time the folded half fits, into LDS
            const bool fits = half <= RL;
            for (uint32_t j = tid; j < half; j += nt) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const Fr v = fold_pair(load_fr(src[k], j), load_fr(src[k], (size_t)j + half), r);
                    if (fits) tab[k * RL + j] = v; else store_fr(slab[k], j, v);
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) src[k] = slab[k];
            resident = fits;
        }
        __syncthreads();   // (LDS and, within the workgroup, the slab: what a lane stored is what the next round's lanes read)
        cur = half;
        ++round;
    }
}

}  // namespace zk
