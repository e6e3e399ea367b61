// multifold_kernels.hpp -- the basic sumcheck prover restructured around k-variable folds (gfx950).
//
// Same observable behaviour as Sumcheck::prove (sumcheck/src/sumcheck.rs:29-61): identical sum, round
// polynomials and challenges.  The restructuring uses two exact identities of the multilinear fold
// (polynomial/src/multilinear/evaluation_form.rs:123-141) when variable 0 (the most significant index bit) is
// folded first, as every sumcheck round does (sumcheck.rs:50):
//   (1) block sums commute with the fold: if B[b] = sum_j T[b*m + j] (2^k blocks of m entries), then the block
//       sums of fold(T, r) are fold(B, r).  The round polynomial (lower-half sum, upper-half sum) of each of the
//       next k rounds is therefore the round polynomial of the 2^k-entry table B: k rounds of transcript run on
//       B alone, inside one workgroup, BEFORE the big table is touched again;
//   (2) k folds collapse into one pass: T_k[j] = sum_b eq_b(r_1..r_k) T[b*m + j], eq_b = prod_i (b_i ? r_i : 1-r_i).
// A 2^24-entry prover thus streams the table twice (block sums, then one 8-variable fold that also emits the
// block sums of its output) instead of ~5.3 times, and issues ~8 kernels instead of ~30.
// Field arithmetic is exact, so the values equal the round-by-round ones bit for bit.
//
// The k-variable fold accumulates sum_b w_b * T_b as an unreduced 17-limb integer (15 column accumulators of
// 96 bits: 64 mads + 64 carry adds per term, half of a Montgomery product) and reduces once per output with
// a 9-word REDC; the weights carry an extra factor 2^32 that the ninth word removes.
#pragma once
#include "sumcheck_kernels.hpp"
#include "wide_acc.hpp"
#include "affine_step.hpp"

namespace zk {

constexpr int MF_MAX_LOGK = 8;   // variables per fold in the single-GPU plan
constexpr int MF_CAP_LOGK = 9;   // what the kernels can take; the sharded plan uses 9 where it saves an exchange (2^27 over 8 GPUs)

// per-workgroup sum of a contiguous chunk of `chunk` entries (chunk a power of two, >= MLE_BLOCK)
static __global__ __launch_bounds__(MLE_BLOCK) void chunk_sums_kernel(const uint64_t* __restrict__ in, uint32_t chunk,
                                                                      uint64_t* __restrict__ partials) {
    __shared__ Fr red[MLE_BLOCK / 64];
    const uint64_t* base = in + 4 * (size_t)blockIdx.x * chunk;
    Fr s = Fr::zero();
    for (uint32_t j = threadIdx.x; j < chunk; j += 4 * MLE_BLOCK) {
        Fr v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (j + u * MLE_BLOCK < chunk) ? load_fr(base, j + u * MLE_BLOCK) : Fr::zero();
#pragma unroll
        for (int u = 0; u < 4; ++u) s = s + v[u];
    }
    s = block_reduce_fr(s, red);
    if (threadIdx.x == 0) store_fr(partials, blockIdx.x, s);
}

// out[b] = sum of the group-th consecutive partials, b < n_blocks; out[n_blocks] = total
static __global__ __launch_bounds__(MLE_BLOCK) void group_sums_kernel(const uint64_t* __restrict__ partials, uint32_t group,
                                                                      uint32_t n_blocks, uint64_t* __restrict__ out) {
    __shared__ Fr red[MLE_BLOCK / 64];
    Fr tot = Fr::zero();
    for (uint32_t b = threadIdx.x; b < n_blocks; b += MLE_BLOCK) {
        Fr s = Fr::zero();
        for (uint32_t g = 0; g < group; ++g) s = s + load_fr(partials, (size_t)b * group + g);
        store_fr(out, b, s);
        tot = tot + s;
    }
    tot = block_reduce_fr(tot, red);
    if (threadIdx.x == 0) store_fr(out, n_blocks, tot);
}

// ---- fine block sums for the overlapped plan -------------------------------------------------------------
// sums[c] = sum of the c-th run of FINE_CHUNK consecutive entries.  A wave owns two adjacent runs (8 loads of 2 KiB in flight per
// wave); no loop, the grid covers the table (n / (8 FINE_CHUNK) workgroups).
// Probes (tools/ubench_fine.hip and in-situ A/Bs, 2^24 entries, same box; profiles/r04/NOTES.md): the loads alone take
// 82.2-82.5 us non-temporal, 85.9 plain; this kernel 90.3-91.0.  Its two runs half a table apart + non-temporal loads: 87.1-87.7 in
// isolation, but in the prover the k-variable fold behind it then ran 95 instead of 84 us (it had been finding the tail of THIS pass in
// the 256 MiB Infinity Cache) and the step did not move.  Four runs per wave, waves permuted by strides of 2^3..2^12 runs: 88-96 us.
// Successive passes in alternating directions (each starting in the half the previous one left in that cache): step 0.3277 / 0.3307
// against 0.3297 / 0.3321 ms -- inside the noise.  All dropped.  The ceiling of a read-only stream on this part is the same from
// anywhere: a table that FITS the Infinity Cache (64 / 128 / 256 MiB swept twice) is read at 6.4-7.2 TB/s.
constexpr int FINE_CHUNK = 256;
static __global__ __launch_bounds__(MLE_BLOCK) void fine_sums_kernel(const uint64_t* __restrict__ in, size_t n_chunks,
                                                                     uint64_t* __restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t c0 = ((size_t)blockIdx.x * (MLE_BLOCK / 64) + wave) * 2;
    if (c0 >= n_chunks) return;
    const bool two = c0 + 1 < n_chunks;
    const uint64_t* base = in + 4 * (c0 * FINE_CHUNK);
    Fr v[8];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = load_fr(base, lane + 64 * u);
#pragma unroll
    for (int u = 4; u < 8; ++u) v[u] = two ? load_fr(base, lane + 64 * u) : Fr::zero();
    Fr a = (v[0] + v[1]) + (v[2] + v[3]);
    Fr b = (v[4] + v[5]) + (v[6] + v[7]);
    wave_reduce_fr2(a, b);              // DPP / permlane moves: no LDS traffic beside the loads
    if (lane == 0) {
        store_fr(sums, c0, a);
        if (two) store_fr(sums, c0 + 1, b);
    }
}

// One workgroup per output b: the sum of in[b*group .. (b+1)*group) (the coarse block sums from the fine ones), written as
// a Montgomery residue to out_mont[b] and / or as a canonical integer -- what the serial kernel's sum tree holds -- to
// out_canon[b] (either may be null)
static __global__ __launch_bounds__(MLE_BLOCK) void group_sums_wg_kernel(const uint64_t* __restrict__ in, uint32_t group,
                                                                         uint64_t* __restrict__ out_mont, uint64_t* __restrict__ out_canon) {
    __shared__ Fr red[MLE_BLOCK / 64];
    const uint64_t* base = in + 4 * (size_t)blockIdx.x * group;
    Fr s = Fr::zero();
    for (uint32_t j = threadIdx.x; j < group; j += 4 * MLE_BLOCK) {
        Fr v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (j + u * MLE_BLOCK < group) ? load_fr(base, j + u * MLE_BLOCK) : Fr::zero();
#pragma unroll
        for (int u = 0; u < 4; ++u) s = s + v[u];
    }
    s = block_reduce_fr(s, red);
    if (threadIdx.x == 0) {
        if (out_mont) store_fr(out_mont, blockIdx.x, s);
        if (out_canon) store_fr(out_canon, blockIdx.x, fr_from_mont_outlined(s));
    }
}

constexpr int TREE_MAX_LOG = 10;   // the serial kernel keeps tables of up to 2^10 entries (and their sum trees) in LDS

struct SmallArgs {
    const uint64_t* src;    // mode 0: the table itself (2^log_n entries); mode 1: partial sums, `group` per entry
    uint32_t group;         // mode 1: partials per table entry (0 = mode 0)
    uint32_t stride;        // mode 1: 0 = entry j owns partials j*group .. +group; else partial g of entry j is src[g*stride + j]
    uint32_t canon;         // the source values are canonical integers already (blockfold_kernel / group_sums_wg_kernel<true>)
    uint32_t log_n;         // working table has 2^log_n entries (<= 2^TREE_MAX_LOG)
    uint32_t n_rounds;      // rounds to run, <= log_n
    uint32_t round0;        // index of the first round run here
    uint32_t first;         // 0 continue; 1 start the transcript, sum = lo + hi; 2 sum = claimed; 3 sum = *d_claimed
    FrArg claimed;
    const uint64_t* d_claimed;
    uint64_t* weights_out;  // nullable: 2^n_rounds fold weights eq_b(r) * 2^32 (Montgomery form)
    uint64_t* final_out;    // nullable: the table left after n_rounds folds
    // The LAST kernel of a proof delivers it: host_delta != 0 is the distance (in u64) from the device span [state .. round polynomials] to
    // its pinned host mirror -- the rounds of earlier kernels are copied there by the output wave, this kernel's own outputs are stored
    // twice -- so no hipMemcpyAsync (8 us with its launch gap) follows the last round.
    long long host_delta;
    // ... and says so: once everything the host reads from the mirror has been stored, `seq` goes into the pinned word `seq_word` (a
    // system-scope release), ahead of the epilogue, the end-of-kernel write-back and the completion event.  The host spins on the word
    // and falls back to the event (sumcheck_collect).  Null for launches that deliver nothing (and for the sharded prover's).
    uint64_t seq;
    uint64_t* seq_word;
};

constexpr int SMALL_BLOCK = 512;   // 8 waves: the transcript wave, two schedule waves, five waves for the trees and weights

// n_rounds sumcheck rounds (half sums -> transcript -> challenge -> fold, sumcheck.rs:40-51) of a small table.
//
// The table sits in LDS together with its SUM TREE (node q = 2^l + b holds the sum of block b when the table is
// cut into 2^l blocks; the leaves are the table).  Folding the table at variable 0 folds every level the same way:
//     new[q] = old[q + p] + r * (old[q + 2p] - old[q + p]),  p = largest power of two <= q,
// so after a fold the next round polynomial (lo, hi) = new[2], new[3] is available WITHOUT a reduction, and every
// node is independent work.
// The tree is kept in CANONICAL (non-Montgomery) form: the transcript absorbs canonical bytes, so (lo, hi) need no
// conversion, and a product of a Montgomery-form challenge with a canonical difference is again canonical.
// Wave 0 runs nothing but the transcript chain plus the round's closing step lo' = t[4] + c * (t[6] - t[4]).  That step is no
// Montgomery product any more: twenty lanes of the last helper wave have spent the round on a table of the digit multiples
// (t[6] - t[4]) * 2^(28 k), and behind the digest one limb per lane is ten multiply-adds, one quotient word and a carry resolved by
// ballots (affine_step.hpp); the digest is published raw, and whoever needs the challenge as a field element reduces it for itself.
// The table's operand is itself one challenge old: D = X + c Y with X, Y from level 3 of the old tree, so the builders need two
// products behind the barrier and none of them waits for a conversion of c.  Waves 1 and 2 take the same step for their copies
// of lo' / hi' and prepare the message schedules of the next round's two SHA-256 blocks and nothing else (with tree work on top
// they were the last to reach the barrier); waves 3, 5, 6, 7 fold the tree and the k-variable fold weights; wave 4 writes the
// outputs (Montgomery form; three conversions on three lanes).  The first round of a launch has no table and multiplies by
// E = to_mont(t[6] - t[4]) from the prologue.  One barrier per round; the trees, the tables and the digest slot are double-buffered.
// (Stamps of a 2^24 prove, tools/diag_small.py, measured: a steady round = 1.50 + 1.46 us of state rounds + 0.53 us for the step
// (was 0.94 for the product) + 0.23 us to publish and pass the barrier = 3.87 us, was 4.53; profiles/serial_rounds/NOTES.md.)
static __global__ __launch_bounds__(SMALL_BLOCK) void sumcheck_small_kernel(SmallArgs a, SumcheckDev* st,
                                                                            uint64_t* __restrict__ round_polys,
                                                                            uint64_t* __restrict__ challenges) {
#include "sumcheck_small_body.hpp"
}
// dynamic LDS of the kernel above: trees (3 x 2^log_n), weights (1.5 x 2^weight_rounds; weight_rounds < 0: none), the
// grouped mode's scratch, the small shared slots, the four tables of digit multiples and their builders' exchange
__host__ __device__ constexpr size_t small_lds_bytes(uint32_t log_n, int weight_rounds, bool grouped) {
    return ((size_t)3 * ((size_t)1 << log_n) + (weight_rounds >= 0 ? 3 * ((size_t)1 << weight_rounds) / 2 : 0u) + 1 +
            (grouped ? SMALL_BLOCK : 0) + 2 + 2 * AFF_DIGITS) * 32 + (64 + 64 + 16 + 4 + 4 * AFF_TABLE_WORDS) * 4;
}

// Fold weights of k known points (MultilinearTrait::evaluation folds variable 0 repeatedly, evaluation_form.rs:162-175):
// w[b] = 2^32 * prod_i (b_i ? r_i : 1 - r_i), b_1 = most significant bit of b.  One lane per weight.
static __global__ __launch_bounds__(MLE_BLOCK) void eq_weights_kernel(PtsArg pts, uint32_t first, uint32_t k,
                                                                      uint64_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * MLE_BLOCK + threadIdx.x;
    if (b >= (1u << k)) return;
    Fr w;
    constexpr uint32_t c[8] = {0xcaaf6b13u, 0x355094eau, 0x69a568efu, 0xf6b10cb3u, 0x40cc3869u, 0xe2c926a6u, 0xed269aadu, 0x736a6d3bu};
#pragma unroll
    for (int i = 0; i < 8; ++i) w.l[i] = c[i];
    const Fr one = Fr::one();
    for (uint32_t i = 0; i < k; ++i) {
        Fr r = fr_from_pts(pts, first + i);
        if (!((b >> (k - 1 - i)) & 1)) r = one - r;
        w = w * r;
    }
    store_fr(out, b, w);
}

// The weight tables of an evaluation in one pass (zkhip_mle_evaluation), one lane per entry:
//   w1[b], b < 2^k1       the fold weights of the first k1 points (with the factor 2^32, as above);
//   wa[x], x < 2^(k2 - s) and wb[y], y < 2^s: the plain eq tables (Montgomery form, no factor) of the next k2 - s and the last s
//   points -- the eq table of all k2 remaining points is their outer product, eq[x * 2^s + y] = wa[x] * wb[y], formed where it is
//   used (one product per output): at most max(k1, k2 - s, s) products one after another here instead of k2.
static __global__ __launch_bounds__(MLE_BLOCK) void eval_weights_kernel(PtsArg pts, uint32_t k1, uint32_t k2, uint32_t s, uint64_t* __restrict__ w1,
                                                                        uint64_t* __restrict__ wa, uint64_t* __restrict__ wb) {
    size_t b = (size_t)blockIdx.x * MLE_BLOCK + threadIdx.x;
    const size_t n1 = (size_t)1 << k1, na = (size_t)1 << (k2 - s), nb = (size_t)1 << s;
    uint32_t k, first;
    uint64_t* out;
    Fr w = Fr::one();
    if (b < n1) {
        k = k1; first = 0; out = w1;
        constexpr uint32_t c[8] = {0xcaaf6b13u, 0x355094eau, 0x69a568efu, 0xf6b10cb3u, 0x40cc3869u, 0xe2c926a6u, 0xed269aadu, 0x736a6d3bu};
#pragma unroll
        for (int i = 0; i < 8; ++i) w.l[i] = c[i];
    } else if (b < n1 + na) {
        b -= n1; k = k2 - s; first = k1; out = wa;
    } else if (b < n1 + na + nb) {
        b -= n1 + na; k = s; first = k1 + k2 - s; out = wb;
    } else {
        return;
    }
    const Fr one = Fr::one();
    for (uint32_t i = 0; i < k; ++i) {
        Fr r = fr_from_pts(pts, first + i);
        if (!((b >> (k - 1 - i)) & 1)) r = one - r;
        w = w * r;
    }
    store_fr(out, b, w);
}
// out[0] = sum of n records (the tiles' shares of an evaluation)
static __global__ __launch_bounds__(MLE_BLOCK) void sum_records_kernel(const uint64_t* __restrict__ records, uint32_t n, uint64_t* __restrict__ out) {
    __shared__ Fr red[MLE_BLOCK / 64];
    Fr s = Fr::zero();
    for (uint32_t i = threadIdx.x; i < n; i += 4 * MLE_BLOCK) {
        Fr v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (i + u * MLE_BLOCK < n) ? load_fr(records, i + u * MLE_BLOCK) : Fr::zero();
#pragma unroll
        for (int u = 0; u < 4; ++u) s = s + v[u];
    }
    s = block_reduce_fr(s, red);
    if (threadIdx.x == 0) store_fr(out, 0, s);
}

// ---- the k-variable fold -------------------------------------------------------------------------------
// out[j] = sum_{b < 2^k} w[b] * in[b*m + j], j < m.
// A wave covers G consecutive outputs x (64/G) term groups; a workgroup's S = blockDim/64 waves split the 2^k terms
// further, so one output is shared by S * 64/G lanes.  Every lane reduces its own unreduced partial sum (the
// weights' 2^32 factor makes each 9-word REDC a proper Montgomery residue, so partial results simply add); the
// groups of a wave combine by shuffles, the waves through LDS.  G = 64 streams big tables (2 KiB per wave-load);
// G = 16 keeps the chip busy when only a few hundred outputs are left.
// Also writes the workgroup's sum of outputs to partials[blockIdx.x] (block sums of the output table).
template <int G, int DEPTH = 4, bool NT = false>
static __global__ __launch_bounds__(1024) void multifold_kernel(const uint64_t* __restrict__ in, size_t m, uint32_t k,
                                                                const uint64_t* __restrict__ weights,
                                                                uint64_t* __restrict__ out,
                                                                uint64_t* __restrict__ partials) {
    constexpr int TG = 64 / G;                                // term groups inside a wave
    // dynamic LDS: 2^k weights, then the (waves - 1) x G partial outputs -- (32 << k) + 32 (waves - 1) G bytes.  LDS decides
    // how many workgroups share a CU, so it is sized exactly (a fixed 16 KiB for the weights cost the streaming fold 30 %).
    extern __shared__ __attribute__((aligned(16))) unsigned char zk_dyn_lds[];
    Fr* w_lds = reinterpret_cast<Fr*>(zk_dyn_lds);
    Fr* part = w_lds + (1u << k);
    const uint32_t n_terms = 1u << k;
    for (uint32_t b = threadIdx.x; b < n_terms; b += blockDim.x) w_lds[b] = load_fr(weights, b);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t n_waves = blockDim.x >> 6;
    const uint32_t slice = wave * TG + lane / G;              // term slice of this lane
    const uint32_t per = n_terms / (n_waves * TG);            // host guarantees >= 1
    const uint32_t oj = lane % G;
    const size_t j = (size_t)blockIdx.x * G + oj;
    WideAcc acc;
    acc.clear();
    const uint32_t b0 = slice * per;
    const uint64_t* p = in + 4 * ((size_t)b0 * m + j);
    const size_t row = 4 * m;
    for (uint32_t t = 0; t < per; t += DEPTH) {
        Fr v[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) if (t + u < per) v[u] = NT ? load_fr_nt(p + (size_t)(t + u) * row) : load_fr(p + (size_t)(t + u) * row, 0);
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) if (t + u < per) acc.mac(w_lds[b0 + t + u], v[u]);
    }
    Fr o = wide_reduce(acc.lo, acc.hi);
#pragma unroll
    for (int d = 32; d >= G; d >>= 1) o = o + shfl_down_fr(o, d);   // lanes < G now hold the wave's sums
    if (wave != 0 && lane < G) part[(wave - 1) * G + lane] = o;
    __syncthreads();
    if (wave == 0) {
        if (lane < G) {
            for (uint32_t w2 = 1; w2 < n_waves; ++w2) o = o + part[(w2 - 1) * G + lane];
            store_fr(out, j, o);
        } else {
            o = Fr::zero();
        }
        Fr s = wave_reduce_fr(o);
        if (lane == 0) store_fr(partials, blockIdx.x, s);
    }
}

// out[j] = to_mont(sum_y in[y*m + j]): the partial tables of blockfold_kernel added up and brought back to Montgomery form
// (the sharded prover's local 256-entry table before it is gathered)
static __global__ __launch_bounds__(MLE_BLOCK) void slice_sums_kernel(const uint64_t* __restrict__ in, uint32_t ny, uint32_t m,
                                                               uint64_t* __restrict__ out) {
    const uint32_t j = blockIdx.x * MLE_BLOCK + threadIdx.x;
    if (j >= m) return;
    Fr s = load_fr(in, j);
    for (uint32_t y = 1; y < ny; ++y) s = s + load_fr(in, (size_t)y * m + j);
    store_fr(out, j, fr_to_mont_outlined(s));
}

// ---- k-variable fold of a SMALL table (<= 2^18 entries), spread over the chip -----------------------------------------
// partial[y*m + c] = sum over the term range y of w[b] * in[b*m + c], as CANONICAL integers (the serial kernel's form; the
// conversion is linear, so partial tables still add up).  multifold_kernel<16> gives such a table to m/16 workgroups (16 at
// m = 256: ~16 us of one-wave-per-SIMD latency).  Here a workgroup is 256 lanes, ONE wave per SIMD: the products are
// chains of multiply-adds with 64-way instruction parallelism, so a wave alone on its SIMD issues back to back, and the
// grid is sized to reach all 256 CUs (with 1024 lanes -- four waves per SIMD -- on 32 or 64 CUs its instruction count alone
// accounts for the 11-14 us it took; the count and what is measured: profiles/blockfold/NOTES.md).  A workgroup takes 8 consecutive outputs x up to
// 32 term slices of <= 4 terms each; a wave is 8 outputs x 8 slices, summed by three shuffle levels, and the four waves
// combine through LDS behind ONE barrier.  The term ranges go to blockIdx.y; the serial kernel adds the gridDim.y (<= 8)
// partial tables (SmallArgs::stride).
constexpr int BF_BLOCK = 256;
constexpr int BF_LOG_OW = 3;                               // outputs per workgroup: 8 (one 256-byte run per slice and term)
constexpr int BF_SLICES = BF_BLOCK >> BF_LOG_OW;           // term slices per workgroup: 32
constexpr int BF_MAX_PER = 4;                              // terms per lane: WideAcc's capacity as pinned in tests/test_gpu_arith.py
constexpr int BF_MAX_NY = 8;                               // partial tables: the serial kernel's strided prologue keeps 8 loads in flight
constexpr int BF_TARGET_WGS = 256;                         // workgroups to aim for when the terms allow it: one per CU

// The grid and the split of the 2^k terms for a fold to m outputs: m / 8 workgroups x ny term ranges; in a range, `sl` (<= 32)
// slices of `per` (<= 4) consecutive terms, so sl * per * ny = 2^k.  ny is what fills the chip (BF_TARGET_WGS) or what
// per <= 4 forces, whichever is larger, and at most 8: ny * m <= 2048 for m <= 1024, the room of the prover's first partial
// tables.  A table too small for that leaves slices idle (sl < 32) rather than CUs.  The one rule for the library, the
// sharded stage's buffer sizes and the test driver.
struct BlockfoldShape { uint32_t log_ow, sl, per, ny; };
__host__ __device__ constexpr bool blockfold_shape(uint32_t m, uint32_t k, BlockfoldShape* sh) {
    if (m == 0 || (m & (m - 1)) != 0 || (m >> BF_LOG_OW) == 0) return false;       // a power of two, at least one workgroup's outputs
    if (k == 0 || k > 10) return false;                                              // 2^10 terms = 32 slices x 4 terms x 8 ranges
    const uint32_t terms = 1u << k, wgx = m >> BF_LOG_OW;
    const uint32_t fill = wgx >= (uint32_t)BF_TARGET_WGS ? 1u : (uint32_t)BF_TARGET_WGS / wgx;
    const uint32_t forced = (terms + BF_SLICES * BF_MAX_PER - 1) / (BF_SLICES * BF_MAX_PER);
    uint32_t ny = fill > forced ? fill : forced;
    if (ny > (uint32_t)BF_MAX_NY) ny = BF_MAX_NY;
    if (ny > terms) ny = terms;
    const uint32_t range = terms / ny;                                               // terms of one workgroup
    sh->log_ow = BF_LOG_OW;
    sh->sl = range < (uint32_t)BF_SLICES ? range : (uint32_t)BF_SLICES;
    sh->per = range / sh->sl;
    sh->ny = ny;
    return true;
}

// grid (m >> BF_LOG_OW, ny), BF_BLOCK lanes; sl, per, ny from blockfold_shape
static __global__ __launch_bounds__(BF_BLOCK) void blockfold_kernel(const uint64_t* __restrict__ in, uint32_t m, uint32_t sl_cnt,
                                                                    uint32_t per, const uint64_t* __restrict__ weights,
                                                                    uint64_t* __restrict__ partial) {
    constexpr uint32_t OW = 1u << BF_LOG_OW, WAVES = BF_BLOCK / 64;
    __shared__ Fr part[(WAVES - 1) * OW];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t o = lane & (OW - 1), sl = wave * (64 / OW) + (lane >> BF_LOG_OW);
    const uint32_t c = blockIdx.x * OW + o;
    const uint32_t b0 = (blockIdx.y * sl_cnt + sl) * per;
    Fr r = Fr::zero();
    if (sl < sl_cnt) {                                   // a whole number of waves idles, except where sl_cnt < 8
        Fr v[BF_MAX_PER], w[BF_MAX_PER];                 // every load in flight before the first product
#pragma unroll
        for (int u = 0; u < BF_MAX_PER; ++u) {
            if ((uint32_t)u < per) { v[u] = load_fr(in, (size_t)(b0 + u) * m + c); w[u] = load_fr(weights, b0 + u); }
        }
        WideAcc acc;
        acc.clear();
#pragma unroll
        for (int u = 0; u < BF_MAX_PER; ++u) {
            if ((uint32_t)u < per) acc.mac(w[u], v[u]);
        }
        r = wide_reduce(acc.lo, acc.hi);
    }
#pragma unroll
    for (int d = 32; d >= (int)OW; d >>= 1) r = r + shfl_down_fr(r, d);      // lanes < 8: the wave's eight slices added up
    if (wave != 0 && lane < OW) part[(wave - 1) * OW + lane] = r;
    __syncthreads();
    if (wave == 0 && lane < OW) {
#pragma unroll
        for (uint32_t w2 = 1; w2 < WAVES; ++w2) r = r + part[(w2 - 1) * OW + lane];
        store_fr(partial, (size_t)blockIdx.y * m + c, fr_from_mont_outlined(r));
    }
}

}  // namespace zk
