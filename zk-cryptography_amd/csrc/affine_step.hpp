// affine_step.hpp -- (t + d * D) mod r on the lanes of a row, from a table of digit multiples of D (gfx950).
//
// The serial prover kernel closes every round with lo' = t[4] + c * (t[6] - t[4]): a Montgomery product whose one operand, the
// challenge c, is the digest that has just appeared, and whose other operand D has been known for most of the round.  A lone wave pays
// per instruction, so everything that depends on D alone is done ahead by lanes with time to spare:
//     T_k = D * 2^(28 k) mod r, canonical, k = 0 .. 9                                      (affine_table_store)
// and what is left behind the digest d (the RAW 256 bits, not reduced: d = sum_k d_k 2^(28 k), ten digits of 28 bits) is
//     S = t + sum_k d_k T_k  ==  t + d * D  (mod r),
// one limb per lane: lane j < 8 of a row of 16 accumulates col_j = t[j] + sum_k d_k T_k[j] with ten v_mad_u64_u32 and no carries
// (col_j < 2^32 + 10 * 2^60 < 2^64), then the row reduces S = sum_j col_j 2^(32 j) by ONE quotient word:
//     S < r (1 + sum_k d_k) <= r (1 + 9 (2^28 - 1) + 15) < 2^31.18 r < 2^286.04, so q = floor(S / r) < 2^31.18;
//     top' = col_7 + floor(col_6 / 2^32) lies in (S / 2^224 - 2.001, S / 2^224];
//     q^ = floor(top' * MU / 2^64) with MU = floor(2^288 / r) (34 bits) lies in (S / r - 0.26, S / r], so q - 1 <= q^ <= q;
//     R = S - q^ r = (S + q^ (2^256 - r)) mod 2^256 < 2 r < 2^256: one multiply-add per lane on top of the column's low word, the high
//     words handed one lane up twice (after the columns, after the multiply-add), the carries that are left resolved by a
//     generate / propagate pair of ballots and one 64-bit scalar addition instead of a ripple;
//     one conditional subtraction of r makes R canonical; a second one is kept as margin (it never subtracts while the bounds above hold).
// The result equals from_mont-free arithmetic on canonical integers: t + mont(c, to_mont(D)) with c = d mod r, bit for bit.
// Rows are independent (every mask below is taken per row of 16), so a wave can take up to four triples side by side.
#pragma once
#include "fp.hpp"

namespace zk {

constexpr int AFF_DIGITS = 10;            // digits of the digest
constexpr int AFF_DIGIT_BITS = 28;
constexpr int AFF_LANE_WORDS = 12;        // a lane's ten table words, padded to three 16-byte loads' worth (48 bytes)
constexpr int AFF_TABLE_WORDS = 8 * AFF_LANE_WORDS;   // one table in LDS: word AFF_LANE_WORDS * j + k = T_k[j]

// Rows 0 .. 9: 2^(28 k) in Montgomery form (2^(28 k) * 2^256 mod r): mont(D, .) = D * 2^(28 k), canonical for canonical D.
// Rows 10 .. 19: 2^(28 k) * 2^512 mod r: mont(D, .) = to_mont(D * 2^(28 k)).
static __constant__ uint32_t AFF_POW_MONT[2 * AFF_DIGITS][8] = {
    {0xfffffffeu, 0x00000001u, 0x00034802u, 0x5884b7fau, 0xecbc4ff5u, 0x998c4fefu, 0xacc5056fu, 0x1824b159u},
    {0xdcaaf6b2u, 0x2355094du, 0xa699014eu, 0xf375260du, 0xebe0430au, 0x87cb91f0u, 0x50a25f75u, 0x6567bec7u},
    {0x120121c9u, 0xebc98da2u, 0x14c66acbu, 0x8676d066u, 0xa9939320u, 0x2382db8fu, 0xdcc56ed3u, 0x3840cb63u},
    {0x883c74a3u, 0x28e39d79u, 0x9724b837u, 0xfa113d52u, 0xf6f815aeu, 0x2fe69ddbu, 0x2995dcb6u, 0x5c2064bbu},
    {0x2348f820u, 0xa53acf2au, 0xc830c1b7u, 0x51e1c8bfu, 0x696029a1u, 0x89b7c93du, 0xb9c07cd0u, 0x40ad8d6fu},
    {0xf712c9b0u, 0xab21c5d1u, 0xb05c2342u, 0xe1e037d0u, 0xc76d0786u, 0x6132d479u, 0x9185dfe8u, 0x1ec1c051u},
    {0xfbc14b42u, 0x23afe158u, 0x0f78891bu, 0xc839f2f1u, 0x1582b229u, 0x7989f729u, 0x6ed01e4au, 0x22452ae9u},
    {0x1b4528ecu, 0x9476ebc8u, 0x3fd2a529u, 0x0b3a3b18u, 0xe6447717u, 0xe6670373u, 0xfbd11361u, 0x11c2650fu},
    {0xbd8c85feu, 0x8427cc90u, 0x0fe630beu, 0xc8ff7852u, 0x27715045u, 0x2b4d2b66u, 0xe5a19691u, 0x05753400u},
    {0xdf3f29c7u, 0x0c999e98u, 0x4878d702u, 0xf26a5d9du, 0xe8f39c19u, 0x99f809cau, 0x31c3276eu, 0x16311cfdu},
    {0xf3f29c6du, 0xc999e990u, 0x87925c23u, 0x2b6cedcbu, 0x7254398fu, 0x05d31496u, 0x9f59ff11u, 0x0748d9d9u},
    {0xcefe9ec4u, 0x10408b02u, 0x81216fd5u, 0x95de93b4u, 0x80951780u, 0x9aa9ea96u, 0xdd800be2u, 0x675f1e93u},
    {0x31bba87bu, 0x3b344171u, 0x7ede9435u, 0x9902f3d6u, 0x5be041a9u, 0x4fe7f137u, 0xcb4a3990u, 0x412524b5u},
    {0xa7024848u, 0x1c19723fu, 0x9e1adbcfu, 0x786af0dbu, 0x53ef6d01u, 0x8a7e6bbeu, 0x754967a5u, 0x30cae084u},
    {0x79440e2cu, 0x012c1658u, 0x513d58f8u, 0xf93e134du, 0xd548296fu, 0x06dfaacdu, 0x6a5a6867u, 0x5f47a474u},
    {0xb2d98e44u, 0x94bab29eu, 0x9fd1a321u, 0x20f825eeu, 0x2653d3dau, 0x3ccfaa71u, 0x1927907cu, 0x2dcde358u},
    {0x39ada2e5u, 0xf17ff5ffu, 0x405e5444u, 0x9571c140u, 0x80d885ccu, 0x4503a7fdu, 0x5759c5d6u, 0x661b97c2u},
    {0x41e84f61u, 0x01b28acdu, 0x3af48bffu, 0xba360e86u, 0xd63f6230u, 0x695b1d64u, 0x1114036du, 0x2d12291au},
    {0x09c78bb7u, 0xda56f93fu, 0x951b60f5u, 0xa1a23219u, 0x95799a1du, 0x0a05d103u, 0x82e9b152u, 0x55500f41u},
    {0x6439b73bu, 0xfc62c180u, 0xb8ceec58u, 0xd6efbb11u, 0x9d157cc1u, 0x1a70b147u, 0xcf278b13u, 0x0e218030u}};
constexpr uint32_t AFF_MU_LO = 0x355094edu;   // floor(2^288 / r) = 2 * 2^32 + AFF_MU_LO
constexpr uint64_t AFF_LIMB_LANES = 0x00FF00FF00FF00FFull;   // lanes 0 .. 7 of every row

// row < 2 * AFF_DIGITS
__device__ __forceinline__ Fr affine_pow_mont(uint32_t k) {
    const uint4* c = reinterpret_cast<const uint4*>(AFF_POW_MONT[k]);
    const uint4 a = c[0], b = c[1];
    Fr r;
    r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
    r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
    return r;
}
// a builder lane's share of a table: T_k = mont(D, pow) with pow = affine_pow_mont(k), D canonical -- or, where D = X + c * Y with
// c known last, T_k = mont(X, affine_pow_mont(k)) + mont(c, mont(Y, affine_pow_mont(AFF_DIGITS + k))), one product behind c
__device__ __forceinline__ void affine_table_store(uint32_t* __restrict__ tbl, uint32_t k, const Fr& tk) {
#pragma unroll
    for (int j = 0; j < 8; ++j) tbl[AFF_LANE_WORDS * j + k] = tk.l[j];
}

// the ten digits of d (little-endian limbs)
__device__ __forceinline__ void affine_digits(const uint32_t (&d)[8], uint32_t (&dg)[AFF_DIGITS]) {
#pragma unroll
    for (int k = 0; k < AFF_DIGITS; ++k) {
        const int w = (AFF_DIGIT_BITS * k) >> 5, s = (AFF_DIGIT_BITS * k) & 31;
        const uint64_t pair = ((uint64_t)(w + 1 < 8 ? d[w + 1] : 0u) << 32) | d[w];
        dg[k] = (uint32_t)(pair >> s) & ((1u << AFF_DIGIT_BITS) - 1);
    }
}

// per-lane constants of the step: this lane's limb of r and of 2^256 - r (both 0 on lanes 8 .. 15 of a row)
struct AffineLane {
    uint32_t p, n;
    __device__ __forceinline__ void init() {
        const uint32_t j = threadIdx.x & 15;
        uint32_t v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v = (j == (uint32_t)i) ? FrParams::p(i) : v;
        p = v;
        n = j == 0 ? 0u - v : j < 8 ? ~v : 0u;   // 2^256 - r = ~r + 1, and r's limb 0 is 1: no carry beyond limb 0
    }
};

template <int CTRL> __device__ __forceinline__ uint32_t aff_dpp0(uint32_t v) {    // lanes without a source read 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// w + (this lane's bit of a mask of carries)
__device__ __forceinline__ uint32_t aff_add_carry(uint32_t w, uint64_t carries) {
    uint32_t r;
    asm("v_addc_co_u32 %0, vcc, 0, %1, %2" : "=v"(r) : "v"(w), "s"(carries) : "vcc");
    return r;
}
// a - b - (this lane's bit of a mask of borrows)
__device__ __forceinline__ uint32_t aff_sub_borrow(uint32_t a, uint32_t b, uint64_t borrows) {
    uint32_t r;
    asm("v_subb_co_u32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(borrows) : "vcc");
    return r;
}
__device__ __forceinline__ uint32_t aff_select(uint64_t lanes, uint32_t if_set, uint32_t if_clear) {
    uint32_t r;
    asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(lanes));
    return r;
}
// The step's result in the order a message block wants (big-endian words): lane i of a row reads lane 15 - i (limb j lands on lane
// 15 - j: words 8 .. 15 of a block) or, within each half row, lane 7 - i (limb j on lane 7 - j: words 0 .. 7).  The two wait states a DPP
// read needs after the write of its source are inside the statement: the source comes out of the statements above.
__device__ __forceinline__ uint32_t aff_row_mirror(uint32_t v) {
    uint32_t r;
    asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_mirror row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v));
    return r;
}
__device__ __forceinline__ uint32_t aff_row_half_mirror(uint32_t v) {
    uint32_t r;
    asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_half_mirror row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v));
    return r;
}
// carries INTO every position of a row from the positions that generate one and those that pass one on (never both): the carries of
// the addition (G | P) + G, read off its sum
__device__ __forceinline__ uint64_t aff_carries(uint64_t gen, uint64_t prop) { return ((gen | prop) + gen) ^ prop; }

// Every lane of the wave calls.  tj: limb j of t on lane j < 8 of a row (ignored elsewhere); tbl: the row's table; dg: the row's
// digits (the same on all its lanes).  Returns limb j of (t + d * D) mod r, canonical, on lane j < 8; lanes 8 .. 15 return junk.
__device__ __forceinline__ uint32_t affine_step_rows(const AffineLane& c, uint32_t tj, const uint32_t* __restrict__ tbl,
                                                     const uint32_t (&dg)[AFF_DIGITS]) {
    constexpr int SHL = 0x100, SHR = 0x110;
    const uint32_t j = threadIdx.x & 15;
    uint32_t tk[AFF_LANE_WORDS];
    uint64_t col = 0;
    if (j < 8) {
        const uint4* q = reinterpret_cast<const uint4*>(tbl + AFF_LANE_WORDS * j);
        const uint4 a = q[0], b = q[1];
        const uint2 e = *reinterpret_cast<const uint2*>(q + 2);
        tk[0] = a.x; tk[1] = a.y; tk[2] = a.z; tk[3] = a.w; tk[4] = b.x; tk[5] = b.y; tk[6] = b.z; tk[7] = b.w; tk[8] = e.x; tk[9] = e.y;
        col = tj;
#pragma unroll
        for (int k = 0; k < AFF_DIGITS; ++k) col += (uint64_t)dg[k] * tk[k];
    }
    const uint32_t clo = (uint32_t)col, chi = (uint32_t)(col >> 32);
    const uint32_t hprev = aff_dpp0<SHR + 1>(chi);                   // the high word of the column one lane down
    // lane 7: the quotient word from the top of S (the other lanes compute along on their own columns)
    const uint64_t top = col + hprev;
    const uint64_t a96 = (uint64_t)(uint32_t)(top >> 32) * AFF_MU_LO + (((uint64_t)(uint32_t)top * AFF_MU_LO) >> 32);
    uint32_t q = (uint32_t)((a96 + 2 * top) >> 32);                  // floor(top * MU / 2^64): top < 2^62.04, no overflow
    q = j == 7 ? q : 0u;
    q |= aff_dpp0<SHL + 1>(q);                                       // lane 7 -> lanes 6, 7 -> 4 .. 7 -> 0 .. 7
    q |= aff_dpp0<SHL + 2>(q);
    q |= aff_dpp0<SHL + 4>(q);
    // S + q (2^256 - r): position j holds lo(col_j) + q n_j + hi(col_(j-1)) < 2^63.3; its high word goes one lane up again
    const uint64_t g = (uint64_t)q * c.n + clo + hprev;
    const uint32_t gprev = aff_dpp0<SHR + 1>((uint32_t)(g >> 32));
    const uint32_t w = (uint32_t)g + gprev;
    const uint64_t gen = __builtin_amdgcn_ballot_w64(w < gprev);
    const uint64_t prop = __builtin_amdgcn_ballot_w64(w == 0xFFFFFFFFu) & AFF_LIMB_LANES;
    uint32_t r = aff_add_carry(w, aff_carries(gen, prop));           // limbs 0 .. 7: R = S - q r (position 8 holds q: dropped)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const uint64_t lt = __builtin_amdgcn_ballot_w64(r < c.p) & AFF_LIMB_LANES;
        const uint64_t eq = __builtin_amdgcn_ballot_w64(r == c.p) & AFF_LIMB_LANES;
        const uint64_t bor = aff_carries(lt, eq);                    // borrows into every position of R - r
        const uint64_t below = (bor >> 8) & 0x0001000100010001ull;   // the borrow out of limb 7: R < r, per row
        r = aff_select((below << 8) - below, r, aff_sub_borrow(r, c.p, bor));
    }
    return r;
}

}  // namespace zk
