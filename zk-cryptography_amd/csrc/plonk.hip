// plonk.hip -- C-ABI entry points of the PLONK prover and verifier (plonk/src/protocol/{prover,verifier,utils,transcript}.rs,
// transcripts/merlin/src/lib.rs).  gfx950 only; no CPU fallback for the prover.  The wire, selector and permutation polynomials stay on
// the device for the whole call: the nine commitments, six evaluations and one status word cross to the host, where the Merlin
// transcript (SHA-256 of a few hundred bytes per round) derives the challenges between the rounds.
#include "../../include/zkhip.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "host_fr.hpp"
#include "host_g1.hpp"
#include "host_util.hpp"
#include "pairing_internal.hpp"
#include "plonk_batch_kernels.hpp"
#include "plonk_kernels.hpp"
#include "plonk_scalars.hpp"
#include "plonk_transcript.hpp"
#include "plonk_verify_kernels.hpp"
#include "tunables.hpp"

using namespace zk;

namespace {

// Host only, each with a stand-alone sanitizer program under tests/cpp: plonk_scalars.hpp (HFr, h_is_zero, h_neg, h_pow, l1_at and the
// verifier's scalar algebra) and plonk_transcript.hpp (the Merlin transcript, the rounds' schedule PlonkRoundTranscript and the ABI's
// orders P_*, E_*, C_*).
using namespace zkplonk;
using zkhost::fr_add;
using zkhost::fr_mul;
using zkhost::fr_sub;

inline HFr h_load(const uint64_t* p) { HFr r; std::memcpy(r.l, p, 32); return r; }
inline FrArg fa(const HFr& a) { FrArg r; std::memcpy(r.v, a.l, 32); return r; }
inline bool h_eq(const HFr& a, const HFr& b) { return std::memcmp(a.l, b.l, 32) == 0; }

// ---- the key --------------------------------------------------------------------------------------------------------------------
// Coset evaluations of the eight preprocessed columns, of L_1 and of X: ten vectors of D elements.  They are kept with the key up to
// this budget -- at n = 2^20 (D = 2^22) they take 1.25 GiB, less than the 1.6 GiB shifted-SRS table the commits of that size already
// hold -- and recomputed per proof (ten transforms) above it.
static_assert(zk::env::PLONK_CACHE_BUDGET.def == 2LL << 30, "the budget the lines above speak of");
// diagnostic aid (tests/test_gpu_plonk.py): ZKHIP_PLONK_CACHE_BUDGET=<bytes> replaces the budget, 0 makes every key an uncached one.
// Read at each key's creation, not once per process: a key keeps the choice it was made with.
size_t plonk_cache_budget() { return (size_t)zk::env::read(zk::env::PLONK_CACHE_BUDGET); }
constexpr int N_PRE = 10;
const uint64_t COSET_SHIFT = 7;          // arkworks' multiplicative generator of Fr; the quotient does not depend on the choice

}  // namespace

struct zkhip_plonk_key {
    zkhip_ctx* ctx = nullptr;
    size_t n = 0, D = 0, S = 0;          // rows, coset size, stride of a coefficient vector (n + 8: room for the blinding, zero-padded)
    uint32_t log_n = 0, log_D = 0, ratio = 0;
    const uint64_t* srs_xy = nullptr; const void* srs_table = nullptr; const uint8_t* srs_inf = nullptr; size_t n_points = 0;   // views
    DevMem evals, coeffs, omega, gpow, ginv, pre, work;
    DevMem batch_work;                   // zkhip_plonk_prove_batch: the work areas of batch_chunk proofs, allocated by the first batch call
    PinMem batch_pin;
    uint32_t batch_chunk = 0;
    HFr w_n, zh_inv[8];
    uint64_t* col_eval(int k) const { return (uint64_t*)evals.get() + 4 * n * k; }
    uint64_t* col_coeff(int k) const { return (uint64_t*)coeffs.get() + 4 * S * k; }
};

namespace {

// work area of one proof (elements of 32 bytes)
struct Work {
    uint64_t *A, *B, *C, *Z, *PI, *TL, *TM, *TH, *W, *Q1, *Q2, *F, *ACC;   // S each
    uint64_t *ev, *T;                                                       // 5 D, D
    uint64_t *bp, *bx, *hv, *hc, *out;                                      // block products / horner scratch / 8 results
    int* flags;
    uint64_t* pre;                                                          // 10 D when the key holds no cache
    size_t zero_bytes;                                                      // the leading part a proof clears
};
// workgroups of a Horner scan over n coefficients; a job's row of workgroup values (and of carries) in the work area
inline uint32_t horner_blocks(size_t n) { return (uint32_t)((n + (size_t)HS_T * HS_L - 1) / ((size_t)HS_T * HS_L)); }
inline size_t horner_row(const zkhip_plonk_key& k) { return (size_t)horner_blocks(k.S) + 1; }

// ---- the round table ------------------------------------------------------------------------------------------------------------
// What the five rounds commit, transform, evaluate, divide and combine, stated once: zkhip_plonk_prove walks these rows with proof 0's
// pointers, BatchRun::rounds packs the same rows into its kernels' argument structs.  A row's polynomial is a member of the proof's
// work area (`own`) or, where `own` is null, coefficient column `key_col` of the key; its length is n + extra.
struct RoundPoly {
    uint64_t* Work::*own; int key_col; int extra;
    bool at_zeta_w;                                            // Horner jobs: the point is w zeta, not zeta
    uint64_t* Work::*quotient;                                 // divisions: where (p(X) - p(z)) / (X - z) goes
};
constexpr RoundPoly own_poly(uint64_t* Work::*m, int extra, bool at_zeta_w = false, uint64_t* Work::*quotient = nullptr) {
    return {m, -1, extra, at_zeta_w, quotient};
}
constexpr RoundPoly key_poly(int col) { return {nullptr, col, 0, false, nullptr}; }
// the commitments of rounds 1, 2, 3 and 5 (prover.rs:113-123, 167-175, 249-258, 361-376): first point of the proof, count, polynomials
struct CommitRound { int first, m; RoundPoly p[3]; };
constexpr CommitRound COMMIT_WIRES = {P_AS, 3, {own_poly(&Work::A, 2), own_poly(&Work::B, 2), own_poly(&Work::C, 2)}};
constexpr CommitRound COMMIT_ACC = {P_ACC, 1, {own_poly(&Work::Z, 3)}};
constexpr CommitRound COMMIT_T = {P_TL, 3, {own_poly(&Work::TL, 1), own_poly(&Work::TM, 1), own_poly(&Work::TH, 6)}};
constexpr CommitRound COMMIT_OPENINGS = {P_WZ, 2, {own_poly(&Work::Q1, 5), own_poly(&Work::Q2, 2)}};
// round 3: the rows of `ev`, in the order plonk_quotient_kernel reads them
constexpr RoundPoly COSET_INPUTS[PB_COSET_ROWS] = {own_poly(&Work::A, 2), own_poly(&Work::B, 2), own_poly(&Work::C, 2), own_poly(&Work::Z, 3),
                                                   own_poly(&Work::PI, 0)};
// round 4: the six evaluations in the ABI's order E_*, then PI(zeta) for round 5; job j's value is element j of `out`
constexpr RoundPoly EVAL_JOBS[PB_JOBS] = {own_poly(&Work::A, 2), own_poly(&Work::B, 2), own_poly(&Work::C, 2), key_poly(5), key_poly(6),
                                          own_poly(&Work::Z, 3, true),       // apply_w_to_polynomial(z)(zeta) = z(w zeta)
                                          own_poly(&Work::PI, 0)};
// round 5: W_zeta = (r + nu-combination) / (X - zeta), W_zeta_omega = (z - z(w zeta)) / (X - w zeta)
constexpr RoundPoly DIVIDE_JOBS[2] = {own_poly(&Work::W, 6, false, &Work::Q1), own_poly(&Work::Z, 3, true, &Work::Q2)};
// round 5: the vectors of plonk_linearise_kernel's terms, in the order of round5_scalars' weights
constexpr RoundPoly LIN_TERMS[PLONK_LIN_TERMS] = {key_poly(0), key_poly(1), key_poly(2), key_poly(3), key_poly(4), own_poly(&Work::Z, 3), key_poly(7),
                                                  own_poly(&Work::TL, 1), own_poly(&Work::TM, 1), own_poly(&Work::TH, 6), own_poly(&Work::A, 2),
                                                  own_poly(&Work::B, 2), own_poly(&Work::C, 2), key_poly(5), key_poly(6)};
static_assert(EVAL_JOBS[E_ZW].at_zeta_w && EVAL_JOBS[E_S1].key_col == 5 && EVAL_JOBS[E_S2].key_col == 6, "the evaluations in the ABI's order");

uint64_t* poly_at(const zkhip_plonk_key& k, const Work& w, const RoundPoly& r) { return r.own ? w.*r.own : k.col_coeff(r.key_col); }
// bit j set: row j is the proof's own polynomial (the batch kernels move it by the proof's offset), not the key's
template <int N> constexpr uint32_t own_mask(const RoundPoly (&rows)[N]) {
    uint32_t m = 0;
    for (int j = 0; j < N; ++j) m |= (rows[j].own != nullptr ? 1u : 0u) << j;
    return m;
}
// commit, coset and division rows are read as w.*row.own: every one of them must be the proof's own
constexpr bool all_own(const CommitRound& r) {
    for (int j = 0; j < r.m; ++j) if (r.p[j].own == nullptr) return false;
    return true;
}
static_assert(all_own(COMMIT_WIRES) && all_own(COMMIT_ACC) && all_own(COMMIT_T) && all_own(COMMIT_OPENINGS) &&
              own_mask(COSET_INPUTS) == (1u << PB_COSET_ROWS) - 1 && DIVIDE_JOBS[0].quotient != nullptr && DIVIDE_JOBS[1].quotient != nullptr,
              "a commit, a coset input or a division names a member of the work area");
static_assert(own_mask(EVAL_JOBS) == 0x67u && own_mask(DIVIDE_JOBS) == 3u && own_mask(LIN_TERMS) == ((1u << 5) | (0x3fu << 7)),
              "sigma_1 and sigma_2 are the key's among the evaluations; z, the parts of t and the wires are the proof's among the terms");
struct CommitSet { uint64_t* polys[3]; size_t lens[3]; };
CommitSet commit_set(const Work& w, size_t n, const CommitRound& r) {
    CommitSet s = {};
    for (int j = 0; j < r.m; ++j) { s.polys[j] = w.*r.p[j].own; s.lens[j] = n + r.p[j].extra; }
    return s;
}

size_t work_layout(const zkhip_plonk_key& k, char* base, bool with_pre, Work* w) {
    size_t off = 0;
    auto take = [&](size_t elems) { uint64_t* p = (uint64_t*)(base + off); off += (elems * 32 + 255) & ~(size_t)255; return p; };
    const size_t nb = (k.S + GP_ROWS - 1) / GP_ROWS + 1, hb = horner_row(k);
    Work t;
    uint64_t** s[] = {&t.A, &t.B, &t.C, &t.Z, &t.PI, &t.TL, &t.TM, &t.TH, &t.W, &t.Q1, &t.Q2, &t.F, &t.ACC};
    for (auto p : s) *p = take(k.S);
    t.flags = (int*)take(1);
    t.zero_bytes = off;
    t.bp = take(nb); t.bx = take(nb); t.hv = take(hb); t.hc = take(hb); t.out = take(8);
    t.ev = take(5 * k.D); t.T = take(k.D);
    t.pre = with_pre ? take((size_t)N_PRE * k.D) : nullptr;
    if (w) *w = t;
    return off;
}

// forward transform onto the coset g <w_D>: the scaling c_i g^i rides in the transform's first pass
int coset_forward(const zkhip_plonk_key& k, const uint64_t* src, size_t n_src, uint64_t* dst) {
    zkhip_ctx* c = k.ctx;
    if (k.log_D >= 12) return zk_ntt_scaled_transform(c, src, n_src, (const uint64_t*)k.gpow.get(), dst, k.log_D);
    hipLaunchKernelGGL(plonk_scale_pad_kernel, dim3(mle_grid_stream(k.D)), dim3(MLE_BLOCK), 0, c->stream, src, (const uint64_t*)k.gpow.get(), n_src, k.D, dst);
    ZK_HIP(c, hipGetLastError());
    return zkhip_domain_transform(c, dst, k.D, dst, k.log_D, 0);
}

int powers(zkhip_ctx* c, const HFr& base, const HFr& scale, size_t count, uint64_t* out) {
    hipLaunchKernelGGL(plonk_powers_kernel, dim3(mle_grid_stream(count)), dim3(MLE_BLOCK), 0, c->stream, fa(base), fa(scale), count, out);
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// the ten coset columns: q_m, q_l, q_r, q_o, q_c, sigma_1..3, L_1 = ifft(1, 0, ..) = (1/n, 1/n, ..), X; tmp: k.S elements
int fill_pre(const zkhip_plonk_key& k, uint64_t* pre, uint64_t* tmp) {
    zkhip_ctx* c = k.ctx;
    for (int j = 0; j < 8; ++j) ZK_TRY(coset_forward(k, k.col_coeff(j), k.n, pre + 4 * k.D * j));
    const HFr n_inv = zkhost::fr_inv(zkhost::fr_from_u64((uint64_t)k.n));
    ZK_TRY(powers(c, zkhost::fr_one(), n_inv, k.n, tmp));
    ZK_TRY(coset_forward(k, tmp, k.n, pre + 4 * k.D * 8));
    const HFr one = zkhost::fr_one();
    ZK_HIP(c, hipMemsetAsync(tmp, 0, 32, c->stream));
    ZK_HIP(c, hipMemcpyAsync(tmp + 4, one.l, 32, hipMemcpyHostToDevice, c->stream));   // (0, 1): the polynomial X, whose coset evaluations are the points
    ZK_HIP(c, hipStreamSynchronize(c->stream));                    // `one` is a stack object
    return coset_forward(k, tmp, 2, pre + 4 * k.D * 9);
}

// up to three commitments in flight, the longest first (a later commit in flight may not be larger than the first)
int commit_group(const zkhip_plonk_key& k, const uint64_t* const* polys, const size_t* lens, int m, uint64_t* const* out_xy, uint8_t* const* out_inf) {
    zkhip_ctx* c = k.ctx;
    int order[3] = {0, 1, 2};
    for (int i = 0; i < m; ++i)
        for (int j = i + 1; j < m; ++j)
            if (lens[order[j]] > lens[order[i]]) std::swap(order[i], order[j]);
    uint32_t ticket[3];
    int rc = ZKHIP_OK, begun = 0;
    for (; begun < m && rc == ZKHIP_OK; ++begun) {
        const int p = order[begun];
        rc = zkhip_kzg_commit_begin(c, k.srs_table ? nullptr : k.srs_xy, k.srs_table, k.srs_inf, k.n_points, polys[p], lens[p], 0, &ticket[begun]);
        if (rc != ZKHIP_OK) break;
    }
    for (int i = 0; i < begun; ++i) {
        const int p = order[i];
        const int r = rc == ZKHIP_OK ? zkhip_kzg_commit_end(c, ticket[i], out_xy[p], out_inf[p]) : zkhip_kzg_commit_end(c, ticket[i], nullptr, nullptr);
        if (rc == ZKHIP_OK) rc = r;
    }
    return rc;
}

// p(z) of n coefficients -> out (device): the scan of zkhip_dense_evaluate
void eval_at(zkhip_ctx* c, const Work& w, const uint64_t* coeffs, size_t n, const HFr& z, uint64_t* out) {
    const uint32_t nb = horner_blocks(n);
    hipLaunchKernelGGL(horner_scan_kernel<false>, dim3(nb), dim3(HS_T), 0, c->stream, coeffs, n, fa(z), w.hv, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(horner_top_kernel, dim3(1), dim3(1024), 0, c->stream, w.hv, nb, fa(z), w.hc, out);
}
// (p(X) - p(z)) / (X - z): n - 1 quotient coefficients, the scan of zkhip_univariate_kzg_open; the remainder p(z) goes to rem
void divide_by_linear(zkhip_ctx* c, const Work& w, const uint64_t* coeffs, size_t n, const HFr& z, uint64_t* quotient, uint64_t* rem) {
    const uint32_t nb = horner_blocks(n);
    hipLaunchKernelGGL(horner_scan_kernel<false>, dim3(nb), dim3(HS_T), 0, c->stream, coeffs, n, fa(z), w.hv, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(horner_top_kernel, dim3(1), dim3(1024), 0, c->stream, w.hv, nb, fa(z), w.hc, (uint64_t*)nullptr);
    hipLaunchKernelGGL(horner_scan_kernel<true>, dim3(nb), dim3(HS_T), 0, c->stream, coeffs, n, fa(z), nullptr, w.hc, quotient, rem);
}

int read_flags(zkhip_ctx* c, const Work& w, bool* any) {
    int h[PLONK_FLAGS];
    ZK_HIP(c, hipMemcpyAsync(h, w.flags, sizeof h, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    *any = false;
    for (int i = 0; i < PLONK_FLAGS; ++i) *any = *any || h[i] != 0;
    return ZKHIP_OK;
}

// round 5's scalars (prover.rs:295-359) from the challenges up to nu and the seven values of round 4 (the six evaluations, then
// PI(zeta)): the fifteen weights of plonk_linearise_kernel in its order of terms, and the constant c0
void round5_scalars(const zkhip_plonk_key& k, const HFr* ch, const HFr* ev, HFr* s, HFr* c0_out) {
    const size_t n = k.n;
    const HFr beta = ch[C_BETA], gamma = ch[C_GAMMA], alpha = ch[C_ALPHA], nu = ch[C_NU], zeta = ch[C_ZETA];
    const HFr az = ev[E_A], bz = ev[E_B], cz = ev[E_C], s1z = ev[E_S1], s2z = ev[E_S2], zwz = ev[E_ZW], piz = ev[6];
    const HFr a2 = fr_mul(alpha, alpha), zn = h_pow(zeta, (uint64_t)n), zh = fr_sub(zn, zkhost::fr_one());
    const HFr l1z = l1_at(zeta, zh, (uint64_t)n);
    const HFr bzeta = fr_mul(beta, zeta);
    const HFr p1 = fr_mul(fr_mul(fr_add(fr_add(az, bzeta), gamma), fr_add(fr_add(bz, fr_add(bzeta, bzeta)), gamma)),
                          fr_add(fr_add(cz, fr_add(bzeta, fr_add(bzeta, bzeta))), gamma));
    const HFr p2 = fr_mul(fr_mul(fr_add(fr_add(az, fr_mul(beta, s1z)), gamma), fr_add(fr_add(bz, fr_mul(beta, s2z)), gamma)), zwz);
    HFr nup[6];
    nup[0] = zkhost::fr_one();
    for (int j = 1; j < 6; ++j) nup[j] = fr_mul(nup[j - 1], nu);
    const HFr w[PLONK_LIN_TERMS] = {fr_mul(az, bz), az, bz, cz, zkhost::fr_one(), fr_add(fr_mul(alpha, p1), fr_mul(a2, l1z)),
                                    h_neg(fr_mul(fr_mul(alpha, beta), p2)), h_neg(zh), h_neg(fr_mul(zh, zn)), h_neg(fr_mul(zh, fr_mul(zn, zn))),
                                    nup[1], nup[2], nup[3], nup[4], nup[5]};
    for (int j = 0; j < PLONK_LIN_TERMS; ++j) s[j] = w[j];
    HFr c0 = fr_sub(piz, fr_mul(fr_mul(alpha, fr_add(cz, gamma)), p2));
    c0 = fr_sub(c0, fr_mul(a2, l1z));
    const HFr opened[5] = {az, bz, cz, s1z, s2z};
    for (int j = 0; j < 5; ++j) c0 = fr_sub(c0, fr_mul(nup[j + 1], opened[j]));
    *c0_out = c0;
}

void absorb_challenges_from_proof(const uint64_t* xy, const uint8_t* inf, const uint64_t* evals, HFr* ch) {   // protocol/utils.rs:56-96
    PlonkRoundTranscript t;
    t.first_round(xy, inf);
    t.second_round(xy, inf);
    t.third_round(xy, inf);
    t.fourth_round(evals);
    t.fifth_round(xy, inf);
    std::memcpy(ch, t.ch, sizeof t.ch);
}

// ---- host G1 for the verifier's combination ---------------------------------------------------------------------------------------
using zkhost::Xyzz;
Xyzz g1_generator_host() {
    static const uint32_t gx[12] = {0xfd530c16u, 0x5cb38790u, 0x9976fff5u, 0x7817fc67u, 0x143ba1c1u, 0x154f95c7u,
                                    0xf3d0e747u, 0xf0ae6acdu, 0x21dbf440u, 0xedce6eccu, 0x9e0bfb75u, 0x12017741u};
    static const uint32_t gy[12] = {0x0ce72271u, 0xbaac93d5u, 0x7918fd8eu, 0x8c22631au, 0x570725ceu, 0xdd595f13u,
                                    0x50405194u, 0x51ac5829u, 0xad0059c0u, 0x0e1c8c3fu, 0x5008a26au, 0x0bbc3efcu};
    uint64_t xy[12];
    for (int i = 0; i < 6; ++i) {
        xy[i] = (uint64_t)gx[2 * i] | ((uint64_t)gx[2 * i + 1] << 32);
        xy[6 + i] = (uint64_t)gy[2 * i] | ((uint64_t)gy[2 * i + 1] << 32);
    }
    return zkhost::xyzz_from_affine(xy, false);
}
Xyzz g1_mul_limbs(const Xyzz& p, const uint64_t* k /* canonical, 4 limbs */) {
    Xyzz acc = zkhost::xyzz_identity();
    for (int i = 255; i >= 0; --i) {
        acc = zkhost::xyzz_double(acc);
        if ((k[i / 64] >> (i % 64)) & 1) acc = zkhost::xyzz_add(acc, p);
    }
    return acc;
}
Xyzz g1_mul(const Xyzz& p, const HFr& mont) { const HFr k = zkhost::fr_from_mont(mont); return g1_mul_limbs(p, k.l); }
// finite points only: on y^2 = x^3 + 4 and of order r
bool g1_valid(const uint64_t* xy) {
    zkhost::Fq x, y;
    std::memcpy(x.l, xy, 48); std::memcpy(y.l, xy + 6, 48);
    if (zkhost::geq_p(x.l) || zkhost::geq_p(y.l)) return false;
    zkhost::Fq four = zkhost::fq_dbl(zkhost::fq_dbl(zkhost::fq_one()));
    if (!zkhost::fq_eq(zkhost::fq_sqr(y), zkhost::fq_add(zkhost::fq_mul(zkhost::fq_sqr(x), x), four))) return false;
    return zkhost::is_identity(g1_mul_limbs(zkhost::xyzz_from_affine(xy, false), zkhost::FR_P));
}

}  // namespace

extern "C" int zkhip_plonk_key_destroy(zkhip_plonk_key* key) {
    if (!key) return ZKHIP_OK;
    if (key->ctx) {
        (void)key->ctx->activate();
        key->ctx->drain_streams();      // nothing of this key's may still be read by a kernel
    }
    delete key;
    return ZKHIP_OK;
}

extern "C" int zkhip_plonk_key_create(zkhip_ctx* c, size_t n, const uint64_t* const* h_column_ptrs, const uint64_t* d_points_xy,
                                      const void* d_table, const uint8_t* d_points_inf, size_t n_points, zkhip_plonk_key** out,
                                      uint64_t* h_commits_xy, uint8_t* h_commits_inf) {
    if (!c || !h_column_ptrs || !out || !h_commits_xy || !h_commits_inf || (!d_points_xy && !d_table)) return ZKHIP_ERR_ARG;
    for (int j = 0; j < 8; ++j) if (!h_column_ptrs[j]) return ZKHIP_ERR_ARG;
    *out = nullptr;
    if (!is_pow2(n) || n < 4) return ZKHIP_ERR_SHAPE;             // Domain::new rounds up; the compiler only makes powers of two
    size_t D = 1;
    while (D < 3 * n + 6) D <<= 1;
    if (log2_exact(D) > 30) return ZKHIP_ERR_SHAPE;
    if (n_points < n + 6) return ZKHIP_ERR_INDEX;                  // powers_of_tau_in_g1[i] out of bounds (univariate_kzg.rs:53) at t_high
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;                 // the columns' transforms and the eight commits need the workspace: nothing allocated or copied
    ZK_TRY(c->activate());
    std::unique_ptr<zkhip_plonk_key> k(new (std::nothrow) zkhip_plonk_key());
    if (!k) return ZKHIP_ERR_NOMEM;
    k->ctx = c; k->n = n; k->D = D; k->S = n + 8;
    k->log_n = log2_exact(n); k->log_D = log2_exact(D); k->ratio = (uint32_t)(D / n);
    k->srs_xy = d_table ? nullptr : d_points_xy; k->srs_table = d_table; k->srs_inf = d_points_inf; k->n_points = n_points;
    const bool cache = (size_t)N_PRE * D * 32 <= plonk_cache_budget();
    const size_t work_bytes = work_layout(*k, nullptr, !cache, nullptr);
    if (dev_alloc(k->evals, 8 * n * 32) != hipSuccess || dev_alloc(k->coeffs, 8 * k->S * 32) != hipSuccess ||
        dev_alloc(k->omega, n * 32) != hipSuccess || dev_alloc(k->gpow, k->S * 32) != hipSuccess ||
        dev_alloc(k->ginv, (3 * n + 8) * 32) != hipSuccess || dev_alloc(k->work, work_bytes) != hipSuccess ||
        (cache && dev_alloc(k->pre, (size_t)N_PRE * D * 32) != hipSuccess))
        return ZKHIP_ERR_NOMEM;
    HFr w_D, tmp1, tmp2;
    ZK_TRY(zkhip_domain_params((uint64_t)n, k->w_n.l, tmp1.l, tmp2.l));
    ZK_TRY(zkhip_domain_params((uint64_t)D, w_D.l, tmp1.l, tmp2.l));
    const HFr g = zkhost::fr_from_u64(COSET_SHIFT);
    {   // Z_H(g w_D^j) = g^n rho^(j mod D/n) - 1, rho = w_D^n
        const HFr gn = h_pow(g, (uint64_t)n), rho = h_pow(w_D, (uint64_t)n);
        HFr cur = gn;
        for (uint32_t j = 0; j < 8; ++j) {
            k->zh_inv[j] = j < k->ratio ? zkhost::fr_inv(fr_sub(cur, zkhost::fr_one())) : zkhost::fr_zero();
            cur = fr_mul(cur, rho);
        }
    }
    ZK_HIP(c, hipMemsetAsync(k->coeffs.get(), 0, 8 * k->S * 32, c->stream));
    for (int j = 0; j < 8; ++j) {
        ZK_HIP(c, hipMemcpyAsync(k->col_eval(j), h_column_ptrs[j], n * 32, hipMemcpyDeviceToDevice, c->stream));
        ZK_TRY(zkhip_domain_transform(c, k->col_eval(j), n, k->col_coeff(j), k->log_n, 1));      // to_coefficient_poly
    }
    ZK_TRY(powers(c, k->w_n, zkhost::fr_one(), n, (uint64_t*)k->omega.get()));
    ZK_TRY(powers(c, g, zkhost::fr_one(), k->S, (uint64_t*)k->gpow.get()));
    ZK_TRY(powers(c, zkhost::fr_inv(g), zkhost::fr_one(), 3 * n + 8, (uint64_t*)k->ginv.get()));
    if (cache) {
        Work w;
        work_layout(*k, (char*)k->work.get(), false, &w);
        ZK_TRY(fill_pre(*k, (uint64_t*)k->pre.get(), w.W));
    }
    for (int j = 0; j < 8; ++j) {                                  // VerifierPreprocessedInput::vpi (verifier.rs:24-36)
        const int rc = d_table ? zkhip_kzg_commit_table(c, d_table, d_points_inf, n_points, k->col_coeff(j), n, 0, h_commits_xy + 12 * j, h_commits_inf + j)
                               : zkhip_kzg_commit(c, d_points_xy, d_points_inf, n_points, k->col_coeff(j), n, 0, h_commits_xy + 12 * j, h_commits_inf + j);
        ZK_TRY(rc);
    }
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    *out = k.release();
    return ZKHIP_OK;
}

extern "C" int zkhip_plonk_prove(zkhip_plonk_key* key, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, const uint64_t* d_public,
                                 const uint64_t* h_blinding, uint64_t* h_points_xy, uint8_t* h_points_inf, uint64_t* h_evals,
                                 uint64_t* h_challenges) {
    if (!key || !d_a || !d_b || !d_c || !d_public || !h_blinding || !h_points_xy || !h_points_inf || !h_evals) return ZKHIP_ERR_ARG;
    const zkhip_plonk_key& k = *key;
    zkhip_ctx* c = k.ctx;
    ZK_TRY(c->activate());
    const size_t n = k.n, D = k.D;
    Work w;
    work_layout(k, (char*)k.work.get(), !k.pre, &w);
    const uint64_t* pre = k.pre ? (const uint64_t*)k.pre.get() : w.pre;
    HFr bl[11];
    for (int i = 0; i < 11; ++i) {
        bl[i] = h_load(h_blinding + 4 * i);
        if (zkhost::fr_geq_p(bl[i].l)) return ZKHIP_ERR_ARG;
    }
    // the transforms and the commits need the context's workspace: refused before the work area is cleared and the outputs are zeroed
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;
    std::memset(h_points_xy, 0, 96 * N_POINTS);
    std::memset(h_points_inf, 0, N_POINTS);
    uint64_t* xy[N_POINTS]; uint8_t* inf[N_POINTS];
    for (int p = 0; p < N_POINTS; ++p) { xy[p] = h_points_xy + 12 * p; inf[p] = h_points_inf + p; }
    ZK_HIP(c, hipMemsetAsync(w.A, 0, w.zero_bytes, c->stream));
    PlonkRoundTranscript tr;
    const HFr* const ch = tr.ch;
    auto commit = [&](const CommitRound& r) {
        const CommitSet cs = commit_set(w, n, r);
        return commit_group(k, cs.polys, cs.lens, r.m, &xy[r.first], &inf[r.first]);
    };

    // ---- round 1 (prover.rs:98-123): a_s = (r0 X + r1) Z_H + a, likewise b_s, c_s
    {
        const uint64_t* wires[3] = {d_a, d_b, d_c};
        for (int j = 0; j < 3; ++j) {
            uint64_t* const dst = w.*COMMIT_WIRES.p[j].own;
            ZK_TRY(zkhip_domain_transform(c, wires[j], n, dst, k.log_n, 1));
            PlonkBlindArg b = {};
            std::memcpy(b.v, bl[2 * j + 1].l, 32);                 // constant coefficient: rands[1], then rands[0] X
            std::memcpy(b.v + 4, bl[2 * j].l, 32);
            hipLaunchKernelGGL(plonk_blind_kernel, dim3(1), dim3(64), 0, c->stream, dst, n, 2u, b);
        }
        ZK_TRY(zkhip_domain_transform(c, d_public, n, w.PI, k.log_n, 1));
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(commit(COMMIT_WIRES));
    }
    tr.first_round(h_points_xy, h_points_inf);
    // ---- round 2 (:125-175): the accumulator, z = (r0 + r1 X + r2 X^2) Z_H + acc
    {
        PlonkCols cols;
        for (int j = 0; j < 8; ++j) cols.q[j] = k.col_eval(j);
        const uint32_t nb = (uint32_t)((n + GP_ROWS - 1) / GP_ROWS);
        {
            ProfScope ps(c, "plonk_grand_product", 32.0 * 14.0 * (double)n);
            hipLaunchKernelGGL(plonk_gp_ratio_kernel, dim3(nb), dim3(GP_T), 0, c->stream, d_a, d_b, d_c, d_public, cols, (const uint64_t*)k.omega.get(), n,
                               fa(ch[C_BETA]), fa(ch[C_GAMMA]), w.F, w.bp, w.flags);
            hipLaunchKernelGGL(plonk_gp_top_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint64_t*)w.bp, nb, w.bx);
            hipLaunchKernelGGL(plonk_gp_apply_kernel, dim3(nb), dim3(GP_T), 0, c->stream, (const uint64_t*)w.F, (const uint64_t*)w.bx, n, w.ACC, w.flags);
        }
        ZK_HIP(c, hipGetLastError());
        bool bad = false;
        ZK_TRY(read_flags(c, w, &bad));
        if (bad) return ZKHIP_ERR_ARG;      // a row breaks the gate identity, a denominator vanishes or the accumulator does not close
        ZK_TRY(zkhip_domain_transform(c, w.ACC, n, w.Z, k.log_n, 1));
        PlonkBlindArg b = {};
        for (int j = 0; j < 3; ++j) std::memcpy(b.v + 4 * j, bl[6 + j].l, 32);
        hipLaunchKernelGGL(plonk_blind_kernel, dim3(1), dim3(64), 0, c->stream, w.Z, n, 3u, b);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(commit(COMMIT_ACC));
    }
    tr.second_round(h_points_xy, h_points_inf);
    // ---- round 3 (:177-258): t = numerator / Z_H on the coset, back to coefficients, split and blinded
    {
        for (int j = 0; j < PB_COSET_ROWS; ++j) ZK_TRY(coset_forward(k, w.*COSET_INPUTS[j].own, n + COSET_INPUTS[j].extra, w.ev + 4 * D * j));
        if (!k.pre) ZK_TRY(fill_pre(k, w.pre, w.W));
        PlonkQuotArg q = {};
        q.beta = fa(ch[C_BETA]); q.gamma = fa(ch[C_GAMMA]); q.alpha = fa(ch[C_ALPHA]); q.alpha2 = fa(fr_mul(ch[C_ALPHA], ch[C_ALPHA]));
        for (int j = 0; j < 8; ++j) q.zh_inv[j] = fa(k.zh_inv[j]);
        q.rot = k.ratio;
        {
            ProfScope ps(c, "plonk_quotient", 32.0 * 17.0 * (double)D);
            hipLaunchKernelGGL(plonk_quotient_kernel, dim3(mle_grid_stream(D)), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t*)w.ev, pre, D, q, w.T);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(zkhip_domain_transform(c, w.T, D, w.T, k.log_D, 1));
        {
            ProfScope ps(c, "plonk_split", 32.0 * (double)(D + 6 * n));
            hipLaunchKernelGGL(plonk_split_kernel, dim3(mle_grid_stream(D)), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t*)w.T, (const uint64_t*)k.ginv.get(), n, D,
                               fa(bl[9]), fa(bl[10]), w.TL, w.TM, w.TH, w.flags);
        }
        ZK_HIP(c, hipGetLastError());
        bool bad = false;
        ZK_TRY(read_flags(c, w, &bad));
        if (bad) return ZKHIP_ERR_ARG;      // Z_H does not divide the numerator: no proof from it
        ZK_TRY(commit(COMMIT_T));
    }
    tr.third_round(h_points_xy, h_points_inf);
    // ---- round 4 (:260-293): six evaluations (and PI(zeta) for round 5)
    const HFr zeta = ch[C_ZETA], zeta_w = fr_mul(zeta, k.w_n);
    HFr ev[PB_JOBS];
    {
        ProfScope ps(c, "plonk_evaluate", 32.0 * 7.0 * (double)n);
        for (int j = 0; j < PB_JOBS; ++j) {
            const RoundPoly& e = EVAL_JOBS[j];
            eval_at(c, w, poly_at(k, w, e), n + e.extra, e.at_zeta_w ? zeta_w : zeta, w.out + 4 * j);
        }
    }
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipMemcpyAsync(ev, w.out, sizeof ev, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(h_evals, ev, 32 * N_EVALS);
    tr.fourth_round(h_evals);
    // ---- round 5 (:295-376): W_zeta = (r + nu-combination) / (X - zeta), W_zeta_omega = (z - z(w zeta)) / (X - w zeta)
    {
        HFr s[PLONK_LIN_TERMS], c0;
        round5_scalars(k, ch, ev, s, &c0);
        PlonkLinArg L = {};
        for (int j = 0; j < PLONK_LIN_TERMS; ++j) { L.p[j] = poly_at(k, w, LIN_TERMS[j]); L.s[j] = fa(s[j]); }
        L.c0 = fa(c0);
        {
            ProfScope ps(c, "plonk_linearise", 32.0 * 16.0 * (double)n);
            hipLaunchKernelGGL(plonk_linearise_kernel, dim3(mle_grid_stream(n + 6)), dim3(MLE_BLOCK), 0, c->stream, L, n + 6, w.W);
        }
        {
            ProfScope ps(c, "plonk_divide", 96.0 * 2.0 * (double)n);
            for (int j = 0; j < 2; ++j) {
                const RoundPoly& d = DIVIDE_JOBS[j];
                divide_by_linear(c, w, w.*d.own, n + d.extra, d.at_zeta_w ? zeta_w : zeta, w.*d.quotient, w.out + 4 * j);
            }
        }
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(commit(COMMIT_OPENINGS));
    }
    tr.fifth_round(h_points_xy, h_points_inf);
    if (h_challenges) std::memcpy(h_challenges, ch, sizeof tr.ch);
    return ZKHIP_OK;
}

// ---- the batched prover -------------------------------------------------------------------------------------------------------------
// zkhip_plonk_prove_batch proves CHUNKS of proofs: round r of every proof of a chunk before round r + 1 of any, one synchronisation per
// round and chunk, the launches of a chunk independent of the proofs in it (plonk_batch_kernels.hpp).  A chunk is
// min(batch, PLONK_BATCH_CHUNK, what fits PLONK_BATCH_BUDGET) proofs, at least one: every proof owns a work area of the single
// prover's layout plus the workgroup values of its seven Horner jobs, and a key without a coset cache adds its ten coset columns ONCE
// (they are the key's, not a proof's: the budget pays for them before it is divided).  The area is allocated by the first batch call,
// grown if a later call's chunk is larger, kept with the key and freed with it.
constexpr size_t PLONK_BATCH_BUDGET = (size_t)256 << 20;
constexpr uint32_t PLONK_BATCH_CHUNK = 64;

namespace {

struct BatchLayout {
    size_t per = 0, ws = 0, fs = 0;                            // a proof's area: bytes, elements, ints
    size_t hb = 0, o_hv = 0, o_hc = 0;                         // workgroup values per Horner job; the two scratch rows in a proof's area
    size_t o_par = 0, o_cols = 0, o_pre = 0, o_areas = 0, dev_bytes = 0;
    size_t p_par = 0, p_cols = 0, p_flags = 0, p_out = 0, pin_bytes = 0;
};
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
BatchLayout batch_layout(const zkhip_plonk_key& k, uint32_t chunk) {
    BatchLayout L;
    const size_t base = work_layout(k, nullptr, false, nullptr);
    L.hb = horner_row(k);
    L.o_hv = base;
    L.o_hc = L.o_hv + al256((size_t)PB_JOBS * L.hb * 32);
    L.per = L.o_hc + al256((size_t)PB_JOBS * L.hb * 32);
    L.ws = L.per / 32; L.fs = L.per / sizeof(int);
    L.o_par = 0;
    L.o_cols = L.o_par + al256((size_t)chunk * PB_SLOTS * 32);
    L.o_pre = L.o_cols + al256((size_t)chunk * 4 * sizeof(uint64_t*));
    L.o_areas = L.o_pre + (k.pre ? 0 : al256((size_t)N_PRE * k.D * 32));
    L.dev_bytes = L.o_areas + (size_t)chunk * L.per;
    L.p_par = 0;
    L.p_cols = L.p_par + al256((size_t)chunk * PB_SLOTS * 32);
    L.p_flags = L.p_cols + al256((size_t)chunk * 4 * sizeof(uint64_t*));
    L.p_out = L.p_flags + al256((size_t)chunk * PLONK_FLAGS * sizeof(int));
    L.pin_bytes = L.p_out + al256((size_t)chunk * PB_JOBS * 32);
    return L;
}
uint32_t batch_chunk_for(const zkhip_plonk_key& k, size_t batch) {
    const size_t per = batch_layout(k, 1).per, pre_bytes = k.pre ? 0 : (size_t)N_PRE * k.D * 32;
    const size_t fit = PLONK_BATCH_BUDGET > pre_bytes ? (PLONK_BATCH_BUDGET - pre_bytes) / per : 0;
    return (uint32_t)std::max<size_t>(1, std::min({batch, (size_t)PLONK_BATCH_CHUNK, fit}));
}

// the pointer table of a chunk as the gather kernel reads it: proof b's a, b, c, public at [4 b .. 4 b + 3]
void pack_columns(const uint64_t* const* a, const uint64_t* const* b, const uint64_t* const* c, const uint64_t* const* pub, size_t first, uint32_t count,
                  const uint64_t** out) {
    for (uint32_t i = 0; i < count; ++i) {
        out[4 * i] = a[first + i]; out[4 * i + 1] = b[first + i]; out[4 * i + 2] = c[first + i]; out[4 * i + 3] = pub[first + i];
    }
}

// one proof of a chunk on the host: its transcript, challenges, blinding and verdict
struct BatchProof {
    PlonkRoundTranscript tr;                                   // with the proof's challenges, tr.ch
    HFr ev[PB_JOBS];
    bool refused = false;
};

struct BatchRun {
    zkhip_plonk_key& k;
    zkhip_ctx* c;
    BatchLayout L;
    uint32_t bc;                                               // proofs of this chunk
    char* dev; char* pin;
    Work w;                                                    // proof 0's area
    uint64_t *hv, *hc;
    const uint64_t* par;                                       // device
    HFr* h_par;                                                // pinned
    std::vector<BatchProof> pr;
    uint64_t* xy; uint8_t* inf;                                // the chunk's first proof in the caller's arrays

    HFr& slot(uint32_t b, uint32_t s) { return h_par[(size_t)b * PB_SLOTS + s]; }
    int upload_par() {
        ZK_HIP(c, hipMemcpyAsync(dev + L.o_par, pin + L.p_par, (size_t)bc * PB_SLOTS * 32, hipMemcpyHostToDevice, c->stream));
        return ZKHIP_OK;
    }
    template <class F> void each(F f) {                        // host work per proof: on the context's pool
        ZkHostPool* pool = bc > 1 ? c->pool() : nullptr;
        if (!pool) { for (uint32_t b = 0; b < bc; ++b) if (!pr[b].refused) f(b); }
        else pool->run(bc, [&](unsigned b) { if (!pr[b].refused) f(b); });
    }
    int transform(const uint64_t* src, uint64_t* dst, size_t n_src, uint32_t log_n, int inverse) {
        return zkhip_domain_transform_batch(c, bc, src, L.ws, n_src, dst, L.ws, log_n, inverse);
    }
    void blind(uint64_t* const* polys, uint32_t m, uint32_t kk, const uint8_t (*slots)[3]) {
        PlonkBlindBatchArg a = {};
        for (uint32_t q = 0; q < m; ++q) { a.p[q] = polys[q]; for (int j = 0; j < 3; ++j) a.slot[q][j] = slots[q][j]; }
        hipLaunchKernelGGL(plonk_batch_blind_kernel, dim3(m, bc), dim3(64), 0, c->stream, a, k.n, kk, par, L.ws);
    }
    int copy_flags() {                                         // rides on the round's synchronisation
        ZK_HIP(c, hipMemcpy2DAsync(pin + L.p_flags, PLONK_FLAGS * sizeof(int), w.flags, L.per, PLONK_FLAGS * sizeof(int), bc, hipMemcpyDeviceToHost, c->stream));
        return ZKHIP_OK;
    }
    void read_flags() {
        const int* f = (const int*)(pin + L.p_flags);
        for (uint32_t b = 0; b < bc; ++b)
            for (int i = 0; i < PLONK_FLAGS; ++i) if (f[PLONK_FLAGS * b + i]) pr[b].refused = true;
    }
    // One round's commits of the chunk, m polynomials per proof, results at point `first` on; ends in the round's synchronisation.
    // Short path: one launch chain for all of them.  Otherwise commit_group, three in flight, proof after proof.
    int commit(const CommitRound& r) {
        const CommitSet cs = commit_set(w, k.n, r);
        uint64_t* const* polys = cs.polys;
        const size_t* lens = cs.lens;
        const uint32_t m = (uint32_t)r.m;
        const int first = r.first;
        if (k.srs_table && zk_msm_commit_batch_serves(k.n_points, k.n + 6)) {
            size_t off[3];
            for (uint32_t j = 0; j < m; ++j) off[j] = (size_t)(polys[j] - w.A) / 4;
            return zk_msm_commit_batch(c, k.srs_table, k.srs_inf, k.n_points, w.A, L.ws, bc, m, off, lens, xy + 12 * first, inf + first, N_POINTS);
        }
        ZK_HIP(c, hipStreamSynchronize(c->stream));            // the flags and values of this round: a refused proof is not committed
        read_flags();
        for (uint32_t b = 0; b < bc; ++b) {
            if (pr[b].refused) continue;
            const uint64_t* p[3]; uint64_t* oxy[3]; uint8_t* oinf[3];
            for (uint32_t j = 0; j < m; ++j) {
                p[j] = polys[j] + 4 * (size_t)b * L.ws;
                oxy[j] = xy + 12 * ((size_t)b * N_POINTS + first + j);
                oinf[j] = inf + (size_t)b * N_POINTS + first + j;
            }
            ZK_TRY(commit_group(k, p, lens, (int)m, oxy, oinf));
        }
        return ZKHIP_OK;
    }
    // the jobs of one Horner launch chain from rows of the round table; *nb: the workgroups of the longest job
    template <int N> HornerBatchArg horner_arg(const RoundPoly (&jobs)[N], uint32_t* nb) {
        static_assert(N <= PB_JOBS, "a launch takes up to PB_JOBS jobs");
        HornerBatchArg h = {};
        size_t longest = 0;
        for (int j = 0; j < N; ++j) {
            h.coeffs[j] = poly_at(k, w, jobs[j]);
            h.quotient[j] = jobs[j].quotient ? w.*jobs[j].quotient : nullptr;
            h.len[j] = (uint32_t)(k.n + jobs[j].extra);
            h.zslot[j] = jobs[j].at_zeta_w ? PB_ZETA_W : PB_ZETA;
            longest = std::max<size_t>(longest, h.len[j]);
        }
        h.own = own_mask(jobs);
        h.vstride = (uint32_t)L.hb;
        *nb = horner_blocks(longest);
        return h;
    }
    int rounds(const uint64_t* const* h_cols, bool* pre_ready);
};

int BatchRun::rounds(const uint64_t* const* h_cols, bool* pre_ready) {
    const size_t n = k.n, D = k.D, ws = L.ws, fs = L.fs;
    const uint64_t* pre = k.pre ? (const uint64_t*)k.pre.get() : (const uint64_t*)(dev + L.o_pre);
    auto points = [&](uint32_t b) { return xy + 12 * (size_t)N_POINTS * b; };      // proof b's nine points and their flags
    auto flags = [&](uint32_t b) { return inf + (size_t)N_POINTS * b; };
    ZK_HIP(c, hipMemset2DAsync(w.A, L.per, 0, w.zero_bytes, bc, c->stream));
    // ---- round 1: the columns into the areas, to coefficients, blinded, committed
    std::memcpy(pin + L.p_cols, h_cols, (size_t)bc * 4 * sizeof(uint64_t*));
    ZK_HIP(c, hipMemcpyAsync(dev + L.o_cols, pin + L.p_cols, (size_t)bc * 4 * sizeof(uint64_t*), hipMemcpyHostToDevice, c->stream));
    ZK_TRY(upload_par());
    uint64_t* const stage = w.ev;                              // a, b, c, public of a proof in evaluation form: n each (the coset rows come later)
    {
        ProfScope ps(c, "plonk_batch_gather", 64.0 * 4.0 * (double)n * bc);
        hipLaunchKernelGGL(plonk_batch_gather_kernel, dim3(mle_grid_stream(n), 4, bc), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t* const*)(dev + L.o_cols), n,
                           stage, ws);
    }
    ZK_HIP(c, hipGetLastError());
    {
        uint64_t* dst[4] = {w.A, w.B, w.C, w.PI};
        for (int j = 0; j < 4; ++j) ZK_TRY(transform(stage + 4 * n * j, dst[j], n, k.log_n, 1));
        static const uint8_t slots[3][3] = {{1, 0, 0}, {3, 2, 0}, {5, 4, 0}};      // constant coefficient: rands[1], then rands[0] X
        blind(dst, 3, 2, slots);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(copy_flags());
        ZK_TRY(commit(COMMIT_WIRES));
    }
    each([&](uint32_t b) {
        pr[b].tr.first_round(points(b), flags(b));
        slot(b, PB_BETA) = pr[b].tr.ch[C_BETA]; slot(b, PB_GAMMA) = pr[b].tr.ch[C_GAMMA];
    });
    // ---- round 2: the accumulator
    ZK_TRY(upload_par());
    {
        PlonkCols cols;
        for (int j = 0; j < 8; ++j) cols.q[j] = k.col_eval(j);
        const uint32_t nb = (uint32_t)((n + GP_ROWS - 1) / GP_ROWS);
        {
            ProfScope ps(c, "plonk_batch_grand_product", 32.0 * 14.0 * (double)n * bc);
            hipLaunchKernelGGL(plonk_batch_gp_ratio_kernel, dim3(nb, bc), dim3(GP_T), 0, c->stream, (const uint64_t*)stage, (const uint64_t*)(stage + 4 * n),
                               (const uint64_t*)(stage + 8 * n), (const uint64_t*)(stage + 12 * n), cols, (const uint64_t*)k.omega.get(), n, par, w.F, w.bp,
                               w.flags, ws, fs);
            hipLaunchKernelGGL(plonk_batch_gp_top_kernel, dim3(bc), dim3(1024), 0, c->stream, (const uint64_t*)w.bp, nb, w.bx, ws);
            hipLaunchKernelGGL(plonk_batch_gp_apply_kernel, dim3(nb, bc), dim3(GP_T), 0, c->stream, (const uint64_t*)w.F, (const uint64_t*)w.bx, n, w.ACC, w.flags,
                               ws, fs);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(copy_flags());
        ZK_TRY(transform(w.ACC, w.Z, n, k.log_n, 1));
        uint64_t* polys[1] = {w.Z};
        static const uint8_t slots[1][3] = {{6, 7, 8}};
        blind(polys, 1, 3, slots);
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(commit(COMMIT_ACC));
        read_flags();       // a row breaks the gate identity, a denominator vanishes or the accumulator does not close: that proof is refused
    }
    each([&](uint32_t b) {
        pr[b].tr.second_round(points(b), flags(b));
        slot(b, PB_ALPHA) = pr[b].tr.ch[C_ALPHA]; slot(b, PB_ALPHA2) = fr_mul(pr[b].tr.ch[C_ALPHA], pr[b].tr.ch[C_ALPHA]);
    });
    // ---- round 3: the quotient on the coset
    ZK_TRY(upload_par());
    {
        PlonkPadBatchArg pad = {};
        for (int j = 0; j < PB_COSET_ROWS; ++j) { pad.src[j] = w.*COSET_INPUTS[j].own; pad.len[j] = (uint32_t)(n + COSET_INPUTS[j].extra); }
        {
            ProfScope ps(c, "plonk_batch_scale_pad", 32.0 * 5.0 * (double)(D + n) * bc);
            hipLaunchKernelGGL(plonk_batch_scale_pad_kernel, dim3(mle_grid_stream(D), PB_COSET_ROWS, bc), dim3(MLE_BLOCK), 0, c->stream, pad,
                               (const uint64_t*)k.gpow.get(), D, w.ev, ws);
        }
        ZK_HIP(c, hipGetLastError());
        for (int j = 0; j < PB_COSET_ROWS; ++j) ZK_TRY(transform(w.ev + 4 * D * j, w.ev + 4 * D * j, D, k.log_D, 0));
        if (!k.pre && !*pre_ready) {
            ZK_TRY(fill_pre(k, (uint64_t*)(dev + L.o_pre), w.W));
            *pre_ready = true;
        }
        PlonkQuotBatchArg q = {};
        for (int j = 0; j < 8; ++j) q.zh_inv[j] = fa(k.zh_inv[j]);
        q.rot = k.ratio;
        {
            ProfScope ps(c, "plonk_batch_quotient", 32.0 * 17.0 * (double)D * bc);
            hipLaunchKernelGGL(plonk_batch_quotient_kernel, dim3(mle_grid_stream(D), bc), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t*)w.ev, pre, D, q, par, w.T, ws);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(transform(w.T, w.T, D, k.log_D, 1));
        {
            ProfScope ps(c, "plonk_batch_split", 32.0 * (double)(D + 6 * n) * bc);
            hipLaunchKernelGGL(plonk_batch_split_kernel, dim3(mle_grid_stream(D), bc), dim3(MLE_BLOCK), 0, c->stream, (const uint64_t*)w.T,
                               (const uint64_t*)k.ginv.get(), n, D, par, w.TL, w.TM, w.TH, w.flags, ws, fs);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(copy_flags());
        ZK_TRY(commit(COMMIT_T));
        read_flags();       // Z_H does not divide the numerator: no proof from it
    }
    each([&](uint32_t b) {
        pr[b].tr.third_round(points(b), flags(b));
        slot(b, PB_ZETA) = pr[b].tr.ch[C_ZETA]; slot(b, PB_ZETA_W) = fr_mul(pr[b].tr.ch[C_ZETA], k.w_n);
    });
    // ---- round 4: the six evaluations and PI(zeta), seven jobs per proof in one scan and one top launch
    ZK_TRY(upload_par());
    {
        uint32_t nb;
        const HornerBatchArg h = horner_arg(EVAL_JOBS, &nb);
        {
            ProfScope ps(c, "plonk_batch_evaluate", 32.0 * 7.0 * (double)n * bc);
            hipLaunchKernelGGL(horner_batch_scan_kernel<false>, dim3(nb, PB_JOBS, bc), dim3(HS_T), 0, c->stream, h, par, hv, (const uint64_t*)nullptr,
                               (uint64_t*)nullptr, ws);
            hipLaunchKernelGGL(horner_batch_top_kernel, dim3(PB_JOBS, bc), dim3(1024), 0, c->stream, h, par, (const uint64_t*)hv, hc, w.out, ws);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_HIP(c, hipMemcpy2DAsync(pin + L.p_out, PB_JOBS * 32, w.out, L.per, PB_JOBS * 32, bc, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipStreamSynchronize(c->stream));
    }
    each([&](uint32_t b) {
        std::memcpy(pr[b].ev, pin + L.p_out + (size_t)b * PB_JOBS * 32, sizeof pr[b].ev);
        pr[b].tr.fourth_round(pr[b].ev[0].l);
        HFr c0;
        round5_scalars(k, pr[b].tr.ch, pr[b].ev, &slot(b, PB_LIN), &c0);
        slot(b, PB_C0) = c0;
    });
    // ---- round 5: the linearisation and the two opening quotients
    ZK_TRY(upload_par());
    {
        PlonkLinBatchArg lin = {};
        for (int j = 0; j < PLONK_LIN_TERMS; ++j) lin.p[j] = poly_at(k, w, LIN_TERMS[j]);
        lin.own = own_mask(LIN_TERMS);                         // z, the three parts of t, the three wires
        {
            ProfScope ps(c, "plonk_batch_linearise", 32.0 * 16.0 * (double)n * bc);
            hipLaunchKernelGGL(plonk_batch_linearise_kernel, dim3(mle_grid_stream(n + 6), bc), dim3(MLE_BLOCK), 0, c->stream, lin, n + 6, par, w.W, ws);
        }
        uint32_t nb;
        const HornerBatchArg h = horner_arg(DIVIDE_JOBS, &nb);
        {
            ProfScope ps(c, "plonk_batch_divide", 96.0 * 2.0 * (double)n * bc);
            hipLaunchKernelGGL(horner_batch_scan_kernel<false>, dim3(nb, 2, bc), dim3(HS_T), 0, c->stream, h, par, hv, (const uint64_t*)nullptr, (uint64_t*)nullptr, ws);
            hipLaunchKernelGGL(horner_batch_top_kernel, dim3(2, bc), dim3(1024), 0, c->stream, h, par, (const uint64_t*)hv, hc, (uint64_t*)nullptr, ws);
            hipLaunchKernelGGL(horner_batch_scan_kernel<true>, dim3(nb, 2, bc), dim3(HS_T), 0, c->stream, h, par, (uint64_t*)nullptr, (const uint64_t*)hc, w.out, ws);
        }
        ZK_HIP(c, hipGetLastError());
        ZK_TRY(copy_flags());
        ZK_TRY(commit(COMMIT_OPENINGS));
    }
    each([&](uint32_t b) {
        pr[b].tr.fifth_round(points(b), flags(b));
    });
    return ZKHIP_OK;
}

}  // namespace

extern "C" uint32_t zkhip_plonk_batch_chunk(const zkhip_plonk_key* key) { return key ? batch_chunk_for(*key, PLONK_BATCH_CHUNK) : 0; }

extern "C" int zkhip_plonk_prove_batch(zkhip_plonk_key* key, uint32_t batch, const uint64_t* const* h_a_ptrs, const uint64_t* const* h_b_ptrs,
                                       const uint64_t* const* h_c_ptrs, const uint64_t* const* h_public_ptrs, const uint64_t* h_blinding,
                                       uint64_t* h_points_xy, uint8_t* h_points_inf, uint64_t* h_evals, uint64_t* h_challenges, int32_t* h_status) {
    if (!key) return ZKHIP_ERR_ARG;
    if (!batch) return ZKHIP_OK;
    if (!h_a_ptrs || !h_b_ptrs || !h_c_ptrs || !h_public_ptrs || !h_blinding || !h_points_xy || !h_points_inf || !h_evals || !h_status) return ZKHIP_ERR_ARG;
    if (batch > 65535) return ZKHIP_ERR_SHAPE;
    for (uint32_t b = 0; b < batch; ++b) if (!h_a_ptrs[b] || !h_b_ptrs[b] || !h_c_ptrs[b] || !h_public_ptrs[b]) return ZKHIP_ERR_ARG;
    zkhip_plonk_key& k = *key;
    zkhip_ctx* c = k.ctx;
    ZK_TRY(c->activate());
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;             // a commit or a split-phase session holds the context's workspace
    const uint32_t chunk = batch_chunk_for(k, batch);
    if (chunk > 1 && chunk > k.batch_chunk) {                   // the first batch call, or a larger chunk than any before
        ZK_HIP(c, hipStreamSynchronize(c->stream));            // nothing of an earlier batch may still read the old area
        const BatchLayout L = batch_layout(k, chunk);
        DevMem dev; PinMem pin;
        if (dev_alloc(dev, L.dev_bytes) != hipSuccess || pin_alloc(pin, L.pin_bytes) != hipSuccess) { (void)hipGetLastError(); return ZKHIP_ERR_NOMEM; }
        k.batch_work = std::move(dev); k.batch_pin = std::move(pin); k.batch_chunk = chunk;
    }
    bool any_refused = false, pre_ready = false;
    for (uint32_t b0 = 0; b0 < batch; b0 += chunk) {
        const uint32_t bc = std::min(chunk, batch - b0);
        uint64_t* xy = h_points_xy + 12 * (size_t)N_POINTS * b0;
        uint8_t* inf = h_points_inf + (size_t)N_POINTS * b0;
        uint64_t* evals = h_evals + 4 * (size_t)N_EVALS * b0;
        uint64_t* chal = h_challenges ? h_challenges + 4 * (size_t)N_CHALLENGES * b0 : nullptr;
        std::vector<uint8_t> refused(bc, 0);
        if (bc == 1) {                                         // a chunk of one proof is the single prover
            const int rc = zkhip_plonk_prove(key, h_a_ptrs[b0], h_b_ptrs[b0], h_c_ptrs[b0], h_public_ptrs[b0], h_blinding + 44 * (size_t)b0, xy, inf, evals, chal);
            if (rc != ZKHIP_OK && rc != ZKHIP_ERR_ARG) return rc;
            refused[0] = rc == ZKHIP_ERR_ARG;
        } else {
            BatchRun run{k, c, batch_layout(k, k.batch_chunk), bc};
            run.dev = (char*)k.batch_work.get(); run.pin = (char*)k.batch_pin.get();
            work_layout(k, run.dev + run.L.o_areas, false, &run.w);
            run.hv = (uint64_t*)(run.dev + run.L.o_areas + run.L.o_hv); run.hc = (uint64_t*)(run.dev + run.L.o_areas + run.L.o_hc);
            run.par = (const uint64_t*)(run.dev + run.L.o_par); run.h_par = (HFr*)(run.pin + run.L.p_par);
            run.pr.resize(bc);
            run.xy = xy; run.inf = inf;
            std::memset(run.h_par, 0, (size_t)bc * PB_SLOTS * 32);
            for (uint32_t b = 0; b < bc; ++b) {
                const uint64_t* bl = h_blinding + 44 * (size_t)(b0 + b);
                for (int i = 0; i < 11; ++i) if (zkhost::fr_geq_p(bl + 4 * i)) run.pr[b].refused = true;     // an unreduced blinding scalar
                if (!run.pr[b].refused) std::memcpy(&run.slot(b, PB_BLIND), bl, 11 * 32);
            }
            std::memset(xy, 0, 96 * (size_t)N_POINTS * bc);
            std::memset(inf, 0, (size_t)N_POINTS * bc);
            std::vector<const uint64_t*> cols(4 * (size_t)bc);
            pack_columns(h_a_ptrs, h_b_ptrs, h_c_ptrs, h_public_ptrs, b0, bc, cols.data());
            const int rc = run.rounds(cols.data(), &pre_ready);
            if (rc != ZKHIP_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
            for (uint32_t b = 0; b < bc; ++b) {
                refused[b] = run.pr[b].refused;
                if (refused[b]) continue;
                std::memcpy(evals + 4 * (size_t)N_EVALS * b, run.pr[b].ev, 32 * N_EVALS);
                if (chal) std::memcpy(chal + 4 * (size_t)N_CHALLENGES * b, run.pr[b].tr.ch, 32 * N_CHALLENGES);
            }
        }
        for (uint32_t b = 0; b < bc; ++b) {
            h_status[b0 + b] = refused[b] ? ZKHIP_ERR_ARG : ZKHIP_OK;
            if (!refused[b]) continue;
            any_refused = true;                                // its outputs are zero; every other proof is what it would be without it
            std::memset(xy + 12 * (size_t)N_POINTS * b, 0, 96 * N_POINTS);
            std::memset(inf + (size_t)N_POINTS * b, 0, N_POINTS);
            std::memset(evals + 4 * (size_t)N_EVALS * b, 0, 32 * N_EVALS);
            if (chal) std::memset(chal + 4 * (size_t)N_CHALLENGES * b, 0, 32 * N_CHALLENGES);
        }
    }
    return any_refused ? ZKHIP_ERR_ARG : ZKHIP_OK;
}

// compute_verifier_challenges (protocol/utils.rs:56-96): host only, no GPU
extern "C" int zkhip_plonk_challenges(const uint64_t* h_points_xy, const uint8_t* h_points_inf, const uint64_t* h_evals, uint64_t* h_challenges) {
    if (!h_points_xy || !h_points_inf || !h_evals || !h_challenges) return ZKHIP_ERR_ARG;
    for (int e = 0; e < N_EVALS; ++e) if (zkhost::fr_geq_p(h_evals + 4 * e)) return ZKHIP_ERR_ARG;
    HFr ch[N_CHALLENGES];
    absorb_challenges_from_proof(h_points_xy, h_points_inf, h_evals, ch);
    std::memcpy(h_challenges, ch, sizeof ch);
    return ZKHIP_OK;
}

// PlonkVerifier::verify (verifier.rs:62-172)
extern "C" int zkhip_plonk_verify(zkhip_ctx* c, size_t n, const uint64_t* h_vk_xy, const uint8_t* h_vk_inf, const uint64_t* h_points_xy,
                                  const uint8_t* h_points_inf, const uint64_t* h_evals, const uint64_t* d_public, const uint64_t* d_g2_xy,
                                  const uint8_t* d_g2_inf, size_t n_g2, uint8_t* h_ok) {
    if (!c || !h_vk_xy || !h_vk_inf || !h_points_xy || !h_points_inf || !h_evals || !d_public || !d_g2_xy || !d_g2_inf || !h_ok) return ZKHIP_ERR_ARG;
    const uint8_t was = *h_ok;
    *h_ok = 0;
    if (!is_pow2(n) || n < 4 || log2_exact(n) > 28) return ZKHIP_ERR_SHAPE;
    if (n_g2 < 2) return ZKHIP_ERR_INDEX;                          // powers_of_tau_in_g2[1] (verifier.rs:34)
    for (int e = 0; e < N_EVALS; ++e) if (zkhost::fr_geq_p(h_evals + 4 * e)) return ZKHIP_ERR_ARG;
    for (int p = 0; p < N_POINTS; ++p) if (!h_points_inf[p] && !g1_valid(h_points_xy + 12 * p)) return ZKHIP_ERR_ARG;
    for (int p = 0; p < 8; ++p) if (!h_vk_inf[p] && !g1_valid(h_vk_xy + 12 * p)) return ZKHIP_ERR_ARG;
    if (c->ws_loans.lent()) { *h_ok = was; return ZKHIP_ERR_BUSY; }      // PI(zeta) and the pairing need the workspace: nothing allocated or launched, *h_ok as it was
    ZK_TRY(c->activate());
    HFr ch[N_CHALLENGES];
    absorb_challenges_from_proof(h_points_xy, h_points_inf, h_evals, ch);
    const HFr zeta = ch[C_ZETA], mu = ch[C_MU];
    // PI(zeta): to_coefficient_poly().evaluate(zeta) on the device
    DevMem tmp;
    const size_t prep_bytes = zkhip_g2_prepared_bytes(2);
    const size_t o_pi = 0, o_g1 = (n * 32 + 255) & ~(size_t)255, o_inf = o_g1 + 256, o_gt = o_inf + 256, o_prep = o_gt + 2 * 576 + 128;
    if (dev_alloc(tmp, o_prep + prep_bytes) != hipSuccess) return ZKHIP_ERR_NOMEM;
    char* base = (char*)tmp.get();
    HFr piz, wn, t1, t2;
    ZK_TRY(zkhip_domain_params((uint64_t)n, wn.l, t1.l, t2.l));
    ZK_TRY(zkhip_domain_transform(c, d_public, n, (uint64_t*)(base + o_pi), log2_exact(n), 1));
    ZK_TRY(zkhip_dense_evaluate(c, (const uint64_t*)(base + o_pi), n, zeta.l, piz.l));
    HFr e[N_EVALS];
    for (int j = 0; j < N_EVALS; ++j) e[j] = h_load(h_evals + 4 * j);
    const HFr az = e[E_A], bz = e[E_B], cz = e[E_C];
    const zkplonk::VerifierScalars sc = zkplonk::verifier_scalars((uint64_t)n, ch, e, piz);     // plonk_scalars.hpp
    const HFr zn = sc.zn, zh = sc.zh, k_acc = sc.k_acc, k_s3 = sc.k_s3, es = sc.es;
    const HFr* nup = sc.nup;
    auto pt = [&](const uint64_t* xy, const uint8_t* inf, int i) { return zkhost::xyzz_from_affine(xy + 12 * i, inf[i] != 0); };
    auto P = [&](int i) { return pt(h_points_xy, h_points_inf, i); };
    auto V = [&](int i) { return pt(h_vk_xy, h_vk_inf, i); };       // q_m, q_l, q_r, q_o, q_c, sigma_1, sigma_2, sigma_3
    using zkhost::xyzz_add;
    Xyzz t_comb = xyzz_add(xyzz_add(P(P_TL), g1_mul(P(P_TM), zn)), g1_mul(P(P_TH), fr_mul(zn, zn)));
    Xyzz d1 = xyzz_add(xyzz_add(xyzz_add(g1_mul(V(0), fr_mul(az, bz)), g1_mul(V(1), az)), xyzz_add(g1_mul(V(2), bz), g1_mul(V(3), cz))), V(4));   // :101-105
    d1 = xyzz_add(d1, g1_mul(P(P_ACC), k_acc));                                                                                                 // :106-114
    d1 = xyzz_add(d1, g1_mul(V(7), h_neg(k_s3)));                                                                                               // :115-122
    d1 = xyzz_add(d1, g1_mul(t_comb, h_neg(zh)));                                                                                               // :123-126
    Xyzz f1 = xyzz_add(d1, xyzz_add(xyzz_add(g1_mul(P(P_AS), nup[1]), g1_mul(P(P_BS), nup[2])),
                                    xyzz_add(g1_mul(P(P_CS), nup[3]), xyzz_add(g1_mul(V(5), nup[4]), g1_mul(V(6), nup[5])))));                    // :134-139
    const Xyzz e1_neg = g1_mul(g1_generator_host(), h_neg(es));                                                                                // :141-150
    const Xyzz left = xyzz_add(P(P_WZ), g1_mul(P(P_WZW), mu));                                                                                 // :157-160
    const Xyzz right = xyzz_add(xyzz_add(g1_mul(P(P_WZ), zeta), g1_mul(P(P_WZW), fr_mul(fr_mul(wn, mu), zeta))), xyzz_add(f1, e1_neg));         // :162-169
    // e(right, G2) and e(left, tau G2): prepared entry 0 is the generator, entry 1 the SRS's powers_of_tau_in_g2[1]
    uint64_t g1[24];
    uint8_t g1_inf[2];
    g1_inf[0] = zkhost::xyzz_to_affine(right, g1) ? 0 : 1;
    g1_inf[1] = zkhost::xyzz_to_affine(left, g1 + 12) ? 0 : 1;
    ZK_HIP(c, hipMemcpyAsync(base + o_g1, g1, sizeof g1, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipMemcpyAsync(base + o_inf, g1_inf, 2, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    ZK_TRY(zkhip_kzg_prepare(c, d_g2_xy + 24, d_g2_inf + 1, 1, base + o_prep));
    ZK_TRY(zkhip_pairing_prepared(c, (const uint64_t*)(base + o_g1), (const uint8_t*)(base + o_inf), base + o_prep, 2, (uint64_t*)(base + o_gt)));
    uint64_t gt[144];
    ZK_HIP(c, hipMemcpyAsync(gt, base + o_gt, sizeof gt, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    *h_ok = std::memcmp(gt, gt + 72, 576) == 0 ? 1 : 0;            // GT has one encoding: left == right (:171)
    return ZKHIP_OK;
}

// ---- the batched verifier ---------------------------------------------------------------------------------------------------------
static_assert(C_BETA == 0 && C_GAMMA == 1 && C_ALPHA == 2 && C_ZETA == 3 && C_NU == 4 && C_MU == 5 && E_A == 0 && E_ZW == 5,
              "plonk_scalars.hpp indexes challenges and evaluations in the ABI's order");
static_assert(zkplonk::VERIFY_TERMS == PV_TERMS && N_POINTS == PV_PROOF_POINTS, "one term table on both sides");

// What every proof of one circuit shares: the eight commitments of vpi (validated once), the prepared lines of [G2, tau G2] and the
// table w^0 .. w^(n-1) of the PI pass.
struct zkhip_plonk_vkey {
    zkhip_ctx* ctx = nullptr;
    size_t n = 0;
    HFr w_n, n_inv;
    DevMem vk_xy, vk_inf, prep, omega;
};

extern "C" int zkhip_plonk_vkey_destroy(zkhip_plonk_vkey* vk) {
    if (!vk) return ZKHIP_OK;
    if (vk->ctx) {
        (void)vk->ctx->activate();
        vk->ctx->drain_streams();       // nothing of this key's may still be read by a kernel
    }
    delete vk;
    return ZKHIP_OK;
}

extern "C" int zkhip_plonk_vkey_create(zkhip_ctx* c, size_t n, const uint64_t* h_vk_xy, const uint8_t* h_vk_inf, const uint64_t* d_g2_xy,
                                       const uint8_t* d_g2_inf, size_t n_g2, zkhip_plonk_vkey** out) {
    if (!c || !h_vk_xy || !h_vk_inf || !d_g2_xy || !d_g2_inf || !out) return ZKHIP_ERR_ARG;
    *out = nullptr;
    if (!is_pow2(n) || n < 4 || log2_exact(n) > 28) return ZKHIP_ERR_SHAPE;
    if (n_g2 < 2) return ZKHIP_ERR_INDEX;                          // powers_of_tau_in_g2[1] (verifier.rs:34)
    ZK_TRY(c->activate());
    std::unique_ptr<zkhip_plonk_vkey> k(new (std::nothrow) zkhip_plonk_vkey());
    if (!k) return ZKHIP_ERR_NOMEM;
    k->ctx = c; k->n = n;
    if (dev_alloc(k->vk_xy, PV_VK_POINTS * 96) != hipSuccess || dev_alloc(k->vk_inf, 256) != hipSuccess ||
        dev_alloc(k->prep, zkhip_g2_prepared_bytes(2)) != hipSuccess || dev_alloc(k->omega, n * 32) != hipSuccess)
        return ZKHIP_ERR_NOMEM;
    HFr t1;
    ZK_TRY(zkhip_domain_params((uint64_t)n, k->w_n.l, t1.l, k->n_inv.l));
    k->n_inv = zkhost::fr_inv(zkhost::fr_from_u64((uint64_t)n));
    uint8_t* d_bad = (uint8_t*)k->vk_inf.get() + 64;               // scratch beside the eight flags
    ZK_HIP(c, hipMemcpyAsync(k->vk_xy.get(), h_vk_xy, PV_VK_POINTS * 96, hipMemcpyHostToDevice, c->stream));
    ZK_HIP(c, hipMemcpyAsync(k->vk_inf.get(), h_vk_inf, PV_VK_POINTS, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(plonk_points_check_kernel, dim3(1), dim3(PV_BLOCK), 0, c->stream, (const uint64_t*)k->vk_xy.get(),
                       (const uint8_t*)k->vk_inf.get(), (size_t)PV_VK_POINTS, d_bad);
    ZK_HIP(c, hipGetLastError());
    bool any = false;
    ZK_TRY(zk_pairing_any_flag(c, d_bad, PV_VK_POINTS, &any));
    if (any) return ZKHIP_ERR_ARG;                                 // a commitment off the curve or outside the subgroup
    ZK_TRY(zk_pairing_prepare_kzg(c, d_g2_xy + 24, d_g2_inf + 1, 1, (uint64_t*)k->prep.get(), d_bad));
    ZK_TRY(powers(c, k->w_n, zkhost::fr_one(), n, (uint64_t*)k->omega.get()));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    *out = k.release();
    return ZKHIP_OK;
}

// PlonkVerifier::verify (verifier.rs:62-172) of `batch` proofs of one circuit: h_ok[b] = 1 verifies, 0 does not, 2 malformed
extern "C" int zkhip_plonk_verify_batch(zkhip_plonk_vkey* vk, size_t batch, const uint64_t* h_points_xy, const uint8_t* h_points_inf,
                                        const uint64_t* h_evals, const uint64_t* const* h_public_ptrs, uint8_t* h_ok, uint64_t* h_pair_xy,
                                        uint8_t* h_pair_inf) {
    if (!vk) return ZKHIP_ERR_ARG;
    if (!batch) return ZKHIP_OK;
    if (!h_points_xy || !h_points_inf || !h_evals || !h_public_ptrs || !h_ok || (!h_pair_xy != !h_pair_inf)) return ZKHIP_ERR_ARG;
    for (size_t b = 0; b < batch; ++b) if (!h_public_ptrs[b]) return ZKHIP_ERR_ARG;
    zkhip_ctx* c = vk->ctx;
    ZK_TRY(c->activate());
    const size_t n = vk->n, n_blocks = (n + PV_PI_ROWS - 1) / PV_PI_ROWS, nt = batch * PV_TERMS;
    if (batch > 65535 || n_blocks > 0x7fffffffu) return ZKHIP_ERR_SHAPE;   // the PI pass puts the proofs on the grid's second axis
    // host: challenges and the scalar table of every well-formed proof (an unreduced evaluation makes a proof malformed: zero scalars)
    std::vector<HFr> scal(nt, zkhost::fr_zero()), zetas(batch, zkhost::fr_zero()), factors(batch, zkhost::fr_zero());
    std::vector<uint8_t> malformed(batch, 0);
    for (size_t b = 0; b < batch; ++b) {
        const uint64_t* ev = h_evals + 4 * N_EVALS * b;
        for (int e = 0; e < N_EVALS; ++e) if (zkhost::fr_geq_p(ev + 4 * e)) malformed[b] = 1;
        if (malformed[b]) continue;
        HFr ch[N_CHALLENGES], e[N_EVALS];
        absorb_challenges_from_proof(h_points_xy + 12 * N_POINTS * b, h_points_inf + N_POINTS * b, ev, ch);
        for (int j = 0; j < N_EVALS; ++j) e[j] = h_load(ev + 4 * j);
        const zkplonk::VerifierScalars sc = zkplonk::verifier_scalars((uint64_t)n, ch, e, zkhost::fr_zero());   // es + PI(zeta): the device adds PI(zeta) to -es
        zkplonk::verifier_term_table(sc, ch, e, vk->w_n, &scal[PV_TERMS * b]);
        zetas[b] = ch[C_ZETA];
        factors[b] = fr_mul(sc.zh, vk->n_inv);
    }
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_points = carve(batch * N_POINTS * 96), o_pinf = carve(batch * N_POINTS), o_scal = carve(nt * 32), o_zeta = carve(batch * 32);
    const size_t o_fact = carve(batch * 32), o_cols = carve(batch * 8), o_part = carve(batch * n_blocks * 32), o_hit = carve(batch * 8);
    const size_t o_terms = carve(nt * 192), o_pxy = carve(batch * 2 * 96), o_pairinf = carve(batch * 2), o_oxy = carve(batch * 2 * 96);
    const size_t o_oinf = carve(batch * 2), o_f = carve(batch * 2 * 576), o_bad = carve(nt), o_ok = carve(batch);
    ZK_TRY(c->reserve_ws(off));
    char* ws = (char*)c->ws.ptr;
    auto up = [&](size_t o, const void* h, size_t bytes) { return hipMemcpyAsync(ws + o, h, bytes, hipMemcpyHostToDevice, c->stream); };
    ZK_HIP(c, up(o_points, h_points_xy, batch * N_POINTS * 96));
    ZK_HIP(c, up(o_pinf, h_points_inf, batch * N_POINTS));
    ZK_HIP(c, up(o_scal, scal.data(), nt * 32));
    ZK_HIP(c, up(o_zeta, zetas.data(), batch * 32));
    ZK_HIP(c, up(o_fact, factors.data(), batch * 32));
    ZK_HIP(c, up(o_cols, h_public_ptrs, batch * 8));
    ZK_HIP(c, hipMemsetAsync(ws + o_hit, 0, batch * 8, c->stream));
    const uint64_t* const* d_cols = (const uint64_t* const*)(ws + o_cols);
    uint64_t* d_scal = (uint64_t*)(ws + o_scal);
    uint8_t* d_bad = (uint8_t*)(ws + o_bad);
    const unsigned per_proof_grid = (unsigned)((batch + PV_BLOCK - 1) / PV_BLOCK);
    {
        ProfScope ps(c, "plonk_verify_pi", 64.0 * (double)n * (double)batch);
        hipLaunchKernelGGL(plonk_pi_kernel, dim3((unsigned)n_blocks, (unsigned)batch), dim3(PV_PI_T), 0, c->stream, d_cols, (const uint64_t*)vk->omega.get(),
                           (const uint64_t*)(ws + o_zeta), n, (uint64_t*)(ws + o_part), (unsigned long long*)(ws + o_hit));
        hipLaunchKernelGGL(plonk_pi_finish_kernel, dim3(per_proof_grid), dim3(PV_BLOCK), 0, c->stream, d_cols, (const uint64_t*)(ws + o_part),
                           (const unsigned long long*)(ws + o_hit), (const uint64_t*)(ws + o_fact), batch, n_blocks, d_scal + 4 * PV_TERM_G,
                           (size_t)PV_TERMS, (uint64_t*)nullptr);
    }
    {
        ProfScope ps(c, "plonk_verify_terms", 192.0 * (double)nt);
        hipLaunchKernelGGL(plonk_terms_kernel, dim3((unsigned)((nt + PV_BLOCK - 1) / PV_BLOCK)), dim3(PV_BLOCK), 0, c->stream, (const uint64_t*)vk->vk_xy.get(),
                           (const uint8_t*)vk->vk_inf.get(), (const uint64_t*)(ws + o_points), (const uint8_t*)(ws + o_pinf), (const uint64_t*)d_scal, batch,
                           (uint64_t*)(ws + o_terms), d_bad);
    }
    {
        ProfScope ps(c, "plonk_verify_combine", 192.0 * (double)nt);
        hipLaunchKernelGGL(plonk_combine_kernel, dim3(per_proof_grid), dim3(PV_BLOCK), 0, c->stream, (const uint64_t*)(ws + o_terms), (const uint8_t*)d_bad, batch,
                           (uint64_t*)(ws + o_pxy), (uint8_t*)(ws + o_pairinf), (uint64_t*)(ws + o_oxy), (uint8_t*)(ws + o_oinf));
    }
    ZK_HIP(c, hipGetLastError());
    // e(right, G2) e(-left, tau G2) == 1: two Miller loops, one product, one final exponentiation per proof
    ZK_TRY(zk_pairing_groups(c, (const uint64_t*)(ws + o_pxy), (const uint8_t*)(ws + o_pairinf), (const uint64_t*)vk->prep.get(), 2, batch, 2,
                             (uint64_t*)(ws + o_f), (uint8_t*)(ws + o_ok)));
    std::vector<uint8_t> bad(nt);
    ZK_HIP(c, hipMemcpyAsync(h_ok, ws + o_ok, batch, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipMemcpyAsync(bad.data(), d_bad, nt, hipMemcpyDeviceToHost, c->stream));
    if (h_pair_xy) {
        ZK_HIP(c, hipMemcpyAsync(h_pair_xy, ws + o_oxy, batch * 2 * 96, hipMemcpyDeviceToHost, c->stream));
        ZK_HIP(c, hipMemcpyAsync(h_pair_inf, ws + o_oinf, batch * 2, hipMemcpyDeviceToHost, c->stream));
    }
    ZK_HIP(c, hipStreamSynchronize(c->stream));                    // the call's one wait: verdicts, flags and pair points
    bool any = false;
    for (size_t b = 0; b < batch; ++b) {
        for (int j = 0; j < PV_TERMS; ++j) if (bad[PV_TERMS * b + j]) malformed[b] = 1;
        if (malformed[b]) { h_ok[b] = 2; any = true; }
    }
    return any ? ZKHIP_ERR_ARG : ZKHIP_OK;
}
