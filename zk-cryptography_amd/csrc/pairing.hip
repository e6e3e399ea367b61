// pairing.hip -- C-ABI entry points of the KZG verifier: G2 SRS, prepared lines, the BLS12-381 pairing and batched
// verification of multilinear and univariate openings.  gfx950 only; no CPU fallback.
#include "../../include/zkhip.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "pairing.hpp"
#include "pairing_internal.hpp"
#include "srs_kernels.hpp"

using namespace zk;

namespace {

constexpr int PAIR_BLOCK = 64;
inline unsigned pair_grid(size_t n) { return (unsigned)((n + PAIR_BLOCK - 1) / PAIR_BLOCK); }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// out[i] = scalars[i] * G2 (Group::mul_bigint, trusted_setup.rs:37-45 / univariate_kzg.rs:18-35), affine
__global__ __launch_bounds__(PAIR_BLOCK) void g2_srs_kernel(const uint64_t* __restrict__ scalars, size_t n,
                                                            uint64_t* __restrict__ out_xy, uint8_t* __restrict__ out_inf) {
    const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Fr k = load_fr(scalars, i).from_mont();
    G2Affine a;
    const bool finite = g2_to_affine(g2_mul<8>(g2_generator(), k.l), a);
    store_g2(out_xy, i, a);
    out_inf[i] = finite ? 0 : 1;
}

// tau^i, i = 0..n-1 (tau.pow([i]), univariate_kzg.rs:26)
__global__ __launch_bounds__(PAIR_BLOCK) void g2_power_scalars_kernel(const uint64_t* __restrict__ tau, size_t n,
                                                                      uint64_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Fr t = load_fr(tau, 0);
    Fr acc = Fr::one();
    for (int b = 63; b >= 0; --b) {
        acc = acc * acc;
        if ((i >> b) & 1) acc = acc * t;
    }
    store_fr(out, i, acc);
}

// The 68 Miller-loop lines of each G2 point (entry i of `prep`, PREP_STRIDE_U64 words).  gen_first: entry 0 is the generator's and
// entry i >= 1 that of input point i - 1 (the layout zkhip_kzg_prepare writes).  bad[i] = 1: finite and not a valid G2 element (g2_point_valid).
__global__ __launch_bounds__(PAIR_BLOCK) void g2_prepare_kernel(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf,
                                                                size_t n_entries, int gen_first, uint64_t* __restrict__ prep,
                                                                uint8_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (i >= n_entries) return;
    uint64_t* out = prep + PREP_STRIDE_U64 * i;
    bool at_inf = false, ok = true;
    G2Affine q;
    if (gen_first && i == 0) {
        q = g2_generator();
    } else {
        const size_t j = gen_first ? i - 1 : i;
        at_inf = inf && inf[j];
        q = load_g2(xy, j);
        if (!at_inf) ok = g2_point_valid(q);
    }
    bad[i] = ok ? 0 : 1;
    out[PAIR_LINES * PREP_LINE_U64] = at_inf || !ok ? 1 : 0;
    if (at_inf || !ok) return;
    Fq2 t[3] = {q.x, q.y, Fq2::one()};
    int k = 0;
    for (int b = 62; b >= 0; --b) {
        Line l;
        g2_double_step(t, l);
        store_line(out + PREP_LINE_U64 * k++, l);
        if ((PAIR_X_ABS >> b) & 1) {
            g2_add_step(t, q, l);
            store_line(out + PREP_LINE_U64 * k++, l);
        }
    }
}

// G1 / G2 inputs of zkhip_pairing: bad[i] = 1 when a finite point is off its curve, outside the subgroup or has an unreduced coordinate
__global__ __launch_bounds__(PAIR_BLOCK) void pairing_check_kernel(const uint64_t* __restrict__ g1_xy, const uint8_t* __restrict__ g1_inf,
                                                                   const uint64_t* __restrict__ g2_xy, const uint8_t* __restrict__ g2_inf,
                                                                   size_t n, uint8_t* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    if (!(g1_inf && g1_inf[i])) {
        const G1Affine p = load_affine(g1_xy, i);
        ok = g1_point_valid(p);
    }
    if (ok && g2_xy && !(g2_inf && g2_inf[i])) {
        const G2Affine q = load_g2(g2_xy, i);
        ok = g2_point_valid(q);
    }
    bad[i] = ok ? 0 : 1;
}

// One Miller loop per pair k: G1 point k with G2 point k % q_mod (q_mod = 0: point k), either prepared lines (prep) or affine (q_xy / q_inf).
// A point at infinity on either side gives 1.
__global__ __launch_bounds__(PAIR_BLOCK) void miller_loop_kernel(const uint64_t* __restrict__ p_xy, const uint8_t* __restrict__ p_inf,
                                                                 const uint64_t* __restrict__ q_xy, const uint8_t* __restrict__ q_inf,
                                                                 const uint64_t* __restrict__ prep, size_t n_pairs, size_t q_mod,
                                                                 uint64_t* __restrict__ out_f) {
    const size_t k = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (k >= n_pairs) return;
    const size_t j = q_mod ? k % q_mod : k;
    Fq12 f = f12_one();
    const uint64_t* lines = prep ? prep + PREP_STRIDE_U64 * j : nullptr;
    const bool q_at_inf = prep ? lines[PAIR_LINES * PREP_LINE_U64] != 0 : (q_inf && q_inf[j]);
    if (!(p_inf && p_inf[k]) && !q_at_inf) {
        const G1Affine p = load_affine(p_xy, k);
        const G2Affine q = prep ? G2Affine{Fq2::zero(), Fq2::zero()} : load_g2(q_xy, j);
        miller_loop(f, p, q, lines);
    }
    store_f12(out_f + 72 * k, f);
}

// Product tree over the m Miller-loop values of every group: f[g m + j] *= f[g m + j + stride] for j = 0 mod 2 stride
__global__ __launch_bounds__(PAIR_BLOCK) void f12_product_kernel(uint64_t* __restrict__ f, size_t n_groups, size_t m, size_t stride) {
    const size_t per = (m + 2 * stride - 1) / (2 * stride);
    const size_t t = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (t >= n_groups * per) return;
    const size_t g = t / per, j = (t % per) * 2 * stride;
    if (j + stride >= m) return;
    Fq12 a, b;
    load_f12(f + 72 * (g * m + j), a);
    load_f12(f + 72 * (g * m + j + stride), b);
    f12_mul(a, a, b);
    store_f12(f + 72 * (g * m + j), a);
}

// One final exponentiation per group (its product sits at f[g m]): the GT value (out_gt) and / or the verdict "== 1" (out_ok)
__global__ __launch_bounds__(PAIR_BLOCK) void final_exp_kernel(const uint64_t* __restrict__ f, size_t n_groups, size_t m,
                                                               uint64_t* __restrict__ out_gt, uint8_t* __restrict__ out_ok) {
    const size_t g = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    Fq12 v;
    load_f12(f + 72 * g * m, v);
    final_exponentiation(v);
    if (out_gt) store_f12(out_gt + 72 * g, v);
    if (out_ok) out_ok[g] = f12_is_one(v) ? 1 : 0;
}

// Per opening b and term j (m = n + 1 terms):  j = 0: C - v G1;  j >= 1: z_j pi_j (XYZZ, summed by kzg_combine_kernel), and the
// pairing's G1 argument -pi_j of that term.  bad[b m + j] = 1: C / pi_j finite and off the curve, outside the subgroup or with an unreduced
// coordinate, or v / z_j not a reduced field element.  A refused term contributes the identity: none of its limbs reaches a product.
__global__ __launch_bounds__(PAIR_BLOCK) void kzg_terms_kernel(const uint64_t* __restrict__ commits, const uint8_t* __restrict__ commits_inf,
                                                               const uint64_t* __restrict__ evals, const uint64_t* __restrict__ points,
                                                               const uint64_t* __restrict__ proofs, const uint8_t* __restrict__ proofs_inf,
                                                               size_t batch, size_t n, uint64_t* __restrict__ terms,
                                                               uint64_t* __restrict__ pair_xy, uint8_t* __restrict__ pair_inf,
                                                               uint8_t* __restrict__ bad) {
    const size_t m = n + 1;
    const size_t t = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (t >= batch * m) return;
    const size_t b = t / m, j = t % m;
    const bool at_inf = j == 0 ? commits_inf[b] != 0 : proofs_inf[b * n + j - 1] != 0;
    const G1Affine pt = j == 0 ? load_affine(commits, b) : load_affine(proofs, b * n + j - 1);
    const Fr k = j == 0 ? load_fr(evals, b) : load_fr(points, b * n + j - 1);
    const bool ok = fr_is_reduced(k) && (at_inf || g1_point_valid(pt));
    bad[t] = ok ? 0 : 1;
    G1Xyzz acc = G1Xyzz::identity();
    if (j == 0) {
        if (ok) {
            acc = g1_mul<8>(g1_generator(), k.from_mont().l, true);     // -v G1
            if (!at_inf) g1_madd(acc, pt, false);
        }
    } else {
        if (ok && !at_inf) acc = g1_mul<8>(pt, k.from_mont().l, false);
        store_fq(pair_xy + 12 * t, ok ? pt.x : Fq::zero());
        store_fq(pair_xy + 12 * t + 6, ok ? pt.y.neg() : Fq::zero());
        pair_inf[t] = at_inf || !ok ? 1 : 0;
    }
    store_xyzz(terms, t, acc);
}
// pair point (b, 0) = sum of the opening's m terms, affine
__global__ __launch_bounds__(PAIR_BLOCK) void kzg_combine_kernel(const uint64_t* __restrict__ terms, size_t batch, size_t m,
                                                                 uint64_t* __restrict__ pair_xy, uint8_t* __restrict__ pair_inf) {
    const size_t b = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
    if (b >= batch) return;
    G1Xyzz acc = load_xyzz(terms, b * m);
    for (size_t j = 1; j < m; ++j) g1_add(acc, load_xyzz(terms, b * m + j));
    if (acc.is_identity()) {
        store_fq(pair_xy + 12 * b * m, Fq::zero());
        store_fq(pair_xy + 12 * b * m + 6, Fq::zero());
        pair_inf[b * m] = 1;
        return;
    }
    const Fq inv = pair_fq_inverse(fq_mul(acc.zz, acc.zzz));
    store_fq(pair_xy + 12 * b * m, fq_mul(acc.x, fq_mul(inv, acc.zzz)));
    store_fq(pair_xy + 12 * b * m + 6, fq_mul(acc.y, fq_mul(inv, acc.zz)));
    pair_inf[b * m] = 0;
}

// Miller loops of n_groups x m pairs (G2 point k % q_mod, or k for q_mod = 0), the product tree and the final exponentiations.
// f: n_groups * m * 72 words.
int pairing_groups(zkhip_ctx* c, const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* q_xy, const uint8_t* q_inf,
                   const uint64_t* prep, size_t q_mod, size_t n_groups, size_t m, uint64_t* f, uint64_t* out_gt, uint8_t* out_ok) {
    const size_t n_pairs = n_groups * m;
    {
        ProfScope ps(c, "pairing_miller_loops", 576.0 * (double)n_pairs);
        hipLaunchKernelGGL(miller_loop_kernel, dim3(pair_grid(n_pairs)), dim3(PAIR_BLOCK), 0, c->stream, p_xy, p_inf, q_xy, q_inf, prep,
                           n_pairs, q_mod, f);
    }
    for (size_t stride = 1; stride < m; stride *= 2) {
        const size_t per = (m + 2 * stride - 1) / (2 * stride);
        hipLaunchKernelGGL(f12_product_kernel, dim3(pair_grid(n_groups * per)), dim3(PAIR_BLOCK), 0, c->stream, f, n_groups, m, stride);
    }
    {
        ProfScope ps(c, "pairing_final_exp", 576.0 * (double)n_groups);
        hipLaunchKernelGGL(final_exp_kernel, dim3(pair_grid(n_groups)), dim3(PAIR_BLOCK), 0, c->stream, f, n_groups, m, out_gt, out_ok);
    }
    ZK_HIP(c, hipGetLastError());
    return ZKHIP_OK;
}

// copy n flag bytes back, wait, and tell whether any is set
int any_flag(zkhip_ctx* c, const uint8_t* d_flags, size_t n, bool* any) {
    std::vector<uint8_t> h(n ? n : 1);
    if (n) ZK_HIP(c, hipMemcpyAsync(h.data(), d_flags, n, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    *any = false;
    for (size_t i = 0; i < n; ++i) *any |= h[i] != 0;
    return ZKHIP_OK;
}

// prepared lines of [G2, q_0 .. q_{n-1}] (gen_first) or [q_0 .. q_{n-1}] into d_prep; ERR_ARG on an invalid point
int prepare(zkhip_ctx* c, const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int gen_first, uint64_t* d_prep, uint8_t* d_bad) {
    const size_t entries = n + (gen_first ? 1 : 0);
    if (!entries) return ZKHIP_OK;
    hipLaunchKernelGGL(g2_prepare_kernel, dim3(pair_grid(entries)), dim3(PAIR_BLOCK), 0, c->stream, d_xy, d_inf, entries, gen_first,
                       d_prep, d_bad);
    ZK_HIP(c, hipGetLastError());
    bool any = false;
    ZK_TRY(any_flag(c, d_bad, entries, &any));
    return any ? ZKHIP_ERR_ARG : ZKHIP_OK;
}

// Shared body of the two batched verifiers: n G2 powers per opening (n = n_vars, or 1 = tau G2 for univariate).
int verify_batch(zkhip_ctx* c, size_t batch, size_t n, const uint64_t* h_commits_xy, const uint8_t* h_commits_inf,
                 const uint64_t* h_evals, const uint64_t* h_points, const uint64_t* h_proofs_xy, const uint8_t* h_proofs_inf,
                 const uint64_t* d_g2_xy, const uint8_t* d_g2_inf, const void* d_prepared, uint8_t* h_ok) {
    if (!batch) return ZKHIP_OK;
    if (c->ws_loans.lent()) return ZKHIP_ERR_BUSY;      // refused like a null argument: nothing launched, h_ok untouched
    std::memset(h_ok, 0, batch);              // an error before the verdicts are known leaves none standing
    ZK_TRY(c->activate());
    const size_t m = n + 1, np = batch * m;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    const size_t o_commits = carve(batch * 96), o_cinf = carve(batch), o_evals = carve(batch * 32), o_points = carve(batch * n * 32);
    const size_t o_proofs = carve(batch * n * 96), o_pinf = carve(batch * n), o_terms = carve(np * 192), o_pxy = carve(np * 96);
    const size_t o_pairinf = carve(np), o_f = carve(np * 576), o_bad = carve(np + m), o_ok = carve(batch);
    const size_t o_prep = carve(d_prepared ? 0 : m * PREP_STRIDE_U64 * 8);
    ZK_TRY(c->reserve_ws(off));
    char* ws = (char*)c->ws.ptr;
    auto up = [&](size_t o, const void* h, size_t bytes) {
        return bytes ? hipMemcpyAsync(ws + o, h, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    ZK_HIP(c, up(o_commits, h_commits_xy, batch * 96));
    ZK_HIP(c, up(o_cinf, h_commits_inf, batch));
    ZK_HIP(c, up(o_evals, h_evals, batch * 32));
    ZK_HIP(c, up(o_points, h_points, batch * n * 32));
    ZK_HIP(c, up(o_proofs, h_proofs_xy, batch * n * 96));
    ZK_HIP(c, up(o_pinf, h_proofs_inf, batch * n));
    uint8_t* bad = (uint8_t*)(ws + o_bad);
    const uint64_t* prep = (const uint64_t*)d_prepared;
    if (!prep) {
        ZK_TRY(prepare(c, d_g2_xy, d_g2_inf, n, 1, (uint64_t*)(ws + o_prep), bad));
        prep = (const uint64_t*)(ws + o_prep);
    }
    uint64_t* pair_xy = (uint64_t*)(ws + o_pxy);
    uint8_t* pair_inf = (uint8_t*)(ws + o_pairinf);
    hipLaunchKernelGGL(kzg_terms_kernel, dim3(pair_grid(np)), dim3(PAIR_BLOCK), 0, c->stream, (const uint64_t*)(ws + o_commits),
                       (const uint8_t*)(ws + o_cinf), (const uint64_t*)(ws + o_evals), (const uint64_t*)(ws + o_points),
                       (const uint64_t*)(ws + o_proofs), (const uint8_t*)(ws + o_pinf), batch, n, (uint64_t*)(ws + o_terms), pair_xy,
                       pair_inf, bad);
    hipLaunchKernelGGL(kzg_combine_kernel, dim3(pair_grid(batch)), dim3(PAIR_BLOCK), 0, c->stream, (const uint64_t*)(ws + o_terms), batch,
                       m, pair_xy, pair_inf);
    ZK_HIP(c, hipGetLastError());
    uint8_t* d_ok = (uint8_t*)(ws + o_ok);
    ZK_TRY(pairing_groups(c, pair_xy, pair_inf, nullptr, nullptr, prep, m, batch, m, (uint64_t*)(ws + o_f), nullptr, d_ok));
    ZK_HIP(c, hipMemcpyAsync(h_ok, d_ok, batch, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> h_bad(np);
    ZK_HIP(c, hipMemcpyAsync(h_bad.data(), bad, np, hipMemcpyDeviceToHost, c->stream));
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    bool any = false;
    for (size_t t = 0; t < np; ++t) {
        if (!h_bad[t]) continue;
        any = true;
        h_ok[t / m] = 0;                      // an opening with a refused input never verifies; the others keep their verdicts
    }
    return any ? ZKHIP_ERR_ARG : ZKHIP_OK;
}

}  // namespace

// ---- pairing_internal.hpp: the three helpers above for plonk.hip ------------------------------------------------------------------------
int zk_pairing_groups(zkhip_ctx* c, const uint64_t* d_p_xy, const uint8_t* d_p_inf, const uint64_t* d_prep, size_t q_mod, size_t n_groups, size_t m,
                      uint64_t* d_f, uint8_t* d_out_ok) {
    return pairing_groups(c, d_p_xy, d_p_inf, nullptr, nullptr, d_prep, q_mod, n_groups, m, d_f, nullptr, d_out_ok);
}
int zk_pairing_prepare_kzg(zkhip_ctx* c, const uint64_t* d_xy, const uint8_t* d_inf, size_t n, uint64_t* d_prep, uint8_t* d_bad) {
    return prepare(c, d_xy, d_inf, n, 1, d_prep, d_bad);
}
int zk_pairing_any_flag(zkhip_ctx* c, const uint8_t* d_flags, size_t n, bool* any) { return any_flag(c, d_flags, n, any); }

extern "C" int zkhip_srs_multilinear_g2(zkhip_ctx* c, const uint64_t* h_tau, uint32_t n_vars, uint64_t* d_out_xy, uint8_t* d_out_inf) {
    if (!c || (n_vars && (!h_tau || !d_out_xy || !d_out_inf))) return ZKHIP_ERR_ARG;
    if (!n_vars) return ZKHIP_OK;
    ZK_TRY(c->activate());
    ZK_TRY(c->reserve_ws(32 * (size_t)n_vars));
    uint64_t* d_s = (uint64_t*)c->ws.ptr;
    ZK_HIP(c, hipMemcpyAsync(d_s, h_tau, 32 * (size_t)n_vars, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(g2_srs_kernel, dim3(pair_grid(n_vars)), dim3(PAIR_BLOCK), 0, c->stream, d_s, (size_t)n_vars, d_out_xy, d_out_inf);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipStreamSynchronize(c->stream));      // the host scalars are read by the copy above
    return ZKHIP_OK;
}

extern "C" int zkhip_srs_univariate_g2(zkhip_ctx* c, const uint64_t* h_tau, size_t max_degree, uint64_t* d_out_xy, uint8_t* d_out_inf) {
    if (!c || !h_tau || !d_out_xy || !d_out_inf) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    const size_t n = max_degree + 1;
    ZK_TRY(c->reserve_ws(256 + 32 * n));
    uint64_t* d_tau = (uint64_t*)c->ws.ptr;
    uint64_t* d_s = d_tau + 32;
    ZK_HIP(c, hipMemcpyAsync(d_tau, h_tau, 32, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(g2_power_scalars_kernel, dim3(pair_grid(n)), dim3(PAIR_BLOCK), 0, c->stream, d_tau, n, d_s);
    hipLaunchKernelGGL(g2_srs_kernel, dim3(pair_grid(n)), dim3(PAIR_BLOCK), 0, c->stream, d_s, n, d_out_xy, d_out_inf);
    ZK_HIP(c, hipGetLastError());
    ZK_HIP(c, hipStreamSynchronize(c->stream));
    return ZKHIP_OK;
}

extern "C" size_t zkhip_g2_prepared_bytes(size_t n) { return n * PREP_STRIDE_U64 * 8; }

extern "C" int zkhip_g2_prepare(zkhip_ctx* c, const uint64_t* d_g2_xy, const uint8_t* d_g2_inf, size_t n, void* d_prepared) {
    if (!c || (n && (!d_g2_xy || !d_prepared))) return ZKHIP_ERR_ARG;
    if (!n) return ZKHIP_OK;
    ZK_TRY(c->activate());
    ZK_TRY(c->reserve_ws(n));
    return prepare(c, d_g2_xy, d_g2_inf, n, 0, (uint64_t*)d_prepared, (uint8_t*)c->ws.ptr);
}

extern "C" int zkhip_kzg_prepare(zkhip_ctx* c, const uint64_t* d_g2_xy, const uint8_t* d_g2_inf, size_t n, void* d_prepared) {
    if (!c || !d_prepared || (n && !d_g2_xy)) return ZKHIP_ERR_ARG;
    ZK_TRY(c->activate());
    ZK_TRY(c->reserve_ws(n + 1));
    return prepare(c, d_g2_xy, d_g2_inf, n, 1, (uint64_t*)d_prepared, (uint8_t*)c->ws.ptr);
}

static int pairing_common(zkhip_ctx* c, const uint64_t* d_g1_xy, const uint8_t* d_g1_inf, const uint64_t* d_g2_xy,
                          const uint8_t* d_g2_inf, const void* d_prepared, size_t n, uint64_t* d_out_gt) {
    if (!c || (n && (!d_g1_xy || !d_out_gt || (!d_g2_xy && !d_prepared)))) return ZKHIP_ERR_ARG;
    if (!n) return ZKHIP_OK;
    ZK_TRY(c->activate());
    const size_t o_bad = align256(n * 576);
    ZK_TRY(c->reserve_ws(o_bad + n));
    uint64_t* f = (uint64_t*)c->ws.ptr;
    uint8_t* bad = (uint8_t*)c->ws.ptr + o_bad;
    hipLaunchKernelGGL(pairing_check_kernel, dim3(pair_grid(n)), dim3(PAIR_BLOCK), 0, c->stream, d_g1_xy, d_g1_inf,
                       d_prepared ? nullptr : d_g2_xy, d_g2_inf, n, bad);
    ZK_TRY(pairing_groups(c, d_g1_xy, d_g1_inf, d_g2_xy, d_g2_inf, (const uint64_t*)d_prepared, 0, n, 1, f, d_out_gt, nullptr));
    bool any = false;
    ZK_TRY(any_flag(c, bad, n, &any));
    return any ? ZKHIP_ERR_ARG : ZKHIP_OK;
}

extern "C" int zkhip_pairing(zkhip_ctx* c, const uint64_t* d_g1_xy, const uint8_t* d_g1_inf, const uint64_t* d_g2_xy,
                             const uint8_t* d_g2_inf, size_t n, uint64_t* d_out_gt) {
    if (n && !d_g2_xy) return ZKHIP_ERR_ARG;
    return pairing_common(c, d_g1_xy, d_g1_inf, d_g2_xy, d_g2_inf, nullptr, n, d_out_gt);
}

extern "C" int zkhip_pairing_prepared(zkhip_ctx* c, const uint64_t* d_g1_xy, const uint8_t* d_g1_inf, const void* d_prepared, size_t n,
                                      uint64_t* d_out_gt) {
    if (n && !d_prepared) return ZKHIP_ERR_ARG;
    return pairing_common(c, d_g1_xy, d_g1_inf, nullptr, nullptr, d_prepared, n, d_out_gt);
}

extern "C" int zkhip_kzg_verify_batch(zkhip_ctx* c, size_t batch, uint32_t n_vars, const uint64_t* h_commits_xy,
                                      const uint8_t* h_commits_inf, const uint64_t* h_evals, const uint64_t* h_points,
                                      const uint64_t* h_proofs_xy, const uint8_t* h_proofs_inf, const uint64_t* d_g2_xy,
                                      const uint8_t* d_g2_inf, size_t n_g2, const void* d_prepared, uint8_t* h_ok) {
    if (!c || (batch && (!h_commits_xy || !h_commits_inf || !h_evals || !h_ok))) return ZKHIP_ERR_ARG;
    if (batch && n_vars && (!h_points || !h_proofs_xy || !h_proofs_inf)) return ZKHIP_ERR_ARG;
    if (!d_prepared && n_g2 && !d_g2_xy) return ZKHIP_ERR_ARG;
    if (n_g2 != n_vars) return ZKHIP_ERR_SHAPE;      // sum_pairing_results' assert_eq! (utils.rs:49-50)
    return verify_batch(c, batch, n_vars, h_commits_xy, h_commits_inf, h_evals, h_points, h_proofs_xy, h_proofs_inf, d_g2_xy, d_g2_inf,
                        d_prepared, h_ok);
}

extern "C" int zkhip_univariate_kzg_verify_batch(zkhip_ctx* c, size_t batch, const uint64_t* h_commits_xy, const uint8_t* h_commits_inf,
                                                 const uint64_t* h_evals, const uint64_t* h_points, const uint64_t* h_proofs_xy,
                                                 const uint8_t* h_proofs_inf, const uint64_t* d_g2_xy, const uint8_t* d_g2_inf,
                                                 size_t n_g2, const void* d_prepared, uint8_t* h_ok) {
    if (!c || (batch && (!h_commits_xy || !h_commits_inf || !h_evals || !h_points || !h_proofs_xy || !h_proofs_inf || !h_ok)))
        return ZKHIP_ERR_ARG;
    if (n_g2 < 2) return ZKHIP_ERR_INDEX;            // powers_of_tau_in_g2[1] (univariate_kzg.rs:101)
    if (!d_prepared && !d_g2_xy) return ZKHIP_ERR_ARG;
    return verify_batch(c, batch, 1, h_commits_xy, h_commits_inf, h_evals, h_points, h_proofs_xy, h_proofs_inf,
                        d_g2_xy ? d_g2_xy + 24 : nullptr, d_g2_inf ? d_g2_inf + 1 : nullptr, d_prepared, h_ok);
}
