// plonk_scalars.hpp -- the scalar algebra of PlonkVerifier::verify (plonk/src/protocol/verifier.rs:62-172), host only.
//
// One function computes every field element the verifier's G1 combination needs from the six challenges and the proof's six
// evaluations; zkhip_plonk_verify and zkhip_plonk_verify_batch both call it.  PI(zeta) enters exactly one value, linearly:
// es = mu z_w - r0 + sum nu^j e_j with r0 = PI(zeta) - (..), so a caller that passes PI(zeta) = 0 gets es + PI(zeta) and adds
// PI(zeta) to -es where it has it (the batch does that on the device).  No HIP in this file: tests/cpp/plonk_scalars_sanitize.cpp
// builds it with a host compiler.
#pragma once
#include <cstdint>
#include <cstring>

#include "host_fr.hpp"

namespace zkplonk {

using HFr = zkhost::Fr;

inline bool h_is_zero(const HFr& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
inline HFr h_neg(const HFr& a) { return zkhost::fr_sub(zkhost::fr_zero(), a); }
inline HFr h_pow(HFr a, uint64_t e) {
    HFr acc = zkhost::fr_one();
    for (; e; e >>= 1) { if (e & 1) acc = zkhost::fr_mul(acc, a); a = zkhost::fr_mul(a, a); }
    return acc;
}
// L_1(zeta) = (zeta^n - 1) / (n (zeta - 1)); at zeta = 1 the polynomial with all coefficients 1/n gives 1
inline HFr l1_at(const HFr& zeta, const HFr& zh_zeta, uint64_t n) {
    const HFr d = zkhost::fr_sub(zeta, zkhost::fr_one());
    if (h_is_zero(d)) return zkhost::fr_one();
    return zkhost::fr_mul(zh_zeta, zkhost::fr_inv(zkhost::fr_mul(zkhost::fr_from_u64(n), d)));
}

// challenges beta, gamma, alpha, zeta, nu, mu; evaluations a, b, c, sigma1, sigma2, w_accumulator (the ABI's orders)
struct VerifierScalars {
    HFr zn, zh;          // zeta^n, Z_H(zeta) = zeta^n - 1
    HFr k_acc, k_s3;     // the accumulator commitment's scalar (:106-114); sigma_3's is -k_s3 (:115-122)
    HFr nup[6];          // nu^0 .. nu^5
    HFr es;              // the generator's scalar is -es (:141-150)
};

inline VerifierScalars verifier_scalars(uint64_t n, const HFr* ch, const HFr* e, const HFr& piz) {
    using zkhost::fr_add; using zkhost::fr_mul; using zkhost::fr_sub;
    const HFr beta = ch[0], gamma = ch[1], alpha = ch[2], zeta = ch[3], nu = ch[4], mu = ch[5];
    const HFr az = e[0], bz = e[1], cz = e[2], s1z = e[3], s2z = e[4], zwz = e[5];
    VerifierScalars s;
    const HFr a2 = fr_mul(alpha, alpha);
    s.zn = h_pow(zeta, n);
    s.zh = fr_sub(s.zn, zkhost::fr_one());
    const HFr l1z = l1_at(zeta, s.zh, n);
    const HFr fa1 = fr_add(fr_add(az, fr_mul(s1z, beta)), gamma), fb1 = fr_add(fr_add(bz, fr_mul(s2z, beta)), gamma);
    const HFr r0 = fr_sub(fr_sub(piz, fr_mul(l1z, a2)), fr_mul(alpha, fr_mul(fr_mul(fa1, fb1), fr_mul(fr_add(cz, gamma), zwz))));   // :82-88
    const HFr bzeta = fr_mul(beta, zeta);
    s.k_acc = fr_add(fr_add(fr_mul(fr_mul(fr_mul(fr_add(fr_add(az, bzeta), gamma), fr_add(fr_add(bz, fr_add(bzeta, bzeta)), gamma)),
                                          fr_add(fr_add(cz, fr_add(bzeta, fr_add(bzeta, bzeta))), gamma)), alpha), fr_mul(l1z, a2)), mu);
    s.k_s3 = fr_mul(fr_mul(fr_mul(fa1, fb1), fr_mul(alpha, beta)), zwz);
    s.nup[0] = zkhost::fr_one();
    for (int j = 1; j < 6; ++j) s.nup[j] = fr_mul(s.nup[j - 1], nu);
    s.es = fr_sub(fr_mul(mu, zwz), r0);
    const HFr opened[5] = {az, bz, cz, s1z, s2z};
    for (int j = 0; j < 5; ++j) s.es = fr_add(s.es, fr_mul(s.nup[j + 1], opened[j]));
    return s;
}

// The scalars of the batch's twenty G1 terms in the order of plonk_verify_kernels.hpp, Montgomery form.  wn: the root of unity of the
// group of order n.  With `s` computed for PI(zeta) = 0, entry 17 lacks + PI(zeta).
constexpr int VERIFY_TERMS = 20;
inline void verifier_term_table(const VerifierScalars& s, const HFr* ch, const HFr* e, const HFr& wn, HFr* out) {
    using zkhost::fr_mul;
    const HFr zeta = ch[3], mu = ch[5];
    out[0] = fr_mul(e[0], e[1]); out[1] = e[0]; out[2] = e[1]; out[3] = e[2]; out[4] = zkhost::fr_one();
    out[5] = s.nup[4]; out[6] = s.nup[5]; out[7] = h_neg(s.k_s3);
    out[8] = s.nup[1]; out[9] = s.nup[2]; out[10] = s.nup[3];
    out[11] = s.k_acc;
    out[12] = h_neg(s.zh); out[13] = h_neg(fr_mul(s.zh, s.zn)); out[14] = h_neg(fr_mul(s.zh, fr_mul(s.zn, s.zn)));
    out[15] = zeta; out[16] = fr_mul(fr_mul(wn, mu), zeta);
    out[17] = h_neg(s.es);
    out[18] = zkhost::fr_one(); out[19] = mu;
}

}  // namespace zkplonk
