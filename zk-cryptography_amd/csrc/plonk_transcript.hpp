// plonk_transcript.hpp -- the Fiat-Shamir schedule of the PLONK protocol, host only: MerlinTranscript (transcripts/merlin/src/lib.rs:11-49)
// and PlonkRoundTranscript (plonk/src/protocol/transcript.rs) as prover.rs and protocol/utils.rs:56-96 drive it.
//
// The single prover, every proof of the batched prover and the verifiers' compute_verifier_challenges go through the one
// PlonkRoundTranscript below, so a label or the order of a round is stated once.  No HIP in this file:
// tests/cpp/plonk_transcript_sanitize.cpp builds it with a host compiler.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "host_fr.hpp"
#include "host_g1.hpp"

namespace zkplonk {

using HFr = zkhost::Fr;
static_assert(sizeof(HFr) == 32, "an array of HFr is read as four words per element (fourth_round)");

// proof layout of the ABI: points as, bs, cs, accumulator, t_low, t_mid, t_high, w_zeta, w_zeta_omega; evaluations a, b, c, sigma1,
// sigma2, w_accumulator; challenges beta, gamma, alpha, zeta, nu, mu
enum { P_AS, P_BS, P_CS, P_ACC, P_TL, P_TM, P_TH, P_WZ, P_WZW, N_POINTS };
enum { E_A, E_B, E_C, E_S1, E_S2, E_ZW, N_EVALS };
enum { C_BETA, C_GAMMA, C_ALPHA, C_ZETA, C_NU, C_MU, N_CHALLENGES };

// canonical integer of a Montgomery Fq element in decimal, leading zeros trimmed (ark-ff 0.4.2 Display for Fp: zero prints as "")
inline std::string fq_decimal(const uint64_t* mont) {
    zkhost::Fq a, one = zkhost::fq_zero();
    std::memcpy(a.l, mont, 48);
    one.l[0] = 1;
    zkhost::Fq c = zkhost::fq_mul(a, one);
    std::string out;
    for (;;) {
        bool zero = true;
        for (int i = 0; i < 6; ++i) zero = zero && c.l[i] == 0;
        if (zero) break;
        unsigned __int128 rem = 0;                                 // c /= 10^19
        const uint64_t base = 10000000000000000000ull;
        for (int i = 5; i >= 0; --i) {
            const unsigned __int128 cur = (rem << 64) | c.l[i];
            c.l[i] = (uint64_t)(cur / base);
            rem = cur % base;
        }
        char buf[24];
        snprintf(buf, sizeof buf, "%019llu", (unsigned long long)(uint64_t)rem);
        out.insert(0, buf);
    }
    const size_t nz = out.find_first_not_of('0');
    return nz == std::string::npos ? std::string() : out.substr(nz);
}
// ark-ec 0.4.2 Display for an affine point: "(x, y)", the identity "infinity"
inline std::string point_string(const uint64_t* xy, bool inf) {
    if (inf) return "infinity";
    return "(" + fq_decimal(xy) + ", " + fq_decimal(xy + 6) + ")";
}

struct Merlin {
    zkhost::Sha256 hasher;
    explicit Merlin(const char* label) {                           // :12-21
        hasher.update((const uint8_t*)"Merlin Transcript", 17);
        hasher.update((const uint8_t*)label, std::strlen(label));
    }
    void append_message(const char* label, const uint8_t* m, size_t len) {   // :23-28 label, len as 8 bytes little-endian, message
        hasher.update((const uint8_t*)label, std::strlen(label));
        uint8_t le[8];
        for (int i = 0; i < 8; ++i) le[i] = (uint8_t)((uint64_t)len >> (8 * i));
        hasher.update(le, 8);
        hasher.update(m, len);
    }
    void append_scalar(const char* label, const HFr& mont) {       // :30-35 serialize_compressed: 32 bytes little-endian canonical
        const HFr c = zkhost::fr_from_mont(mont);
        uint8_t b[32];
        for (int i = 0; i < 32; ++i) b[i] = (uint8_t)(c.l[i / 8] >> (8 * (i % 8)));
        append_message(label, b, 32);
    }
    void append_point(const char* label, const uint64_t* xy, bool inf) {     // :37-41 the UTF-8 of to_string()
        const std::string s = point_string(xy, inf);
        append_message(label, (const uint8_t*)s.data(), s.size());
    }
    HFr challenge(const char* label) {                             // :43-49 finalize_reset: the label goes into the EMPTY hasher
        uint8_t d[32];
        hasher.finish(d);
        hasher.reset();
        hasher.update((const uint8_t*)label, std::strlen(label));
        uint64_t t[4];
        for (int i = 0; i < 4; ++i) {
            uint64_t w = 0;
            for (int j = 0; j < 8; ++j) w = (w << 8) | d[8 * (3 - i) + j];
            t[i] = w;
        }
        while (zkhost::fr_geq_p(t)) zkhost::fr_sub_p(t);            // from_be_bytes_mod_order
        HFr c, r2;
        std::memcpy(c.l, t, 32);
        std::memcpy(r2.l, zkhost::FR_R2, 32);
        return zkhost::fr_mul(c, r2);
    }
};

// One proof's transcript and the challenges drawn from it so far, ch[C_*].  Every round takes the PROOF's arrays in the ABI's layout
// -- xy: N_POINTS points of 12 words, inf: N_POINTS flags, evals: N_EVALS elements of 4 words (Montgomery form) -- reads its own
// entries of them, which must be final by then, and draws the challenges that follow the round.
struct PlonkRoundTranscript {
    Merlin t{"plonk_protocol"};
    HFr ch[N_CHALLENGES];
    PlonkRoundTranscript() { std::memset(ch, 0, sizeof ch); }
    void first_round(const uint64_t* xy, const uint8_t* inf) {
        points("first_round", xy, inf, P_AS, P_CS);
        ch[C_BETA] = t.challenge("beta");
        ch[C_GAMMA] = t.challenge("gamma");
    }
    void second_round(const uint64_t* xy, const uint8_t* inf) {
        points("second_round", xy, inf, P_ACC, P_ACC);
        ch[C_ALPHA] = t.challenge("alpha");
    }
    void third_round(const uint64_t* xy, const uint8_t* inf) {
        points("third_round", xy, inf, P_TL, P_TH);
        ch[C_ZETA] = t.challenge("zeta");
    }
    void fourth_round(const uint64_t* evals) {
        for (int e = 0; e < N_EVALS; ++e) {
            HFr v;
            std::memcpy(v.l, evals + 4 * e, 32);
            t.append_scalar("fourth_round", v);
        }
        ch[C_NU] = t.challenge("nu");
    }
    void fifth_round(const uint64_t* xy, const uint8_t* inf) {
        points("fifth_round", xy, inf, P_WZ, P_WZW);
        ch[C_MU] = t.challenge("mu");
    }

private:
    void points(const char* label, const uint64_t* xy, const uint8_t* inf, int first, int last) {
        for (int p = first; p <= last; ++p) t.append_point(label, xy + 12 * p, inf[p] != 0);
    }
};

}  // namespace zkplonk
