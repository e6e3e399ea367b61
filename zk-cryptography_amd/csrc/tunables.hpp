// tunables.hpp -- the library's environment switches: ONE list and ONE parser, the only getenv of csrc/.  Host code, standard library
// only (tests/cpp/host_tunables.cpp compiles it with g++).  A switch that is read ONCE is read into a function-local `static const`
// where it is used -- at first use, once per process, nothing on the launch path afterwards -- and the measurements behind a default
// stay in the comments there; the list says what exists.  DESIGN.md section 8.1 has the same list with who sets what.
#pragma once
#include <climits>
#include <cstdlib>

namespace zk::env {
enum Kind { FLAG, INT, BYTES, TEXT };   // FLAG / INT: the leading decimal integer (atoi: no digits = 0), a flag is on when it is non-zero;
                                        // BYTES: the whole string a decimal number, else the default; TEXT: the string itself (text())
enum Outside { IGNORED, CLAMPED };      // an INT outside [lo, hi]: the default, or the nearer bound
enum When { ONCE, FRESH };              // read at first use for the life of the process, or at every use
constexpr long long UNSET = LLONG_MIN;  // the default of an INT whose absence means "the code decides" (by size, by kind of round)
struct Switch { const char* name; Kind kind; long long def, lo, hi; Outside outside; When when; const char* meaning; };

// X(id, kind, default, lo, hi, outside, when, meaning): the variable is ZKHIP_<id>
#define ZK_ENV_SWITCHES(X)                                                                                                              \
    X(PIPE, FLAG, 1, 0, 1, IGNORED, ONCE, "composed rounds one round ahead of the transcript; 0 = round by round, and the GKR host transcript") \
    X(PIPE_WGS, INT, 256, 1, 512, IGNORED, ONCE, "workgroups that take tiles in a pipelined round, at most")                            \
    X(ROUND_DOT, FLAG, 1, 0, 1, IGNORED, ONCE, "K = 5 rounds with the last factor on the matrix cores; 0 = vector form")               \
    X(ROUND_DOT_MIN_LOG, INT, UNSET, 8, 64, CLAMPED, ONCE, "log2 of the pairs from which ROUND_DOT applies (64 = never); unset = 18 first round, 19 folding") \
    X(ROUND_GRID, INT, 0, 1, INT_MAX, IGNORED, ONCE, "workgroups of a composed round, at most; 0 = 512 for one term, the full grid otherwise") \
    X(STAGE, INT, -1, 0, 1, IGNORED, ONCE, "two rounds per pass: 0 = never, 1 = from 2^15 entries, -1 = from the STAGE_MIN_LOG sizes")  \
    X(STAGE_MIN_LOG_ONE, INT, 18, 12, 30, IGNORED, ONCE, "log2 of the entries from which a one-term claim takes stages")                \
    X(STAGE_MIN_LOG_MANY, INT, 18, 12, 30, IGNORED, ONCE, "the same for claims of several terms")                                       \
    X(CROSS_VALU, FLAG, 0, 0, 1, IGNORED, ONCE, "a stage's cross sums on the VALU instead of the matrix cores")                         \
    X(CROSS_GRID, INT, 0, 1, INT_MAX, IGNORED, ONCE, "workgroups of the matrix-core cross sums, at most; 0 = 512")                      \
    X(MF, INT, 1, 0, 9, IGNORED, ONCE, "streaming k-variable fold: 0 = VALU form, 1..9 = matrix cores with this rotation of the term order") \
    X(MF_OCC, INT, 0, 1, 64, IGNORED, ONCE, "workgroups per CU of the matrix-core fold, at most; 0 = no cap")                           \
    X(FINE_LDS, INT, 79872, 0, 158 * 1024, CLAMPED, ONCE, "LDS bytes the fine block sums request to cap their workgroups per CU; 0 = no cap") \
    X(OVERLAP_MIN_LOG, INT, 24, 19, 25, IGNORED, ONCE, "log2 of the entries from which a sumcheck takes the overlapped plan")           \
    X(MSM_SMALL, FLAG, 1, 0, 1, IGNORED, ONCE, "the short path of small commits and openings; 0 = the bucket path at every size")      \
    X(MSM_BATCH_DELTA, INT, 1, 0, 8, IGNORED, ONCE, "window width of a batched commit's problem: log2(n_j) - delta bits")               \
    X(LEVEL_TABLE_DELTA, INT, UNSET, -3, 4, IGNORED, ONCE, "widest window of a shifted table: log2(n_j) - delta bits; unset = by size") \
    X(OPEN_PIPELINES, FLAG, 0, 0, 1, IGNORED, ONCE, "an opening's rounds above 2^14 as commits of their own instead of one batch")      \
    X(GKR_FUSE_SMALL, FLAG, 1, 0, 1, IGNORED, ONCE, "the fused kernels of small GKR layers; 0 = the gate-row kernels at every size")    \
    X(GKR_HOST_TRANSCRIPT, FLAG, 0, 0, 1, IGNORED, ONCE, "the GKR outer transcript on the host, one synchronisation per layer (also with PIPE=0)") \
    X(PLONK_CACHE_BUDGET, BYTES, 2LL << 30, 0, LLONG_MAX, IGNORED, FRESH, "bytes of coset evaluations a PLONK key may keep; 0 = none; read when a key is made") \
    X(RCCL_LIB, TEXT, 0, 0, 0, IGNORED, ONCE, "the first library name tried for RCCL")
#define X(id, ...) inline constexpr Switch id = {"ZKHIP_" #id, __VA_ARGS__};
ZK_ENV_SWITCHES(X)
#undef X
#define X(id, ...) id,
inline constexpr Switch ALL[] = {ZK_ENV_SWITCHES(X)};
#undef X

// the value of a FLAG (0 / 1), INT or BYTES switch under the current environment; text(): a TEXT switch's, or nullptr
inline long long read(const Switch& s) {
    const char* e = std::getenv(s.name);
    if (!e) return s.def;
    char* end = nullptr;
    if (s.kind == BYTES) { const unsigned long long v = std::strtoull(e, &end, 10); return *e && *end == '\0' ? (long long)v : s.def; }
    const long long v = std::atoll(e);
    if (s.kind == FLAG) return v != 0;
    if (v >= s.lo && v <= s.hi) return v;
    return s.outside == CLAMPED ? (v < s.lo ? s.lo : s.hi) : s.def;
}
inline const char* text(const Switch& s) { return std::getenv(s.name); }
}  // namespace zk::env
