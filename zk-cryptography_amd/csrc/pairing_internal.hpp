// pairing_internal.hpp -- what another unit of libzkhip may call of pairing.hip (C++ linkage, not part of the C ABI).  Each forwards to
// the function of the same name there; see pairing.hip for the contracts.
#pragma once
#include <cstddef>
#include <cstdint>

struct zkhip_ctx;

// Miller loops of n_groups x m pairs against prepared lines (entry k % q_mod), the product tree, one final exponentiation per group.
// f: n_groups * m * 72 words of scratch; out_ok[g] = 1 iff the group's product is one.
int zk_pairing_groups(zkhip_ctx* c, const uint64_t* d_p_xy, const uint8_t* d_p_inf, const uint64_t* d_prep, size_t q_mod, size_t n_groups, size_t m,
                      uint64_t* d_f, uint8_t* d_out_ok);
// prepared lines of [G2, q_0 .. q_{n-1}] into d_prep (n + 1 entries); d_bad: n + 1 bytes of scratch.  Synchronises; ZKHIP_ERR_ARG on an
// invalid point.
int zk_pairing_prepare_kzg(zkhip_ctx* c, const uint64_t* d_xy, const uint8_t* d_inf, size_t n, uint64_t* d_prep, uint8_t* d_bad);
// copies n flag bytes back, waits for the stream and tells whether any is set
int zk_pairing_any_flag(zkhip_ctx* c, const uint8_t* d_flags, size_t n, bool* any);
