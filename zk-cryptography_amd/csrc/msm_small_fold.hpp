// msm_small_fold.hpp -- the host end of the MSM's short path: the weighted sums of the plane sums that a chunk's one copy fetched.  Host
// arithmetic alone (host_g1.hpp) on the context's threads (host_util.hpp), so that tests/cpp/host_sanitize.cpp runs it without a device.
#pragma once
#include <cstring>
#include <vector>

#include "host_g1.hpp"
#include "host_util.hpp"
#include "msm_small_plan.hpp"

namespace zk {

// pin: the terms of `count` (instance, problem) pairs as the reduce launch left them, k = instance * nprob + problem: plane t of pair k at
// 192 (k planes + t).  Pair k's commit is sum_t 2^t term_t, <= 20 doublings; its affine point goes to h_out_xy + 12 out_of(k) and its
// identity flag to h_out_inf[out_of(k)].  More than one pair: side by side on `pool` (where there is one).
template <class OutOf>
inline void msm_small_fold(const char* pin, const MsmSmallGeometry& g, uint32_t count, ZkHostPool* pool, uint64_t* h_out_xy, uint8_t* h_out_inf,
                           OutOf out_of) {
    auto finish = [&](uint32_t k) {
        const uint32_t hi = g.hi[k % g.nprob];
        std::vector<zkhost::Xyzz> pts(hi);
        std::vector<uint32_t> exps(hi);
        for (uint32_t t = 0; t < hi; ++t) {
            std::memcpy(&pts[t], pin + 192 * ((size_t)k * g.planes + t), 192);
            exps[t] = t;
        }
        const size_t o = out_of(k);
        h_out_inf[o] = zkhost::xyzz_to_affine(zkhost::weighted_sum_pow2(pts, exps), h_out_xy + 12 * o) ? 0 : 1;
    };
    if (count > 1 && pool) {
        pool->run(count, [&](unsigned k) { finish(k); });
    } else {
        for (uint32_t k = 0; k < count; ++k) finish(k);
    }
}

}  // namespace zk
