// ctx.hpp -- per-device context of libzkhip: stream, workspaces, event-based kernel timing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <vector>

#include "../../include/zkhip.h"
#include "hip_own.hpp"
#include "host_util.hpp"

#define ZK_MAX_ROUNDS 48          /* rounds of one sumcheck: tables of 2^48 entries are far beyond 288 GB; a GKR layer of width 2^24 takes 2 x 24 */
#define ZK_MAX_PARTIALS 4096      /* (lo, hi) pairs: >= the largest grid any reducing kernel uses */

// fixed carve-up of the small device scratch (offsets in uint64_t units)
enum : size_t {
    ZK_SMALL_R = 0,                                           // 4:  one field element (fold point / scalar)
    ZK_SMALL_RES = 16,                                        // 16: small results
    ZK_SMALL_STATE = 64,                                      // 64: SumcheckDev / transcript state
    ZK_SMALL_PTS = 256,                                       // 4*ZK_MAX_ROUNDS evaluation points
    ZK_SMALL_CHALLENGES = ZK_SMALL_PTS + 4 * ZK_MAX_ROUNDS,   // 4*ZK_MAX_ROUNDS
    ZK_SMALL_ROUNDPOLYS = ZK_SMALL_CHALLENGES + 4 * ZK_MAX_ROUNDS,   // up to 8 coefficients x 2 words... 64*ZK_MAX_ROUNDS
    ZK_SMALL_PARTIALS = ZK_SMALL_ROUNDPOLYS + 64 * ZK_MAX_ROUNDS,    // 8 * ZK_MAX_PARTIALS * 8 (composed: up to 8 sums/block)
    ZK_SMALL_END = ZK_SMALL_PARTIALS + 4 * 8 * ZK_MAX_PARTIALS
};
#define ZK_SMALL_BYTES (ZK_SMALL_END * 8)

// pinned host staging (uint64_t units)
enum : size_t {
    ZK_PIN_R = 0,
    ZK_PIN_RES = 16,
    ZK_PIN_PTS = 64,
    ZK_PIN_PROOF = ZK_PIN_PTS + 4 * ZK_MAX_ROUNDS,
    ZK_PIN_END = ZK_PIN_PROOF + 4 + 8 * ZK_MAX_ROUNDS + 4 * ZK_MAX_ROUNDS + 64 * ZK_MAX_ROUNDS
};
#define ZK_PINNED_BYTES (ZK_PIN_END * 8)

#define ZK_HIP(ctx, call)                                   \
    do {                                                    \
        hipError_t _e = (call);                             \
        if (_e != hipSuccess) {                             \
            (ctx)->last_hip = (int)_e;                      \
            return ZKHIP_ERR_HIP;                           \
        }                                                   \
    } while (0)
#define ZK_TRY(expr)                 \
    do {                             \
        int _s = (expr);             \
        if (_s != ZKHIP_OK) return _s; \
    } while (0)

struct ZkProfEvent { zk::Event start, stop; };
struct ZkProfRecord { const char* name; size_t event; double bytes; };

// library structs a context owns without knowing their layout: each deleter is defined in the unit that defines the struct
struct NttCache;                                                        // ntt.hip
struct NttCacheDelete { void operator()(NttCache*) const; };
struct MsmPending;                                                      // msm.hip
struct MsmPendingDelete { void operator()(MsmPending*) const; };
namespace zk { struct MsmGeometry; }                                    // msm_geometry.hpp
struct ZkCtxDestroy { void operator()(zkhip_ctx* c) const { (void)zkhip_ctx_destroy(c); } };   // a context is drained, not just deleted
using ZkCtxOwner = std::unique_ptr<zkhip_ctx, ZkCtxDestroy>;

// Every member that stands for a HIP resource is an owner (hip_own.hpp); a plain handle is a view of one owned elsewhere.  Members go
// away in reverse declaration order, after zkhip_ctx_destroy has made the device current, destroyed the GKR lanes and drained every
// stream the context created -- so among buffers, events and streams the order does not matter.  It does for host_pool: see there.
struct zkhip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;    // the caller's stream (NULL = the device's default stream), or a view of owned_stream
    zk::Stream owned_stream;         // a GKR lane's stream: the only contexts that create their own
    int last_hip = 0;
    zk::GrowBuf ws;                  // large workspace (ping-pong tables, MSM buckets, ...); see reserve_ws / ws_loans
    zk::DevMem d_fingerprint;        // zkhip_srs_fingerprint's 52 words, its stream (highest priority) and the event that orders it behind the caller's
    zk::Stream guard_stream;
    zk::Event guard_ev;
    zk::DevMem d_composed;           // composed provers: ComposedDev (transcript + interpolation matrices of every degree), uploaded once (untyped: ComposedDev needs composed_kernels.hpp)
    zk::DevMem d_gen_table;          // SRS generation: d * 2^(8w) * G for 32 windows x 255 digits, affine (+ infinity flags); built on first use
    std::unique_ptr<NttCache, NttCacheDelete> ntt_state;   // twiddle tables and pass plans of the transforms this context has run (ntt.hip)
    zk::GrowBuf aux;                 // second grow-only buffer for entry points that call others which own the workspace (kzg_open)
    zk::GrowBuf dense_scratch;       // zkhip_dense_points: weights, records and domain values (dense_points_plan.hpp); grows only, never the workspace
    uint32_t outer_token = 0;   // sessions that feed an outer transcript (composed_kernels.hpp): a value no earlier session's flags hold
    // pinned result buffers + events for commits whose host epilogue is deferred (msm_enqueue / msm_finish), and the side
    // streams on which MultilinearKZG::open runs its per-round commits next to each other
    static constexpr int MSM_SLOTS = 6;
    zk::GrowBuf msm_pin[MSM_SLOTS];
    zk::Event msm_ev[MSM_SLOTS];
    zk::Stream side[MSM_SLOTS];
    zk::Event fork_ev, join_ev, serial_ev;
    int ensure_side_streams() {
        for (int i = 0; i < MSM_SLOTS; ++i)
            if (zk::ensure_stream(side[i]) != hipSuccess) return ZKHIP_ERR_HIP;
        if (zk::ensure_event(fork_ev) != hipSuccess || zk::ensure_event(join_ev) != hipSuccess || zk::ensure_event(serial_ev) != hipSuccess) return ZKHIP_ERR_HIP;
        return ZKHIP_OK;
    }
    // The basic prover's streaming fold runs on a LOW-priority stream of its own next to the serial transcript kernel
    // (the dispatcher prefers the serial kernel's single workgroup whenever both are ready).  Measured alternatives
    // (DESIGN.md section 5): a CU-masked fold stream that leaves one CU to the serial kernel -- such streams can only be
    // created "blocking", and the implicit synchronisation with the NULL stream (PyTorch's default) cost 30-60 us per
    // fork / join; sharing a CU with fold waves -- the transcript wave runs at half speed.
    zk::Stream fold_stream;
    int ensure_fold_stream() {
        if (zk::ensure_stream(fold_stream, zk::Prio::Low) != hipSuccess) return ZKHIP_ERR_HIP;
        return ensure_side_streams();
    }
    // coarse block sums left by zkhip_mle_block_sums for the prover's first rounds: a ring (canonical, then Montgomery: 64 KiB
    // each; more entries than proofs in flight), so that the sums of a table whose proof is in flight survive the poly_sum() of the next tables
    static constexpr int COARSE_RING = 16;
    zk::DevMem d_coarse[COARSE_RING];
    const void* coarse_of[COARSE_RING] = {}; size_t coarse_n[COARSE_RING] = {}; uint32_t coarse_k1[COARSE_RING] = {};
    int coarse_owner[COARSE_RING] = {};     // result slot + 1 of the proof that still reads the entry (0: nobody): such an entry is never handed out
    int coarse_next = 0;
    int next_coarse(int* slot) {
        for (int tries = 0; tries < COARSE_RING; ++tries) {
            const int k = coarse_next;
            coarse_next = (coarse_next + 1) % COARSE_RING;
            if (coarse_owner[k]) continue;          // a proof in flight reads it from a stream of its own: no event orders a rewrite behind that
            if (!d_coarse[k] && zk::dev_alloc(d_coarse[k], 2 * 1024 * 32) != hipSuccess) return ZKHIP_ERR_NOMEM;
            coarse_of[k] = nullptr;
            *slot = k;
            return ZKHIP_OK;
        }
        return ZKHIP_ERR_BUSY;                       // unreachable with <= PROOF_SLOTS proofs in flight (one entry each), kept as a guard
    }
    void release_coarse(int proof_slot) {
        for (int k = 0; k < COARSE_RING; ++k) if (coarse_owner[k] == proof_slot + 1) coarse_owner[k] = 0;
    }
    // Sumcheck::prove in flight (zkhip_sumcheck_prove_begin): every ticket has a LANE of its own -- events, workspace and small scratch, a
    // high-priority serial stream and a low-priority fold stream -- so that the streaming passes of one proof run while the transcript rounds
    // of the others hash (the synchronous call keeps the caller's stream and the context's buffers).  Lanes k and k + 4 -- four proofs apart,
    // the older one is done when the younger one begins -- share their two streams: the runtime serves all streams of one priority from four
    // hardware queues, and two streams that take turns in one queue wait for each other's kernels (profiles/r06/NOTES.md section 7: with six
    // serial streams on four queues the first rounds of a proof stood behind another lane's 100 us serial kernel)
    struct ProofLane {
        hipStream_t serial = nullptr, fold = nullptr;   // views: of own_serial / own_fold, or of the streams of lane k - 4
        zk::Stream own_serial, own_fold;
        zk::Event begin_ev, fork_ev, serial_ev;
        zk::GrowBuf ws;
        zk::DevMem small;
    };
    static constexpr int PROOF_SLOTS = 8;      // proofs in flight (measured at 2^24 with 2 .. 12, see bench.py `pipelined`; nothing is gained beyond 8)
    static constexpr int LANE_STREAMS = 4;     // = the hardware queues of one stream priority
    ProofLane lanes[PROOF_SLOTS];
    // With three or more proofs in flight the big fold of a proof is NOT enqueued when the proof begins: it goes onto the CALLER's stream --
    // where poly_sum() puts every table's sums pass -- behind the sums passes of the next one to three tables, so that ONE stream carries
    // all streaming passes back to back (two passes side by side take 2.5 x as long as one, not 2 x) and never waits for a proof's first
    // rounds.  `deferred` holds those second halves, oldest first; they are enqueued by the next zkhip_sumcheck_prove_begin, by
    // zkhip_sumcheck_prove_end of that proof (or of a younger one), and by everything that drains or replaces the caller's stream.
    std::deque<std::pair<int, std::function<int()>>> deferred;      // (proof slot, what is left to enqueue)
    int deferred_rc[PROOF_SLOTS] = {};                              // a second half that could not be enqueued: reported by prove_end of that proof
    // enqueue the oldest entries until `keep` are left, or -- until_slot >= 0 -- until that proof's entry has gone (nothing if it has already)
    int flush_deferred(size_t keep = 0, int until_slot = -1) {
        if (until_slot >= 0) {
            bool there = false;
            for (auto& d : deferred) there = there || d.first == until_slot;
            if (!there) return ZKHIP_OK;
        }
        int rc = ZKHIP_OK;
        while (deferred.size() > keep) {
            const int slot = deferred.front().first;
            std::function<int()> f = std::move(deferred.front().second);
            deferred.pop_front();
            const int r = f();
            if (r != ZKHIP_OK) { deferred_rc[slot] = r; if (rc == ZKHIP_OK) rc = r; }
            if (slot == until_slot) break;
        }
        return rc;
    }
    int ensure_lane_streams(int k) {
        ProofLane& L = lanes[k];
        if (L.serial) return ZKHIP_OK;
        if (k >= LANE_STREAMS) {
            const int rc = ensure_lane_streams(k - LANE_STREAMS);
            if (rc != ZKHIP_OK) return rc;
            L.serial = lanes[k - LANE_STREAMS].serial;
            return ZKHIP_OK;
        }
        if (zk::ensure_stream(L.own_serial, zk::Prio::High) != hipSuccess) return ZKHIP_ERR_HIP;
        L.serial = L.own_serial.get();
        // (measured and dropped, profiles/r06/NOTES.md: some lanes' serial stream at normal instead of high priority, or their fold stream at
        // normal instead of low: 0.27-0.32 ms per proof in flight instead of 0.23; the serial kernels must get in front of every streaming pass)
        return ZKHIP_OK;
    }
    // A lane's low-priority fold stream (only a proof that begins with at most one other in flight keeps its big fold on a stream of its
    // own: tickets 0 and 1) -- created WITH the lane all the same, for lanes 0..3: the runtime serves the streams of one priority from at
    // most four hardware queues, gives a new stream the queue with the fewest streams on it, the FIRST such queue on a tie -- and a queue it
    // has just created for one stream ties with every other single-stream queue.  With the four fold streams the low-priority pool is full
    // when the lanes exist (as the high-priority one is with the four serial streams), and lanes created later by somebody else -- the GKR
    // batch's -- spread over the queues: with fold streams on demand two of its eight lanes landed on ONE queue in bench.py's process
    // (46 % busy each, the others 80-90 %: 0.47 instead of 0.34 ms per depth-8 proof; profiles/r06/NOTES.md).  The price: the synchronous
    // proof's fork onto its own fold stream costs 4 us more once the lanes exist (five low-priority streams on four queues, tools/ab_lanes.py).
    int ensure_lane_fold(int k) {
        ProofLane& L = lanes[k];
        if (L.fold) return ZKHIP_OK;
        if (k >= LANE_STREAMS) {
            const int rc = ensure_lane_fold(k - LANE_STREAMS);
            if (rc != ZKHIP_OK) return rc;
            L.fold = lanes[k - LANE_STREAMS].fold;
            return ZKHIP_OK;
        }
        if (zk::ensure_stream(L.own_fold, zk::Prio::Low) != hipSuccess) return ZKHIP_ERR_HIP;
        L.fold = L.own_fold.get();
        return ZKHIP_OK;
    }
    int ensure_lane(int k, size_t ws_need) {
        ProofLane& L = lanes[k];
        { const int rc = ensure_lane_streams(k); if (rc != ZKHIP_OK) return rc; }
        { const int rc = ensure_lane_fold(k); if (rc != ZKHIP_OK) return rc; }
        if (zk::ensure_event(L.begin_ev) != hipSuccess || zk::ensure_event(L.fork_ev) != hipSuccess || zk::ensure_event(L.serial_ev) != hipSuccess) return ZKHIP_ERR_HIP;
        if (!L.small && zk::dev_alloc(L.small, ZK_SMALL_BYTES) != hipSuccess) return ZKHIP_ERR_NOMEM;
        // grow-only; the lane is idle here (its ticket is free), but what it enqueued last may still read a block it already has
        if (L.ws.ptr) return L.ws.reserve(ws_need, {L.serial, L.fold});
        return L.ws.reserve(ws_need);
    }
    int reserve_msm_pin(int slot, size_t bytes) {
        if (zk::ensure_event(msm_ev[slot]) != hipSuccess) return ZKHIP_ERR_HIP;
        return msm_pin[slot].reserve_pinned(bytes);
    }
    // geometry tables of the commit in slot `slot` (msm_build_geometry): device copy + pinned staging, kept while the geometry is the same
    zk::GrowBuf msm_tab_dev[MSM_SLOTS], msm_tab_pin[MSM_SLOTS];
    std::shared_ptr<const zk::MsmGeometry> msm_tab_geo[MSM_SLOTS];   // the geometry whose tables the device copy holds (kept alive: its address is its identity)
    int reserve_msm_tab(int slot, size_t bytes) {
        const size_t cap = (bytes + 65535) & ~(size_t)65535;
        if (cap > msm_tab_dev[slot].bytes || cap > msm_tab_pin[slot].bytes) msm_tab_geo[slot].reset();      // new blocks: nothing uploaded yet
        ZK_TRY(msm_tab_dev[slot].reserve(cap));
        return msm_tab_pin[slot].reserve_pinned(cap);
    }
    std::vector<ZkCtxOwner> gkr_lanes;   // child contexts of zkhip_gkr_prove_batch (a stream, scratch and transcript state each), destroyed with this one
    // a lane replays a circuit's launch chain as a HIP graph (gkr.hip): its own copy of the layer values + the graph and the addresses it holds
    bool gkr_lane = false;
    zkhip_ctx* gkr_parent = nullptr;            // a lane's owner: the lanes' proofs that allocate or record a graph take turns under its gkr_warm_mu
    std::mutex gkr_warm_mu;
    zk::GrowBuf gkr_in;
    struct GkrGraph {
        zk::GraphExec exec;
        const void *cir = nullptr, *aux = nullptr, *in = nullptr, *ws = nullptr, *pin = nullptr, *composed = nullptr;
        const void *warm_cir = nullptr, *warm_aux = nullptr, *warm_ws = nullptr;      // a plain proof of this circuit has run here (allocations made)
    } gkr_graph;
    // The workspace backs a split-phase prover state or commits in flight: every such borrower holds a ZkLoan of ws_loans for as long
    // as it lives, and reserve_ws refuses while one is out.
    ZkLoanDesk ws_loans;
    // commits in flight (zkhip_kzg_commit_begin / _end): two slots, each with a region of the workspace, a side stream and a
    // pinned result buffer of its own; `async_pend` is an MsmPending allocated by msm.hip
    static constexpr int ASYNC_SLOTS = 3;   // commits in flight (zkhip_kzg_commit_begin); measured with the pipeline filling and draining inside the timed region: 2 / 3 / 4 slots = 3.03 / 2.91 / 2.98 ms per 2^20-point commit
    std::unique_ptr<MsmPending, MsmPendingDelete> async_pend[ASYNC_SLOTS];
    size_t async_region = 0;
    // one cached set of small split-phase buffers, so that a steady stream of sharded proves never allocates
    zk::DevMem sc_small, sc_stage; size_t sc_stage_cap = 0;
    ZkLoanDesk sc_loans;        // held by the state that uses the cached pair
    zk::DevMem d_small;         // fixed small scratch, layout above
    zk::PinMem h_pinned;
    bool profiling = false;
    std::vector<ZkProfEvent> prof_events;
    size_t prof_used = 0;
    std::vector<ZkProfRecord> prof_records;

    int activate() {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { last_hip = (int)e; return ZKHIP_ERR_HIP; }
        return ZKHIP_OK;
    }
    // compute units of the device, read once: what a launch that keeps its workgroups resident sizes its grid by
    uint32_t cu_count = 0;
    int compute_units(uint32_t* cus) {
        if (!cu_count) {
            int v = 0;
            hipError_t e = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device);
            if (e != hipSuccess || v <= 0) { last_hip = (int)e; return ZKHIP_ERR_HIP; }
            cu_count = (uint32_t)v;
        }
        *cus = cu_count;
        return ZKHIP_OK;
    }
    std::set<const void*> big_lds_done;
    // kernels that carve more than 64 KiB of the CU's 160 KiB LDS need the attribute raised once per function
    int allow_big_lds(const void* fn, size_t bytes) {
        if (bytes <= 64 * 1024 || big_lds_done.count(fn)) return ZKHIP_OK;
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) { last_hip = (int)e; return ZKHIP_ERR_HIP; }
        big_lds_done.insert(fn);
        return ZKHIP_OK;
    }
    // Host wait for a stream's work so far: polls an event for up to ~2 ms (a prover call is a few hundred
    // microseconds; a blocking wait's wake-up costs 10-20 us of idle GPU before the next call), then blocks.
    zk::Event done_ev;
    int wait_stream(hipStream_t s = nullptr) {
        if (!s) s = stream;
        if (zk::ensure_event(done_ev) != hipSuccess) return ZKHIP_ERR_HIP;
        if (hipEventRecord(done_ev.get(), s) != hipSuccess) return ZKHIP_ERR_HIP;
        if (s != stream && hipStreamWaitEvent(stream, done_ev.get(), 0) != hipSuccess) return ZKHIP_ERR_HIP;   // the caller's stream stays ordered behind it
        for (int spin = 0; spin < 200000; ++spin) {
            const hipError_t e = hipEventQuery(done_ev.get());
            if (e == hipSuccess) return ZKHIP_OK;
            if (e != hipErrorNotReady) { last_hip = (int)e; return ZKHIP_ERR_HIP; }
        }
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) { last_hip = (int)e; return ZKHIP_ERR_HIP; }
        return ZKHIP_OK;
    }
    int wait_event(hipEvent_t ev) {      // the same for an event already recorded
        for (int spin = 0; spin < 200000; ++spin) {
            const hipError_t e = hipEventQuery(ev);
            if (e == hipSuccess) return ZKHIP_OK;
            if (e != hipErrorNotReady) { last_hip = (int)e; return ZKHIP_ERR_HIP; }
        }
        const hipError_t e = hipEventSynchronize(ev);
        if (e != hipSuccess) { last_hip = (int)e; return ZKHIP_ERR_HIP; }
        return ZKHIP_OK;
    }
    // result slots of the basic prover: pinned copies of [state .. round polynomials] + the event their copy completes at;
    // proof_pending[k] = n_vars of the proof in flight in slot k (0: free)
    // Behind the mirrored span every slot has a SEQUENCE WORD: the proof's last kernel stores proof_seq[k] there (a system-scope release)
    // once the mirror is complete, and the synchronous call's collector spins on it (wait_proof) instead of on the event, which is
    // signalled only after the kernel's epilogue and end-of-kernel write-back (proofs in flight are collected by their event:
    // sumcheck_collect).  proof_seq[k] counts the proofs enqueued into slot k and is never reset, so no
    // earlier proof's word -- collected, abandoned or still to come on the slot's stream -- can pass for this one's.
    static constexpr size_t PROOF_PIN_WORDS = (ZK_SMALL_ROUNDPOLYS - ZK_SMALL_STATE) + 8 * ZK_MAX_ROUNDS;
    zk::PinMem proof_pin[PROOF_SLOTS];
    zk::Event proof_ev[PROOF_SLOTS];
    uint32_t proof_pending[PROOF_SLOTS] = {};
    uint64_t proof_seq[PROOF_SLOTS] = {};
    uint64_t* proof_word(int k) { return (uint64_t*)proof_pin[k].get() + PROOF_PIN_WORDS; }
    int ensure_proof_slot(int k) {
        if (zk::ensure_event(proof_ev[k]) != hipSuccess) return ZKHIP_ERR_HIP;
        if (!proof_pin[k]) {
            if (zk::pin_alloc(proof_pin[k], (PROOF_PIN_WORDS + 8) * 8) != hipSuccess) return ZKHIP_ERR_NOMEM;
            *proof_word(k) = 0;                 // below every value of the counter
        }
        return ZKHIP_OK;
    }
    // Host wait for the proof in slot k: the sequence word for as long as wait_event would poll, then the event -- a faulted kernel or
    // a lost device never writes the word and is reported by the event exactly as before.  With the library's profile on, the event
    // alone: the timeline's events are then complete when the call returns.
    int wait_proof(int k) {
        if (!profiling) {
            const volatile uint64_t* word = proof_word(k);
            const uint64_t want = proof_seq[k];
            const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);      // wait_event's ~2 ms of polling
            do {
                for (int spin = 0; spin < 256; ++spin)
                    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return ZKHIP_OK;
            } while (std::chrono::steady_clock::now() < give_up);
        }
        return wait_event(proof_ev[k].get());
    }
    // proofs still in flight write their results into the pinned slots from their lanes' streams, and no buffer may go away under a
    // kernel: zkhip_ctx_destroy waits for the caller's stream and for every stream the context created
    void drain_streams() {
        hipStreamSynchronize(stream);
        if (fold_stream) hipStreamSynchronize(fold_stream.get());
        for (auto& L : lanes) { if (L.serial) hipStreamSynchronize(L.serial); if (L.fold) hipStreamSynchronize(L.fold); }
        for (auto& s : side) if (s) hipStreamSynchronize(s.get());
        if (guard_stream) hipStreamSynchronize(guard_stream.get());
    }
    uint64_t* small_u64(size_t off) { return (uint64_t*)d_small.get() + off; }
    uint64_t* pinned_u64(size_t off) { return (uint64_t*)h_pinned.get() + off; }
    // grow-only workspaces; growth synchronises (never inside a steady-state timed loop)
    int reserve_aux(size_t bytes) { return aux.reserve(bytes, {stream}, &last_hip); }
    int reserve_ws(size_t bytes) {
        if (ws_loans.lent()) return ZKHIP_ERR_BUSY;     // a live split-phase session or a commit in flight uses it: neither overwrite nor free it
        return ws.reserve(bytes, {stream}, &last_hip);
    }
    // host epilogues of batched commits (created on first use, min(hardware threads, 32) - 1 workers).  Declared last: its threads are
    // joined before anything a job of theirs could reference goes away.
    std::unique_ptr<ZkHostPool> host_pool;
    ZkHostPool* pool() {
        if (!host_pool) {
            const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
            host_pool.reset(new (std::nothrow) ZkHostPool(std::min(hw, 32u) - 1));
        }
        return host_pool.get();
    }
};

// Brackets one kernel launch with HIP events on the context's stream when profiling is on.
struct ProfScope {
    zkhip_ctx* c;
    size_t idx = 0;
    bool on;
    hipStream_t s;
    ProfScope(zkhip_ctx* ctx, const char* name, double bytes, hipStream_t on_stream = nullptr)
        : c(ctx), on(ctx->profiling), s(on_stream ? on_stream : ctx->stream) {
        if (!on) return;
        if (c->prof_used == c->prof_events.size()) {
            ZkProfEvent ev;
            (void)zk::ensure_event(ev.start, hipEventDefault);
            (void)zk::ensure_event(ev.stop, hipEventDefault);
            c->prof_events.push_back(std::move(ev));
        }
        idx = c->prof_used++;
        hipEventRecord(c->prof_events[idx].start.get(), s);
        c->prof_records.push_back({name, idx, bytes});
    }
    ~ProfScope() {
        if (on) hipEventRecord(c->prof_events[idx].stop.get(), s);
    }
};

// cross-unit internals (C++ linkage, not part of the C ABI)
int zk_ntt_scaled_transform(zkhip_ctx* c, const uint64_t* d_src, size_t n_src, const uint64_t* d_mul, uint64_t* d_dst, uint32_t log_n);   // ntt.hip
// zkhip.hip: a batch of basic (k = 1, absorb_sum) or composed sumcheck proofs through sumcheck_batch_kernels.hpp (see there)
int zk_sumcheck_batch_run(zkhip_ctx* c, uint32_t batch, const uint64_t* const* h_table_ptrs, uint32_t k, size_t n, bool absorb_sum,
                          const uint64_t* h_claimed_sums, uint64_t* h_sums, uint64_t* h_round_polys, uint64_t* h_challenges);
bool zk_sumcheck_batch_serves(uint32_t batch, bool basic, uint32_t k, size_t n);   // false: the batched entry points run the single provers
// msm.hip: one round's commits of a chunk of PLONK proofs on the short path (see there)
bool zk_msm_commit_batch_serves(size_t n_points, size_t longest);
int zk_msm_commit_batch(zkhip_ctx* c, const void* d_table_with_header, const uint8_t* d_points_inf, size_t n_points, const uint64_t* d_scalars,
                        size_t q_stride, uint32_t batch, uint32_t m, const size_t* sc_off, const size_t* lens, uint64_t* h_out_xy,
                        uint8_t* h_out_inf, size_t out_stride);
