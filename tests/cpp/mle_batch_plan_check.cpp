// mle_batch_plan_check.cpp -- stand-alone program around csrc/mle_batch_plan.hpp for tests/test_mle_batch_plan_cpu.py (g++, no HIP).
// For log_n 0 .. 17 and batch in {0, 1, 2, min - 1, min, 1023, 1024, 1025, 65535}: the chunks partition [0, batch); workgroups and
// records per job, the LDS request, the workspace bytes and the regime are what the header's comment plans, restated here in the
// program's own words.  And the bit order of a block's weight: the blocks' values weighted by meb_weight_bit add up to a brute-force
// eq product over the whole table, point 0 on the most significant index bit, in a small prime field.
// Prints one line per violation and "checked <cases>"; exit status 1 on a violation.
#include <cstdio>
#include <vector>

#include "../../zk-cryptography_amd/csrc/mle_batch_plan.hpp"

using namespace zk;

static int bad = 0, cases = 0;
static void expect(bool ok, const char* what, size_t a, size_t b) {
    ++cases;
    if (!ok && bad++ < 20) std::printf("%s (%zu, %zu)\n", what, a, b);
}

static size_t al(size_t x) { return (x + 255) / 256 * 256; }

// arithmetic mod the prime 2^31 - 1
static const uint64_t P = 2147483647u;
static uint64_t mul(uint64_t a, uint64_t b) { return a * b % P; }
static uint64_t sub(uint64_t a, uint64_t b) { return (a + P - b) % P; }

// sum over idx of table[idx] * prod_i (bit_i(idx) ? r_i : 1 - r_i), bit_0 = the MOST significant of the `vars` index bits
static uint64_t brute(const std::vector<uint64_t>& table, const std::vector<uint64_t>& r, uint32_t first, uint32_t vars, size_t base) {
    uint64_t s = 0;
    for (size_t idx = 0; idx < ((size_t)1 << vars); ++idx) {
        uint64_t w = 1;
        for (uint32_t i = 0; i < vars; ++i) w = mul(w, ((idx >> (vars - 1 - i)) & 1) ? r[first + i] : sub(1, r[first + i]));
        s = (s + mul(w, table[base + idx])) % P;
    }
    return s;
}

int main() {
    for (uint32_t log_n = 0; log_n <= 17; ++log_n) {
        const uint32_t kmin = meb_min_batch(log_n);
        expect((kmin == 0) == (log_n > 16), "no batch is taken above 2^16 entries, and only there", log_n, kmin);
        std::vector<uint32_t> batches = {0, 1, 2, 1023, 1024, 1025, 65535};
        if (kmin) { batches.push_back(kmin - 1); batches.push_back(kmin); }
        for (uint32_t batch : batches) {
            const MebPlan p = meb_plan(log_n, batch);
            const bool single = log_n >= 17 || batch <= 1 || batch < kmin;
            const MebRegime want = single ? MEB_SINGLE : log_n <= 12 ? MEB_RESIDENT : MEB_BLOCKS;
            expect(p.regime == want && (batch == 0 || meb_regime(log_n, batch) == want), "regime", log_n, batch);
            if (single) {
                expect(p.n_chunks == 0 && p.launches == 0 && p.ws_bytes == 0 && p.pin_bytes == 0 && p.lds_bytes == 0, "the single path plans nothing", log_n, batch);
                continue;
            }
            const uint32_t h = log_n <= 12 ? 0 : log_n - 12;
            expect(p.h == h && p.wgs_per_job == (1u << h), "workgroups per job", log_n, p.wgs_per_job);
            expect(p.records_per_job == (h ? 1u << h : 0u) && p.launches == (h ? 2u : 1u), "records per job and launches", log_n, p.records_per_job);
            expect(p.lds_bytes == (size_t)32 << (log_n - h) && p.lds_bytes <= 160 * 1024 && p.lds_bytes <= MEB_MAX_LDS_BYTES, "LDS request", log_n, p.lds_bytes);
            expect(p.lanes == ((log_n - h) >= 12 ? 1024u : 256u) && p.lanes == meb_lanes(log_n - h) && (h == 0 || p.lanes == MEB_WIDE_BLOCK), "lanes of a workgroup", log_n, p.lanes);
            expect(p.chunk == (batch < 1024 ? batch : 1024) && p.chunk <= MEB_CHUNK, "jobs of a chunk", batch, p.chunk);
            uint32_t next = 0;
            bool parts = p.n_chunks == (batch + 1023) / 1024;
            for (uint32_t i = 0; i < p.n_chunks; ++i) {
                const MebChunk c = meb_chunk(p, batch, i);
                parts = parts && c.first == next && c.count >= 1 && c.count <= p.chunk && (i + 1 == p.n_chunks || c.count == p.chunk);
                next = c.first + c.count;
                // what a chunk uploads and writes stays inside the regions planned for it
                parts = parts && (size_t)c.count * 8 <= p.o_points && p.o_points + (size_t)c.count * log_n * 32 <= p.upload_bytes;
                parts = parts && p.o_results + (size_t)c.count * 32 <= p.o_records && p.o_records + (size_t)c.count * p.records_per_job * 32 <= p.ws_bytes;
            }
            expect(parts && next == batch, "the chunks partition the batch and stay in their regions", log_n, batch);
            const size_t bc = p.chunk, up = al(bc * 8) + al(bc * log_n * 32);
            expect(p.o_points == al(bc * 8) && p.upload_bytes == up && p.o_results == up && p.o_records == up + al(bc * 32), "workspace layout", log_n, batch);
            expect(p.ws_bytes == up + al(bc * 32) + al(bc * p.records_per_job * 32), "workspace bytes", log_n, p.ws_bytes);
            expect(p.pin_bytes == al(bc * 32) + up, "pinned bytes", log_n, p.pin_bytes);
            expect(p.o_points % 32 == 0 && p.o_results % 32 == 0 && p.o_records % 32 == 0, "field elements are aligned", log_n, batch);
        }
    }
    // the weight's bit order: h leading points over the blocks, the rest inside a block of 2^t entries
    for (uint32_t h = 1; h <= 4; ++h) {
        const uint32_t t = 3, vars = h + t;
        std::vector<uint64_t> table((size_t)1 << vars), r(vars);
        uint64_t x = 88172645463325252ull + h;
        auto draw = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x % P; };
        for (auto& v : table) v = draw();
        for (auto& v : r) v = draw();
        uint64_t sum = 0;
        for (uint32_t q = 0; q < (1u << h); ++q) {
            uint64_t w = brute(table, r, h, t, (size_t)q << t);            // block q at the points h ..
            for (uint32_t i = 0; i < h; ++i) w = mul(w, meb_weight_bit(q, h, i) ? r[i] : sub(1, r[i]));
            sum = (sum + w) % P;
        }
        expect(sum == brute(table, r, 0, vars, 0), "the blocks' weighted values add up to the table's evaluation", h, sum);
        // and the other bit order does not (the points are distinct with overwhelming probability)
        uint64_t wrong = 0;
        for (uint32_t q = 0; q < (1u << h); ++q) {
            uint64_t w = brute(table, r, h, t, (size_t)q << t);
            for (uint32_t i = 0; i < h; ++i) w = mul(w, ((q >> i) & 1) ? r[i] : sub(1, r[i]));
            wrong = (wrong + w) % P;
        }
        if (h > 1) expect(wrong != sum, "the reversed bit order is another value", h, wrong);
    }
    std::printf("checked %d\n", cases);
    return bad ? 1 : 0;
}
