// test_mirror_eval_batch.cpp -- DeviceCircuit::evaluation_batch of the C++ host mirror (include/zkhip.hpp): three inputs on
// CIRCUIT_3 (circuit/src/circuit.rs:209-260), batched and singly, both against the CPU oracle; the batch goes into prove_batch as it
// is; the out-of-range throw.  Built and run by tests/test_cpp_mirror_eval_batch.py.  Exit code 0 = all passed.
#include <cstdio>
#include <random>

#include "../../include/zkhip.hpp"
extern "C" {
#include "../../oracle/zkoracle.h"
}

using namespace zkc;
static int g_failed = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("  FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
    } while (0)

static Gate G(GateType t, size_t a, size_t b) { return Gate{t, {a, b}}; }

int main() {
    const GateType A = GateType::Add, M = GateType::Mul;
    Circuit circuit({CircuitLayer{{G(A, 0, 1)}}, CircuitLayer{{G(A, 0, 1), G(M, 2, 3)}}, CircuitLayer{{G(A, 0, 1), G(M, 2, 3), G(M, 4, 5), G(M, 6, 7)}}});
    const size_t n_gates[3] = {1, 2, 4};
    std::vector<uint8_t> gt; std::vector<uint32_t> i0, i1;
    for (auto& l : circuit.layers) Circuit::arrays(l, gt, i0, i1);
    std::vector<std::vector<Fr>> inputs(3);
    for (int64_t v : {2, 3, 1, 4, 1, 2, 3, 4}) inputs[0].push_back(Fr::from(v));          // the reference's input: output 33
    std::mt19937_64 g(2024);
    for (size_t b = 1; b < 3; ++b)
        for (size_t i = 0; i < 8; ++i) { Fr e; for (int j = 0; j < 4; ++j) e.l[j] = g(); e.l[3] &= 0x3FFFFFFFFFFFFFFFULL; inputs[b].push_back(e); }
    DeviceCircuit dev(circuit);
    auto batch = dev.evaluation_batch(inputs);
    EXPECT(batch.size() == 3);
    for (size_t b = 0; b < batch.size(); ++b) {
        std::vector<Fr> want(15);
        size_t lens[4] = {0, 0, 0, 0};
        EXPECT(ora_circuit_evaluation(3, n_gates, gt.data(), i0.data(), i1.data(), reinterpret_cast<const fr_t*>(inputs[b].data()), 8,
                                      reinterpret_cast<fr_t*>(want.data()), lens) == 0);
        auto single = circuit.evaluation(inputs[b]);
        EXPECT(batch[b].lens == single.lens && batch[b].lens == std::vector<size_t>(lens, lens + 4));
        size_t off = 0;
        for (size_t k = 0; k < 4 && k < batch[b].lens.size(); ++k) {
            const std::vector<Fr> w(want.begin() + off, want.begin() + off + lens[k]);
            EXPECT(batch[b].layer(k) == w);
            EXPECT(single.layer(k) == w);
            off += lens[k];
        }
    }
    EXPECT(batch[0].layer(0) == std::vector<Fr>{Fr::from(33)});
    // the batch's evaluations are what prove_batch takes
    auto proofs = dev.prove_batch(batch);
    EXPECT(proofs.size() == 3);
    for (size_t b = 0; b < proofs.size(); ++b) {
        auto one = dev.prove(circuit.evaluation(inputs[b]));
        EXPECT(proofs[b].wb_s == one.wb_s && proofs[b].wc_s == one.wc_s && proofs[b].w_0_mle == one.w_0_mle);
        EXPECT(proofs[b].sumcheck_proofs.size() == one.sumcheck_proofs.size());
        for (size_t k = 0; k < proofs[b].sumcheck_proofs.size() && k < one.sumcheck_proofs.size(); ++k)
            EXPECT(proofs[b].sumcheck_proofs[k].to_bytes() == one.sumcheck_proofs[k].to_bytes());
    }
    EXPECT(dev.evaluation_batch({}).empty());
    // current_input[e.inputs[k]] panics: an input one entry short, singly and batched
    std::vector<std::vector<Fr>> shorter(2, std::vector<Fr>(inputs[1].begin(), inputs[1].begin() + 7));
    bool threw_single = false, threw_batch = false, threw_ragged = false;
    try { circuit.evaluation(shorter[0]); } catch (const std::out_of_range&) { threw_single = true; }
    try { dev.evaluation_batch(shorter); } catch (const std::out_of_range&) { threw_batch = true; }
    try { dev.evaluation_batch({inputs[0], shorter[0]}); } catch (const Panic&) { threw_ragged = true; }
    EXPECT(threw_single && threw_batch && threw_ragged);
    std::printf("eval batch mirror: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
