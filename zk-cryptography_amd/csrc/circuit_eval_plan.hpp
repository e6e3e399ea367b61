// circuit_eval_plan.hpp -- what zkhip_circuit_evaluate_batch (gkr.hip) decides on the host before it enqueues anything: which layers
// get a launch of their own and which share the tail launch, and whether the reference's index panic (circuit/src/circuit.rs:41-50,
// current_input[e.inputs[k]]) would strike.  Functions of the circuit's shape alone: the entry point and
// tests/test_circuit_eval_plan_cpu.py share this one definition.  No HIP in here.
//
// Evaluation runs from the input up: layer n_layers - 1 first, layer 0 (the output) last.  The WIDE layers are the first ones, as long as
// each holds more than CEB_TAIL_GATES gates: one launch per layer for all inputs of a chunk (gate tiles x inputs).  From the first layer
// of at most CEB_TAIL_GATES gates on, every layer up to the output is walked by ONE launch, one workgroup per input -- also a layer that
// is wider again (no circuit of the reference's Circuit::random has one; the tail's lanes stride over whatever they find).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zk {

// log2 of the widest layer the tail launch starts at.  Measured at 8, 10 and 12 (profiles/circuit_eval_batch/NOTES.md, "The width T");
// -DZK_CEB_TAIL_LOG=8 or 12 builds the other sides of that comparison.
#ifndef ZK_CEB_TAIL_LOG
#define ZK_CEB_TAIL_LOG 10
#endif
constexpr uint32_t CEB_TAIL_GATES = 1u << ZK_CEB_TAIL_LOG;
constexpr uint32_t CEB_TILE = 256;           // gates per workgroup of a wide launch (one per lane)
constexpr uint32_t CEB_TAIL_BLOCK = 512;     // lanes of an input's workgroup in the tail launch
constexpr uint32_t CEB_CHUNK = 4096;         // inputs per launch: the grid's second dimension ends at 65535; beyond a few thousand workgroups a launch gains nothing

// the number of wide layers: layers n_layers - 1 .. n_layers - wide get a launch each, layers n_layers - wide - 1 .. 0 the tail launch
inline uint32_t ceb_wide_layers(const size_t* n_gates, uint32_t n_layers, size_t tail_gates = CEB_TAIL_GATES) {
    uint32_t wide = 0;
    while (wide < n_layers && n_gates[n_layers - 1 - wide] > tail_gates) ++wide;
    return wide;
}
// launches of one chunk
inline uint32_t ceb_launches(const size_t* n_gates, uint32_t n_layers, size_t tail_gates = CEB_TAIL_GATES) {
    const uint32_t wide = ceb_wide_layers(n_gates, n_layers, tail_gates);
    return wide + (wide < n_layers ? 1u : 0u);
}
// entries of the table layer k reads: the layer below it, or the input
inline size_t ceb_below_len(const size_t* n_gates, uint32_t n_layers, size_t input_len, uint32_t k) {
    return k + 1 < n_layers ? n_gates[k + 1] : input_len;
}
// The first layer in evaluation order (the highest index) one of whose gates names an entry the table below it does not have, or
// n_layers when there is none.  max_label[k] = the largest label of layer k (anything when the layer has no gate).
inline uint32_t ceb_first_bad_layer(const size_t* n_gates, const uint32_t* max_label, uint32_t n_layers, size_t input_len) {
    for (uint32_t k = n_layers; k-- > 0;)
        if (n_gates[k] && (size_t)max_label[k] >= ceb_below_len(n_gates, n_layers, input_len, k)) return k;
    return n_layers;
}

}  // namespace zk
