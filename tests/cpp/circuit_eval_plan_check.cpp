// circuit_eval_plan_check.cpp -- stand-alone program around csrc/circuit_eval_plan.hpp for tests/test_circuit_eval_plan_cpu.py (g++, no
// HIP).  The launch plan and the label bounds of zkhip_circuit_evaluate_batch on the shapes the entry point meets: Circuit::random at
// every depth, layers at T - 1, T and T + 1 gates, a layer wider than T above a narrow one, empty layers, a circuit that is all wide;
// and, for every layer of a small circuit in turn, a label equal to the length below it (and one short of it).
// Prints one line per violation and "checked <cases>"; exit status 1 on a violation.
#include <cstdio>
#include <vector>

#include "../../zk-cryptography_amd/csrc/circuit_eval_plan.hpp"

using namespace zk;

static int bad = 0, cases = 0;
static void expect(bool ok, const char* what, size_t a, size_t b) {
    ++cases;
    if (!ok && bad++ < 20) std::printf("%s (%zu, %zu)\n", what, a, b);
}

int main() {
    const size_t T = CEB_TAIL_GATES;
    // Circuit::random(d): layer l has 2^l gates; the layers wider than T are the last ones
    for (uint32_t d = 1; d <= 24; ++d) {
        std::vector<size_t> ng(d);
        for (uint32_t l = 0; l < d; ++l) ng[l] = (size_t)1 << l;
        const uint32_t want = d > ZK_CEB_TAIL_LOG + 1 ? d - ZK_CEB_TAIL_LOG - 1 : 0;
        expect(ceb_wide_layers(ng.data(), d) == want, "wide layers of Circuit::random", d, ceb_wide_layers(ng.data(), d));
        expect(ceb_launches(ng.data(), d) == want + 1, "launches of Circuit::random", d, ceb_launches(ng.data(), d));
        for (uint32_t k = 0; k < d; ++k) {
            const bool in_tail = k < d - ceb_wide_layers(ng.data(), d);
            expect(in_tail == (ng[k] <= T), "a layer of Circuit::random is wide exactly when it holds more than T gates", d, k);
        }
    }
    {   // the threshold itself
        const size_t a[3] = {1, 2, T - 1}, b[3] = {1, 2, T}, c[3] = {1, 2, T + 1}, e[3] = {1, T + 1, T + 2};
        expect(ceb_wide_layers(a, 3) == 0 && ceb_wide_layers(b, 3) == 0, "T - 1 and T gates belong to the tail", 0, 0);
        expect(ceb_wide_layers(c, 3) == 1 && ceb_launches(c, 3) == 2, "T + 1 gates: one wide launch", ceb_wide_layers(c, 3), 0);
        expect(ceb_wide_layers(e, 3) == 2 && ceb_launches(e, 3) == 3, "two wide launches", ceb_wide_layers(e, 3), 0);
    }
    {   // wider again above a narrow layer: the tail keeps it; empty layers; all wide: no tail launch
        const size_t a[4] = {1, 4 * T, 2, 8 * T}, z[3] = {0, 0, 0}, w[2] = {T + 1, T + 5};
        expect(ceb_wide_layers(a, 4) == 1 && ceb_launches(a, 4) == 2, "a wide layer above a narrow one stays in the tail", ceb_wide_layers(a, 4), 0);
        expect(ceb_wide_layers(z, 3) == 0 && ceb_launches(z, 3) == 1, "empty layers", 0, 0);
        expect(ceb_wide_layers(w, 2) == 2 && ceb_launches(w, 2) == 2, "all wide: no tail launch", ceb_wide_layers(w, 2), 0);
        const uint32_t none[3] = {7, 7, 7};
        expect(ceb_first_bad_layer(z, none, 3, 0) == 3, "a layer without gates names nothing", 0, 0);
    }
    // label bounds: layers of 3, 5, 6 gates over an input of 9
    const size_t ng[3] = {3, 5, 6}, below[3] = {5, 6, 9};
    for (uint32_t k = 0; k < 3; ++k) {
        expect(ceb_below_len(ng, 3, 9, k) == below[k], "length of the table below", k, ceb_below_len(ng, 3, 9, k));
        uint32_t top[3] = {4, 5, 8};                      // every layer's largest admissible label
        expect(ceb_first_bad_layer(ng, top, 3, 9) == 3, "labels one short of the length below are in range", k, 0);
        top[k] = (uint32_t)below[k];
        expect(ceb_first_bad_layer(ng, top, 3, 9) == k, "a label equal to the length below", k, ceb_first_bad_layer(ng, top, 3, 9));
        top[k] = 0xffffffffu;
        expect(ceb_first_bad_layer(ng, top, 3, 9) == k, "the largest label there is", k, 0);
    }
    {   // two bad layers: the one evaluation reaches first; a short input
        const uint32_t top[3] = {5, 5, 9};
        expect(ceb_first_bad_layer(ng, top, 3, 9) == 2, "the first bad layer in evaluation order", 0, 0);
        const uint32_t fine[3] = {4, 5, 8};
        expect(ceb_first_bad_layer(ng, fine, 3, 8) == 2 && ceb_first_bad_layer(ng, fine, 3, 0) == 2, "a short input", 0, 0);
    }
    std::printf("checked %d\n", cases);
    return bad ? 1 : 0;
}
