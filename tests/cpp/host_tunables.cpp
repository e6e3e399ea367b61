// csrc/tunables.hpp on its own (g++, no HIP): every entry of the list, then every entry's value under the environment this program
// was started with.  tests/test_tunables_cpu.py runs it under a matrix of values and compares with the expectations written there.
#include <cstdio>

#include "../../zk-cryptography_amd/csrc/tunables.hpp"

int main() {
    using namespace zk::env;
    static const char* kinds[] = {"flag", "int", "bytes", "text"};
    auto num = [](long long v) {
        if (v == UNSET) std::printf("unset"); else std::printf("%lld", v);
    };
    for (const Switch& s : ALL) {
        std::printf("entry %s %s def=", s.name, kinds[s.kind]);
        num(s.def);
        std::printf(" lo=%lld hi=%lld %s %s | %s\n", s.lo, s.hi, s.outside == CLAMPED ? "clamped" : "ignored", s.when == ONCE ? "once" : "fresh", s.meaning);
    }
    for (const Switch& s : ALL) {
        std::printf("value %s ", s.name);
        if (s.kind == TEXT) { const char* t = text(s); if (t) std::printf("text:%s", t); else std::printf("unset"); }
        else if (s.kind == BYTES) std::printf("%llu", (unsigned long long)read(s));
        else num(read(s));
        std::printf("\n");
    }
    return 0;
}
