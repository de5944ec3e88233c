// Dumps the table of scv_expected_majority_i32 (csrc/scvote_expected_table.h, the library's own code) on the CPU: built and run by
// tests/test_expected_table.py, which checks the binomials, the Gauss-Legendre rules and the CPU mirror's rules against it.
// Output: the word count, then one line per double, its IEEE-754 bits in hex (lossless).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../o1_inference_scaling_laws_amd/csrc/scvote_expected_table.h"

int main() {
    std::vector<double> t;
    scv::build_expected_table(t);
    std::printf("%d %d %d\n", (int)t.size(), scv::kExpectedBinomWords, scv::kExpectedMaxQ);
    for (double d : t) {
        uint64_t u;
        std::memcpy(&u, &d, sizeof u);
        std::printf("%016" PRIx64 "\n", u);
    }
    return 0;
}
