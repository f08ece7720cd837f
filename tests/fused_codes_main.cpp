// Prints the plane codes of the window kernel as the kernels' header states them (dtfill_taps.hpp):
//   one line per plane code 0..15: code, the step of the constexpr table, the step code_step returns at run time, code_wins
//   then "reserved <CODE_SOURCE> <CODE_NONE>", "plane <plane_code(0..15)>" and the tap offsets, "tap t di dj"
// Host-only: tests/test_fused_codes.py compiles it with the host compiler.
#include <cstdio>

#include "dtfill_taps.hpp"

int main() {
    for (int c = 0; c < 16; ++c) {
        int di = 99, dj = 99;
        code_step(c, di, dj);
        std::printf("%d %d %d %d %d %d\n", c, CODE_STEP.v[c][0], CODE_STEP.v[c][1], di, dj, (int)code_wins(c));
    }
    std::printf("reserved %d %d\n", CODE_SOURCE, CODE_NONE);
    std::printf("plane");
    for (int c = 0; c < 16; ++c) std::printf(" %d", plane_code(c));
    std::printf("\n");
    for (int t = 0; t < 8; ++t) std::printf("tap %d %d %d\n", t, TAP_OFFSET[t][0], TAP_OFFSET[t][1]);
    return 0;
}
