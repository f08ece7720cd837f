// Prints the l1_cv tap table as the kernels' header states it, one line per parent code 0..15:
//   code di dj weight encoding forward, then the offset tap_decode returns for the code
// Host-only: tests/test_tap_table.py compiles it with the host compiler and compares the lines with tests/parallel_model.py.
#include <cstdio>

#include "dtfill_taps.hpp"

template <int CODE>
static void line() {
    // through template constants, as the kernels' call sites take them
    constexpr int di = code_di(CODE), dj = code_dj(CODE), w = code_weight(CODE), enc = code_enc(CODE);
    int ddi = 99, ddj = 99;
    tap_decode(CODE, ddi, ddj);
    std::printf("%d %d %d %d %d %d %d %d\n", CODE, di, dj, w, enc, (int)code_fwd(CODE), ddi, ddj);
}
template <int... C>
static void lines() {
    int unused[] = {(line<C>(), 0)...};
    (void)unused;
}

int main() {
    lines<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15>();
    std::printf("nibbles %08x %08x\n", TAP_DI_NIB, TAP_DJ_NIB);
    for (int t = 0; t < 8; ++t) std::printf("tap %d %d %d\n", t, tap_di(t), tap_dj(t));
    return 0;
}
