// Prints numpy's index rule for depth_list[label - 1] as the kernels' header states it, one line per case:
//   full label nval idx ok     depth_index, for every nval in 0..6 and label in 0..nval + 2
//   pos  label nval idx ok     depth_index_pos, the same cases with label >= 1 (its precondition)
// Host-only: tests/test_depth_index.py compiles it with the host compiler and compares the lines with numpy itself.
#include <cstdio>

#include "dtfill_index.hpp"

// the rule is constexpr: a kernel's call site may take it at compile time
static_assert(depth_index(0, 3).ok && depth_index(0, 3).idx == 2, "label 0 wraps to the last value");
static_assert(!depth_index(0, 0).ok && !depth_index_pos(4, 3).ok && depth_index_pos(3, 3).ok, "outside [0, nval)");

int main() {
    for (int nval = 0; nval <= 6; ++nval)
        for (int label = 0; label <= nval + 2; ++label) {
            const DepthIndex f = depth_index(label, nval);
            std::printf("full %d %d %d %d\n", label, nval, f.idx, (int)f.ok);
            if (label >= 1) {
                const DepthIndex p = depth_index_pos(label, nval);
                std::printf("pos %d %d %d %d\n", label, nval, p.idx, (int)p.ok);
            }
        }
    return 0;
}
