// dtfill_taps.hpp -- the 5x5 tap table of the l1_cv parent rule: the ONE place where its offsets are written down
// Part of libdtfill.so (included by dtfill_common.hpp).  Plain C++14, no HIP and no other header: a host compiler reads it as it
// stands (tests/test_tap_table.py prints it and compares it with tests/parallel_model.py).
#pragma once

// cv2 tap order (OpenCV 3.4 distanceTransformEx_5x5): forward taps t = 0..7 as (di, dj); the weight of a tap is |di| + |dj|.
// Backward tap t is the NEGATED forward tap t with the same weight.  The first match wins: forward taps in this order for a
// live pixel, backward taps in this order for the others.
constexpr int TAP_OFFSET[8][2] = {{-2, -1}, {-2, 1}, {-1, -2}, {-1, -1}, {-1, 0}, {-1, 1}, {-1, 2}, {0, -1}};
constexpr int tap_di(int t) { return TAP_OFFSET[t][0]; }
constexpr int tap_dj(int t) { return TAP_OFFSET[t][1]; }

// Parent code 0..15 = t (forward) or t | 8 (backward): its offset, its weight, and the step encoding (di + 2) << 3 | (dj + 2)
// that the code planes and step bytes hold (18 = step (0, 0): a source, or no step)
constexpr bool code_fwd(int code) { return !(code & 8); }
constexpr int code_di(int code) { return code_fwd(code) ? tap_di(code & 7) : -tap_di(code & 7); }
constexpr int code_dj(int code) { return code_fwd(code) ? tap_dj(code & 7) : -tap_dj(code & 7); }
constexpr int code_weight(int code) { return (code_di(code) < 0 ? -code_di(code) : code_di(code)) + (code_dj(code) < 0 ? -code_dj(code) : code_dj(code)); }
constexpr int code_enc(int code) { return (code_di(code) + 2) << 3 | (code_dj(code) + 2); }

// the table packed for a run-time lookup: nibble t = offset(t) + 2
constexpr unsigned tap_nibbles(int axis, int t = 0) { return t == 8 ? 0u : (unsigned)(TAP_OFFSET[t][axis] + 2) << (4 * t) | tap_nibbles(axis, t + 1); }
constexpr unsigned TAP_DI_NIB = tap_nibbles(0), TAP_DJ_NIB = tap_nibbles(1);

// the offset of a parent code known only at run time
constexpr void tap_decode(int code, int &di, int &dj) {
    const int sh = (code & 7) * 4;
    di = (int)((TAP_DI_NIB >> sh) & 15u) - 2;
    dj = (int)((TAP_DJ_NIB >> sh) & 15u) - 2;
    if (code & 8) {
        di = -di;
        dj = -dj;
    }
}
