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

// ---- The plane code of the window kernel (dtfill_fused.hpp): what its four code planes and its step bytes (2 * plane code) hold.
// A winner's plane code is its parent code itself.  Two parent codes can never win there, so they are free to mean "source" and
// "undecided", both of step (0, 0):
//   Backward tap 5 (code 13, offset (1, -1), weight 2) and backward tap 6 (code 14, offset (1, -2), weight 3) never select.
//   A backward tap of weight w matches at q iff r = q + offset lies in the window's image part, is decided, and d(r) + w = d(q);
//   d is the L1 distance to the nearest source inside that part, a rectangle, so |d(a) - d(b)| <= |a - b|_1 for its pixels.  Let
//   code 13 or 14 match at q, and s = q + (1, 0): s shares its row with r and its column with q, so it lies in the rectangle too.
//   |s - r|_1 = w - 1 gives d(s) <= d(r) + w - 1 = d(q) - 1, and |s - q|_1 = 1 gives d(s) >= d(q) - 1.  So d(s) = d(q) - 1 < d(q):
//   s was decided at an earlier level, and backward tap 4 (code 12, offset (1, 0), weight 1) matches at q.  Tap 4 comes first, so
//   q is taken before taps 5 and 6 are asked -- and every pixel they would add to the taken mask is in it already, which is why
//   leaving them out changes nothing for tap 7 either.  (fin_body, dtfill_rows.hpp, says the same of its own chain and keeps them.)
// The facts of the table that the argument rests on:
static_assert(code_di(12) == 1 && code_dj(12) == 0 && code_weight(12) == 1, "code 12 steps one row down");
static_assert(code_di(13) == 1 && code_di(14) == 1, "codes 13 and 14 read the row that code 12 reads");
static_assert((code_dj(13) < 0 ? -code_dj(13) : code_dj(13)) == code_weight(13) - 1 &&
              (code_dj(14) < 0 ? -code_dj(14) : code_dj(14)) == code_weight(14) - 1, "their candidates lie weight - 1 beside code 12's");
constexpr int plane_code(int code) { return code; }
constexpr int CODE_SOURCE = 13;  // a source: the root of a chain
constexpr int CODE_NONE = 14;    // an undecided pixel
constexpr bool code_wins(int code) { return code != CODE_SOURCE && code != CODE_NONE; }

// the step of a plane code: code -> (di, dj), (0, 0) for the two reserved codes
struct CodeStepTable {
    int v[16][2];
    constexpr CodeStepTable() : v{} {
        for (int c = 0; c < 16; ++c) {
            v[c][0] = code_wins(c) ? code_di(c) : 0;
            v[c][1] = code_wins(c) ? code_dj(c) : 0;
        }
    }
};
constexpr CodeStepTable CODE_STEP{};
// the same for a plane code known only at run time
constexpr void code_step(int code, int &di, int &dj) {
    tap_decode(code, di, dj);
    if (!code_wins(code)) di = dj = 0;
}
constexpr bool code_step_agrees(int c = 0) {
    int di = 9, dj = 9;
    if (c == 16) return true;
    code_step(c, di, dj);
    return di == CODE_STEP.v[c][0] && dj == CODE_STEP.v[c][1] && code_step_agrees(c + 1);
}
static_assert(code_step_agrees(), "code_step and CODE_STEP are one table");
