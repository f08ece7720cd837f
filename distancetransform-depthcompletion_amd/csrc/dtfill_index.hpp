// dtfill_index.hpp -- numpy's index rule for depth_list[label - 1]: the ONE place where it is written down
// Part of libdtfill.so (included by dtfill_common.hpp).  Plain C++14, no HIP and no other header: a host compiler reads it as it
// stands (tests/test_depth_index.py prints it and compares it with numpy itself).
#pragma once

// The reference fills a pixel with depth_list[label - 1] (tools.py:26), depth_list = x[with_value] (tools.py:24) holding nval
// values, label = 1 + raster rank of the pixel's nearest source, or 0 in a frame without a source.  numpy's rule for an integer
// index: -1 (label 0) wraps to the LAST value; anything else outside [0, nval) raises IndexError, which here is the frame's
// status bit DTFILL_FRAME_INDEX_ERROR.  With nval == 0 the wrapped index is still -1: an error too.
// What a kernel does with the answer is its own: which array it gathers from, NaN for a pixel that is not ok, its in-image
// masks, and one atomicOr per thread at the end.
struct DepthIndex {
    int idx;  // the element of depth_list; meaningful only if ok
    bool ok;  // false: numpy's IndexError
};

// the full rule, label >= 0
constexpr DepthIndex depth_index(int label, int nval) {
    int idx = label - 1;
    if (idx < 0) idx += nval;  // numpy: index -1 wraps to the last element
    return DepthIndex{idx, idx >= 0 && idx < nval};
}

// PRECONDITION: label >= 1 (the pixel has a nearest source).  No wrap can occur, so none is computed: idx = label - 1.
constexpr DepthIndex depth_index_pos(int label, int nval) { return DepthIndex{label - 1, label - 1 < nval}; }
