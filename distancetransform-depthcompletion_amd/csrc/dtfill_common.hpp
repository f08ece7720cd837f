// dtfill_common.hpp -- constants, the routing rule and the tilings (dtfill_route.hpp), the tap table (dtfill_taps.hpp), the depth
// index rule (dtfill_index.hpp) and small device helpers shared by every kernel
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

constexpr int BIG = 1 << 20;       // in-register "infinite" distance
constexpr int INF16 = 0xFFFF;      // stored "infinite" distance in the uint16 scan arrays
constexpr int MAX_HW_SUM = 8192;   // cv2's Q16 INIT_DIST0 = INT_MAX>>2 caps distances at 8191

// frame facts as the frame's publishing block stores them (frame_publish: k_frame, or the first block of the frame in k_fused's launch):
// int32[FI_STRIDE] per frame
constexpr int FI_NSRC = 0, FI_NVAL = 1, FI_MISALIGNED = 2, FI_DLB = 3;  // DLB: lower bound of the largest distance (empty rows)
constexpr int FI_NUNRES = 4;  // tie pixels k_fin handed to k_tiesx (zeroed by the publishing block)
constexpr int FI_SKY = 5;     // l1_cv: rows [0, FI_SKY) hold no source and lie above every source: k_sky's (0: none) ...
constexpr int SKY_OFF = 0x40000000;  // ... unless this bit is set in it: k_fused calls the sky off when it has to hand on one of the two
                              // rows k_sky would start from (FI_SKY, FI_SKY + 1): the sky's rows then count as flagged 1.  The
                              // publishing block and the window blocks may run in one launch: the word starts clear (k_mask) and
                              // both OR into it.  Readers: sky_rows()
constexpr int FI_TR0 = 7;     // l1_cv, a window kernel's frame: the first row of its tiling (the rows above are the sky's: the tile rows split
                              // the rest evenly, so that no tile row is spent on rows that are not the window's)
constexpr int FI_STRIDE = 8;
constexpr int ROUTE_UNKNOWN = -0x7FFFFFFF - 1;  // route[b] from k_mask until the frame's facts are published (reads as "no window")
constexpr u32 L2_ROW_GONE = 0x40000000u;  // l2 row flag: handed to the row search up front (above any far-pixel count's threshold)

// the routing rule (route_decide, the mode bits FM_*, ROUTE_POINTS, ROUTE_PREMARK and the thresholds it rests on) and the tilings of
// the window kernel, k_l2win and k_pts: stated once, there
#include "dtfill_route.hpp"
struct PtsSrc {  // one source of a ROUTE_POINTS frame's list (k_frame writes it in raster order: index = label - 1; k_pts reads it)
    u32 rc;      // row << 16 | column
    float v;     // its depth
};

// the l1_cv parent rule's tap table (offsets, weights, parent codes, step encoding, tap_decode): stated once, there
#include "dtfill_taps.hpp"
// numpy's index rule for depth_list[label - 1] (depth_index, depth_index_pos): stated once, there
#include "dtfill_index.hpp"

// a[0..2] = a 32-pixel word a[1] of a row of bits with its left / right neighbour words: the word shifted so that
// result[c] = row[c + DJ].  The caller passes a pointer into an array (a 3-word row, or row + i of a 5-word row with i <= 2):
// all three words must lie inside it -- nothing here can check that.
template <int DJ>
__device__ __forceinline__ u32 row_shift(const u32 *a) {
    if (DJ == 0) return a[1];
    if (DJ > 0) return __builtin_amdgcn_alignbit(a[2], a[1], DJ);
    return __builtin_amdgcn_alignbit(a[1], a[0], 32 + DJ);
}

// the pixels (of 32) with (d(r) + WGT) mod 8 == d(q) mod 8, on the bit planes x0..x2 of d(r) and b0..b2 of d(q).  d is an exact
// L1 distance field, so for a tap of weight WGT <= 3 |d(r) - d(q)| <= WGT and d(r) + WGT - d(q) lies in [0, 6]: zero iff zero mod 8.
template <int WGT>
__device__ __forceinline__ u32 dist_match(u32 x0, u32 x1, u32 x2, u32 b0, u32 b1, u32 b2) {
    static_assert(WGT >= 1 && WGT <= 3, "a tap's weight");
    u32 s0, s1, s2;  // (d(r) + WGT) mod 8
    if (WGT == 1) {
        s0 = ~x0; s1 = x1 ^ x0; s2 = x2 ^ (x1 & x0);
    } else if (WGT == 2) {
        s0 = x0; s1 = ~x1; s2 = x2 ^ x1;
    } else {
        s0 = ~x0; s1 = ~(x1 ^ x0); s2 = x2 ^ (x1 | x0);
    }
    return ~((s0 ^ b0) | (s1 ^ b1) | (s2 ^ b2));
}

// outlier_removal() (dtfill_outlier.hpp) as k_outlier and k_mask both apply it: cv2's reflect-101 border ...
__device__ __forceinline__ int reflect101(int p, int n) {
    p = p < 0 ? -p : p;
    return p >= n ? 2 * n - 2 - p : p;
}

// ... and the decision for one pixel: tap(ti, tj) is the value of the 7 x 7 window's tap in row ti and column tj (0..6, the
// pixel itself at (3, 3); border already reflected)
template <class Tap>
__device__ __forceinline__ bool is_outlier(Tap tap) {
    float acc = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            if ((i < 3 ? 3 - i : i - 3) + (j < 3 ? 3 - j : j - 3) > 3) continue;  // the 25 taps of the diamond, row-major
            const float t = tap(i, j);
            acc = __fadd_rn(acc, t);  // no contraction, no reassociation
            cnt += t > 0.1f;
        }
    }
    const double mean = (double)acc / ((double)cnt + 0.00001);
    return ((double)tap(3, 3) - mean) > 1.0;
}

// What the reference's drivers do to the filled depth right after the fill, folded into the depth stores:
// rows [row0, H) only (demo.py:292-293: lidar_batch[:, 96:]) and / or the depth floor relu(d - floor) + floor in
// float32 with both roundings (eval_NYU.py:205, test.py:133).  out_depth is then [B, H - row0, W].
struct DepthEpilogue {
    int row0;
    int use_floor;
    float floor_;
};
// The drivers' depth floor np.squeeze(tf.nn.relu(d - 0.9) + 0.9) (eval_NYU.py:205, test.py:133), for the epilogue,
// k_crop_floor and k_png16: float32 step by step -- (d - 0.9f) + 0.9f is NOT d in float32, so both roundings are kept.  A NaN
// stays NaN, as max(x, 0) keeps it in TF's relu and in numpy; fmaxf would return the 0 and turn a NaN depth into the floor.
__device__ __forceinline__ float depth_floor(float d, float floor_) {
    const float t = __fsub_rn(d, floor_);
    return __fadd_rn(t < 0.0f ? 0.0f : t, floor_);
}
__device__ __forceinline__ float depth_epilogue(float d, const DepthEpilogue &ep) {
    return ep.use_floor ? depth_floor(d, ep.floor_) : d;
}

// The pass record: what the kernels of one pass share -- the batch's shape, the input, the outputs and the workspace (carve()
// in dtfill.hip lays it out).  A kernel that takes it by value only unpacks it into the __restrict__ parameters of its body:
// clang ignores __restrict__ on struct members, and without it uniform loads can no longer be proven unclobbered.  k_fused,
// k_rows, k_fin, k_l2win and k_l2env keep positional __restrict__ parameters (their launches unpack the record by name): moved
// into a forceinline body, the same code comes out with more registers (k_l2win: 51 -> 70 VGPRs, with or without the record).
struct Pass {
    int B, H, W;
    int Wd, Wp;          // 64-pixel words per row; bytes per row of a bit plane (Wd * 8)
    int nb, ctp;         // 32-row bands per frame, columns per row of ct
    int ride;            // l1_cv: the frame facts are worked out in k_fused's launch (k_mask then clears what that launch only raises)
    size_t plane_bytes;  // bytes of one plane
    const float *x;
    float src_thr, val_thr;
    float *out_depth, *out_dt;  // out_dt: the caller's, or (l1_cv with row flags, none from the caller) dscratch for k_sky
    int32_t *out_index;
    int *status;                // the caller's frame status, or the workspace's
    DepthEpilogue ep;
    // the workspace
    u64 *srcbits, *valbits;
    u16 *wpre_s, *wpre_v;
    u32 *rowcnt_s, *rowcnt_v, *rowbase_s, *rowbase_v;
    int *finfo, *fflag2;
    u32 *rowfar;         // per row: l1_cv: k_fused left a pixel undecided (-> k_rows, k_fin, k_tiesx); l2: far pixels (k_l2win -> k_l2far, k_l2env)
    int *route, *negflag;
    uint2 *ct;           // k_colT -> k_rows: per 32-row band and column {the band's source bits of the column, distances
                         // from the band's first / last row to the nearest source above / below}; rows of ctp columns
    uint4 *rec;          // k_colT -> k_fin, k_l2env: rank records, per 64-pixel word of a row (label_from_rec); null when neither
                         // labels nor depths are wanted
    u32 *spix;           // k_rows -> k_fin: per pixel, the frame offset of its nearest source in column kmin (null as rec)
    float *dscratch;     // k_fin -> k_tiesx: depths of the rows a depth epilogue drops from the output
    u32 *xlist;          // l1_cv: k_fin -> k_tiesx: the pixels whose chain left their tile; l2: k_l2win -> k_l2far: far pixels
    // l2, ROUTE_POINTS: k_l2win's idle blocks -> k_l2env: the frame's sources in raster order (such a frame has no far list: its
    // slice of xlist holds the source list)
    u32 *srclist() const { return xlist; }
    u32 *xptr;           // k_fin -> k_tiesx: where each listed pixel's chain goes on
    u8 *planes;          // k_rows -> k_fin: bit planes d & 1, d >> 1 & 1, d >> 2 & 1, live, tie; k_fin -> k_tiesx: unresolved; Wp bytes per row
    float *vlist;
    PtsSrc *ptslist;     // k_frame -> k_pts: the sources of a frame that has a handful (l1_cv, ROUTE_POINTS)
};

// the rows [0, n) of frame b that are k_sky's: FI_SKY unless the window kernel called the sky off
__device__ __forceinline__ int sky_rows(const int *__restrict__ finfo, int b) {
    const int v = finfo[b * FI_STRIDE + FI_SKY];
    return (v & SKY_OFF) ? 0 : v;
}

// row flag f of a frame whose sky is / is not k_sky's: is the row one of the any-distance kernels'?
__device__ __forceinline__ bool row_is_anydist(u32 f, int sky_live) { return f == 1u || (f == 2u && !sky_live); }

// Rank records (k_colT -> k_fin, k_l2env): per 64-pixel word of a row {low 32 source bits, sources before them in the frame,
// high 32 bits, sources before those}; records of one word column are consecutive in the row index.  The label of the source
// at (si, sj) = 1 + its raster rank among the frame's sources (cv2's label init) = one 8-byte read + a popcount.
__device__ __forceinline__ int label_from_rec(const uint2 *__restrict__ rec_f /* the frame's records */, int H, int si, int sj) {
    const uint2 r = rec_f[(((size_t)(sj >> 6) * H + si) << 1) + ((sj >> 5) & 1)];
    return (int)r.y + __popc(r.x & ((1u << (sj & 31)) - 1u)) + 1;
}
