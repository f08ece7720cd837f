// dtfill_convb.hpp -- the backward pass of dtfill_conv2d in a fixed summation order: dx, dw and db of the layers of
// SparsityCNN (solution_DeepNet/net.py:11-242), what train.py:232-254's tape needs of a convolution.  include/dtfill.h,
// dtfill_conv2d_backward_data() and dtfill_conv2d_backward_weights(), has the contracts.  Part of libdtfill.so; included by
// dtfill.hip inside its anonymous namespace, after dtfill_conv.hpp, whose kernels the input gradient runs on.  The kernels of
// the wide layers of ResNet18_NO_BN_l2 (dtfill_conv2d_strided, dtfill_conv2d_transpose) are the second part of this file, the
// weight gradient of the image layer (dtfill_conv2d_image) the third; the
// host side, the last, is one path for all seven entry points: dtfill.hip's convb_plan checks a ConvBwLayer's domain and derives
// its frames, segment counts and workspace layout (ConvBwPlan), and convb_data_launch and convb_weights_launch each hold one
// dispatch, in which the narrow layers' kernels are branches beside the wide ones'.
#pragma once

// ------------------------------------------------------------------------------------------------
// g = y > 0 ? dy : dy * alpha is the gradient at the convolution's chain (convb_g), and both gradients are sums over it.
//
// dx is a forward convolution: dtfill_conv2d's chain over g with the kernel flipped and its channel axes exchanged.  So
// k_convb_g writes g densely into the workspace, k_convb_flip writes wT behind it (the weights change every step: the repack
// runs on the device, each call), and the layer runs on dtfill_conv.hpp's kernels as they are: conv_stage, conv_slot and
// conv_tap are not restated here.  Which kernel follows from the backward layer's channels, Cout -> Cin:
//   Cin == 1 or 16   conv_launch: k_conv_mfma (Cout == 1: its Cin == 1 form, a k-step of four taps), k_conv_chain for Cin == 1
//   Cin >= 32        conv_strided_launch at stride 1: k_conv_wide, one pass of Cin / 16 N-tiles
//   Cin >= 32 of a Cout == 1 layer: Cin / 16 launches of k_conv_mfma's Cin == 1 form, each with its 16 columns of wT (repacked
//                    as [Cin / 16][taps][16]) into its 16 channels of dx
// g costs one write and one read of B H W Cout floats beside a layer that reads it ksize^2 times from LDS.
//
// dw and db are a reduction over all B H W pixels: an implicit GEMM with K = the pixels.  An accumulator of
// v_mfma_f32_16x16x4_f32 is D[row][o], 16 rows of (tap, input channel) by the 16 output channels; a k-step is four consecutive
// pixels of a frame row; A[row][k] is x at the pixel under the tap, B[k][o] is g at the pixel.  The MFMA adds its four
// k-products in k order with one rounding each (what dtfill_conv2d's contract rests on, measured by its tests), so a run of
// MFMAs whose k index walks a segment's pixels in raster order IS the contract's level-1 chain, for 256 (row, o) at once.
//   k_convb_dw      Cout == 16.  A work item is (segment, group of 16 input channels), the group fastest; a block of four
//                   waves walks the segment in strips of CB_RS rows: the haloed strip of x (this group's channels) and the
//                   strip of g are staged in LDS, then every wave walks the strip's k-steps for its taps: wave w holds the
//                   taps w, w + 4, ..., one accumulator each (13 for 7x7: 13 independent chains hide the MFMA's 40 cycles of
//                   dependent latency), a row of the tile being an input channel of the group.  One g operand serves all of a
//                   wave's taps.  db is one more accumulator on wave 3 (the wave with the fewest taps) whose A operand is 1.0f.
//                   Cin == 1: the rows of a tile are 16 taps, a wave holds tile w of ceil((taps + 1) / 16), and row `taps`, the
//                   first free one, is the row of ones that makes db.
//                   The LDS images are plain, [pixel][16 channels]: lane (row m, k index kq) reads one float at pixel p + kq,
//                   channel m, so a wave reads 64 consecutive floats, without a bank conflict and without conv_slot's exchange
//                   (which serves the forward's 16-byte reads of four channels); a tap is a constant offset.
//                   A pixel beyond the frame's right edge in the last k-step of a row has zero operands on both sides, +0 * +0
//                   added to the chain: only the sign of a zero can change.  Rows beyond the frame are not walked.
//   k_convb_dw_lane Cout == 1 (correct_4, conv_output: under 0.3 % of the work): one lane per (tap, channel), and one for db,
//                   walks the segment literally.
//   k_convb_sum     level 2: element e of dw and db is the sequential sum of the segments' partials in (b, t, s) order.
// The partials of segment n lie at part[n (rows + 1) Cout ..]: [row][o] as dw is, then db's Cout.
// ------------------------------------------------------------------------------------------------
constexpr int CB_R = DTFILL_CONV_BW_ROWS;  // a segment: rows ...
constexpr int CB_C = DTFILL_CONV_BW_COLS;  // ... and pixels of a row
constexpr int CB_RS = 4;                   // rows of a strip: what a block stages at a time
constexpr int CBL_AHEAD = 8;               // k_convb_dw_lane: links whose operands are in flight together (16 spills SGPRs)
static_assert(CB_R % CB_RS == 0 && CB_C % 4 == 0, "a segment is whole strips of whole k-steps");

struct ConvBwArgs {
    const float *x, *dy, *y;  // dy and y at their channel offset; y NULL for a linear layer
    int dy_channels, y_channels;
    int B, H, W, Cin, Cout, act;
    float alpha;
    int segs_y, segs_x;
    bool xvec, gvec;  // x / dy and y allow 16-byte loads
};

// the gradient at the convolution's chain: a float32 compare on the forward output and one rounded multiply
__device__ __forceinline__ float convb_g(float dy, float y, int act, float alpha) {
#pragma clang fp contract(off)
    return act == DTFILL_CONV_LEAKY ? (y > 0.0f ? dy : dy * alpha) : dy;
}

// g[n, o] of all n pixels of dy's frames, dense; g2 (the wide layers' dresidual, which is g itself) is a second copy, or NULL
__global__ __launch_bounds__(256) void k_convb_g(ConvBwArgs a, float *__restrict__ g, float *__restrict__ g2, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long pixel = idx / a.Cout;
    const int o = (int)(idx - pixel * a.Cout);
    const float dy = a.dy[pixel * a.dy_channels + o];
    const float v = convb_g(dy, a.y ? a.y[pixel * a.y_channels + o] : 0.0f, a.act, a.alpha);
    g[idx] = v;
    if (g2) g2[idx] = v;
}

// wT[i, j, o, c] = w[ksize - 1 - i, ksize - 1 - j, c, o]; `blocked` (Cout == 1, Cin >= 32): [c / 16][tap][c % 16]
// without `flip` the taps stay where they are, wX[i, j, o, c] = w[i, j, c, o]: the stride-2 and the transposed wide layers
__global__ __launch_bounds__(256) void k_convb_flip(const float *__restrict__ w, float *__restrict__ wt, int taps, int Cin, int Cout,
                                                    bool blocked, bool flip) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= taps * Cin * Cout) return;
    const int o = idx % Cout, c = idx / Cout % Cin, tap = idx / Cout / Cin;
    const int ft = flip ? taps - 1 - tap : tap;  // (ksize - 1 - i) ksize + (ksize - 1 - j)
    wt[blocked ? ((c / 16) * taps + ft) * 16 + c % 16 : (ft * Cout + o) * Cin + c] = w[idx];
}

// g of the channels c .. c + 3 of a pixel of dy's and y's frames; vec: by 16-byte loads
__device__ __forceinline__ cv_f4 convb_g4(const ConvBwArgs &a, size_t pixel, int c, bool vec) {
    const float *pd = a.dy + pixel * a.dy_channels + c;
    cv_f4 f = vec ? *reinterpret_cast<const cv_f4 *>(pd) : cv_f4{pd[0], pd[1], pd[2], pd[3]};
    if (a.act == DTFILL_CONV_LEAKY) {
        const float *py = a.y + pixel * a.y_channels + c;
        const cv_f4 y = vec ? *reinterpret_cast<const cv_f4 *>(py) : cv_f4{py[0], py[1], py[2], py[3]};
        f = cv_f4{convb_g(f.x, y.x, a.act, a.alpha), convb_g(f.y, y.y, a.act, a.alpha), convb_g(f.z, y.z, a.act, a.alpha),
                  convb_g(f.w, y.w, a.act, a.alpha)};
    }
    return f;
}

// what a strip of g is: rows h1 .. h1 + CB_RS - 1, columns v0 .. v0 + CB_C - 1 of frame fb, +0 outside the frame, [pixel][16]
__device__ __forceinline__ void convb_stage_g(float *s_g, const ConvBwArgs &a, size_t fb, int h1, int v0, int t) {
    for (int e = t; e < CB_RS * CB_C * 4; e += 256) {
        const int p = e >> 2, s = e & 3;  // channels 4 s .. 4 s + 3 of pixel p of the strip
        const int row = p / CB_C, col = p - row * CB_C;
        const int h = h1 + row, v = v0 + col;
        cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
        if (h < a.H && v < a.W) f = convb_g4(a, fb + (size_t)h * a.W + v, 4 * s, a.gvec);
        *reinterpret_cast<cv_f4 *>(s_g + p * 16 + 4 * s) = f;
    }
}

template <int KS, bool CIN1>
__global__ __launch_bounds__(256, 2) void k_convb_dw(ConvBwArgs a, float *__restrict__ part, long long n_items) {
    constexpr int R = (KS - 1) / 2, TAPS = KS * KS, PC = CIN1 ? 1 : CV_G;
    constexpr int LH = CB_RS + KS - 1, LW = CB_C + KS - 1;
    constexpr int NT = CIN1 ? 1 : (TAPS + 3) / 4;  // accumulators a wave
    static_assert(TAPS % 16 != 0, "the Cin == 1 tiles have a free row for db");
    __shared__ __attribute__((aligned(16))) float s_x[LH * LW * PC];
    __shared__ __attribute__((aligned(16))) float s_g[CB_RS * CB_C * 16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;  // A: row m, pixel kq; B: pixel kq, output channel m; D: channel m, rows 4 kq ..+3
    const int H = a.H, W = a.W, Cin = a.Cin;
    const int groups = CIN1 ? 1 : Cin / CV_G;
    const size_t pstride = ((size_t)TAPS * Cin + 1) * 16;
    // the lane's float offset into s_x of accumulator n's operand, at the strip's first pixel
    int aoff[NT];
    const int mytap = 16 * wave + m;  // Cin == 1: the lane's row as a tap; TAPS: the row of ones; beyond: unused
    if (CIN1) {
        aoff[0] = mytap < TAPS ? (mytap / KS) * LW + mytap % KS + kq : 0;
    } else {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const int tap = min(wave + 4 * n, TAPS - 1);
            aoff[n] = ((tap / KS) * LW + tap % KS + kq) * CV_G + m;
        }
    }
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int g = (int)(item % groups);
        const long long seg = item / groups;
        const int sx = (int)(seg % a.segs_x), sy = (int)(seg / a.segs_x % a.segs_y), b = (int)(seg / a.segs_x / a.segs_y);
        const int h0 = sy * CB_R, v0 = sx * CB_C;
        const size_t fb = (size_t)b * H * W;
        const float *xb = a.x + fb * Cin;
        const int cols = min(CB_C, W - v0), steps = (cols + 3) / 4, whole = cols / 4;  // k-steps of a row; those wholly inside
        cv_f4 acc[NT], accb{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int h1 = h0; h1 < min(h0 + CB_R, H); h1 += CB_RS) {
            // ---- the haloed strip of x, +0 outside the frame, and the strip of g ----
            if (CIN1) {
                for (int p = t; p < LH * LW; p += 256) {
                    const int r = p / LW, c = p - r * LW;
                    const int h = h1 + r - R, v = v0 + c - R;
                    s_x[p] = h >= 0 && h < H && v >= 0 && v < W ? xb[(size_t)h * W + v] : 0.0f;
                }
            } else {
                for (int e = t; e < LH * LW * 4; e += 256) {
                    const int p = e >> 2, s = e & 3;
                    const int r = p / LW, c = p - r * LW;
                    const int h = h1 + r - R, v = v0 + c - R;
                    cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
                    if (h >= 0 && h < H && v >= 0 && v < W) {
                        const float *src = xb + ((size_t)h * W + v) * Cin + g * CV_G + 4 * s;
                        f = a.xvec ? *reinterpret_cast<const cv_f4 *>(src) : cv_f4{src[0], src[1], src[2], src[3]};
                    }
                    *reinterpret_cast<cv_f4 *>(s_x + p * CV_G + 4 * s) = f;
                }
            }
            convb_stage_g(s_g, a, fb, h1, v0, t);
            __syncthreads();
            // ---- the strip's links of every chain, in raster order ----
            const int rows = min(CB_RS, H - h1);
            // one k-step: pixels 4 s .. 4 s + 3 of the strip's row.  EDGE: the row's last step where the frame ends inside it,
            // the only one whose lanes can lie beyond the frame (their g is staged as +0; their x operand is made +0 here)
            auto k_step = [&](auto edge, int row, int s) {
                const bool real = !decltype(edge)::value || v0 + 4 * s + kq < W;
                const float gv = s_g[(row * CB_C + 4 * s + kq) * 16 + m];
                const int at = (row * LW + 4 * s) * PC;
                if (CIN1) {
                    const float xv = mytap < TAPS ? s_x[at + aoff[0]] : mytap == TAPS ? 1.0f : 0.0f;
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(real ? xv : 0.0f, gv, acc[0], 0, 0, 0);
                } else {
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        if (wave + 4 * n < TAPS) {
                            const float xv = s_x[at + aoff[n]];
                            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(real ? xv : 0.0f, gv, acc[n], 0, 0, 0);
                        }
                    if (wave == 3) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(real ? 1.0f : 0.0f, gv, accb, 0, 0, 0);
                }
            };
            if (!CIN1 || 16 * wave <= TAPS) {
#pragma unroll 1
                for (int row = 0; row < rows; ++row) {
#pragma unroll 1
                    for (int s = 0; s < whole; ++s) k_step(std::false_type{}, row, s);
                    if (whole < steps) k_step(std::true_type{}, row, whole);
                }
            }
            __syncthreads();  // the strips are rewritten by the next one, or the next item
        }
        // ---- the segment's partials: [row][o], then db ----
        float *ps = part + (size_t)seg * pstride;
        if (CIN1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = 16 * wave + 4 * kq + e;
                if (row <= TAPS) ps[row * 16 + m] = acc[0][e];
            }
        } else {
#pragma unroll
            for (int n = 0; n < NT; ++n)
                if (wave + 4 * n < TAPS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) ps[((size_t)(wave + 4 * n) * Cin + g * CV_G + 4 * kq + e) * 16 + m] = acc[n][e];
                }
            if (wave == 3 && g == 0 && kq == 0) ps[(size_t)TAPS * Cin * 16 + m] = accb[0];
        }
    }
}

// Cout == 1: lane blockIdx.y * 256 + threadIdx.x is a (tap, channel) of dw, or the last one db; segment blockIdx.x
__global__ __launch_bounds__(256) void k_convb_dw_lane(ConvBwArgs a, int ksize, float *__restrict__ part) {
#pragma clang fp contract(off)
    const int H = a.H, W = a.W, Cin = a.Cin, r = (ksize - 1) / 2;
    const int nrow = ksize * ksize * Cin, row = blockIdx.y * 256 + threadIdx.x;
    if (row > nrow) return;
    const bool ones = row == nrow;
    const int tap = ones ? 0 : row / Cin, c = ones ? 0 : row - tap * Cin, i = tap / ksize - r, j = tap % ksize - r;
    const int seg = blockIdx.x;
    const int sx = seg % a.segs_x, sy = seg / a.segs_x % a.segs_y, b = seg / a.segs_x / a.segs_y;
    const int h0 = sy * CB_R, v0 = sx * CB_C;
    const size_t fb = (size_t)b * H * W;
    const int vend = min(v0 + CB_C, W);
    float acc = 0.0f;
    for (int h = h0; h < min(h0 + CB_R, H); ++h)
        for (int v1 = v0; v1 < vend; v1 += CBL_AHEAD) {
            // the operands of CBL_AHEAD links are asked for together, then the links are made in order: one memory latency a
            // group, not one a link (a lane past the row's end asks for the group's first pixel again and makes no link)
            float xs[CBL_AHEAD], gs[CBL_AHEAD];
#pragma unroll
            for (int u = 0; u < CBL_AHEAD; ++u) {
                const int v = v1 + u < vend ? v1 + u : v1;
                const size_t pixel = fb + (size_t)h * W + v;
                gs[u] = convb_g(a.dy[pixel * a.dy_channels], a.y ? a.y[pixel * a.y_channels] : 0.0f, a.act, a.alpha);
                const int hh = h + i, vv = v + j;
                const bool inside = hh >= 0 && hh < H && vv >= 0 && vv < W;
                xs[u] = ones ? 1.0f : inside ? a.x[(fb + (size_t)hh * W + vv) * Cin + c] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < CBL_AHEAD; ++u)
                if (v1 + u < vend) acc = fmaf(xs[u], gs[u], acc);
        }
    part[(size_t)seg * (nrow + 1) + row] = acc;
}

// level 2: out element e = the partials of the segments 0 .. nseg - 1 added in that order, from +0
__global__ __launch_bounds__(256) void k_convb_sum(const float *__restrict__ part, int pstride, int nseg, int ndw, float *__restrict__ dw,
                                                   float *__restrict__ db) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= pstride) return;
    float acc = 0.0f;
#pragma unroll 8
    for (int n = 0; n < nseg; ++n) acc = acc + part[(size_t)n * pstride + e];
    if (e < ndw)
        dw[e] = acc;
    else if (db)
        db[e - ndw] = acc;
}

template <int KS>
void convb_dw_launch(hipStream_t st, const ConvBwArgs &a, float *part, long long nseg) {
    const long long n_items = a.Cin == 1 ? nseg : nseg * (a.Cin / CV_G);
    const int grid = (int)(n_items < CV_MAX_BLOCKS ? n_items : CV_MAX_BLOCKS);
    if (a.Cin == 1)
        k_convb_dw<KS, true><<<grid, 256, 0, st>>>(a, part, n_items);
    else
        k_convb_dw<KS, false><<<grid, 256, 0, st>>>(a, part, n_items);
}

// ------------------------------------------------------------------------------------------------
// The wide layers: the backward of dtfill_conv2d_strided and dtfill_conv2d_transpose (include/dtfill.h has the contracts).
//
// dx runs on dtfill_conv.hpp's kernels as they are, behind k_convb_g (which also writes dresidual, g itself) and k_convb_flip:
//   stride 1                 conv_strided_launch at stride 1 over g under wT, as above
//   stride 2, 3x3            conv_transpose_launch over g [B,H/2,W/2,Cout] under wX (the channel axes exchanged, no flip)
//   stride 2, 1x1            the same chain has the single tap (0, 0): conv_strided_launch (1x1, stride 1) over g under wX into
//                            the workspace, and k_convb_spread writes it to the even pixels of dx and +0 to the others
//   transposed               conv_strided_launch (3x3, stride 2) over g [B,2H,2W,Cout] under wX
//
// dw and db.  The sum has a SMALL frame, the one the segments lie over and whose pixels are the k index, and a LARGE frame
// that is read under the taps at (S h + i - P, S v + j - P): the output and the input frame of a strided layer (S its stride,
// P = (ksize - 1) / 2 at stride 1 and 0 at stride 2, where H and W are even), the input and the output frame of the
// transposed one (S = 2, P = 0).  k_convb_dw_wide is k_convb_dw over that pair, with one more loop: a work item is (segment,
// group of 16 channels of the large tensor, pass of CBW NB tiles of 16 channels of the small tensor), and the staged strip of
// the large tensor's group serves the NB tiles, one accumulator per (tap of the wave, tile).  TR says which tensor carries
// the derivative: the small one (g, a strided layer; the B operand, x under the tap is A) or the large one (g under the tap
// is B, a transposed layer; x is A).  The product is commutative and the MFMA's k order is the pixels' either way.
// At S = 2 the strip of the large tensor is staged split by column parity, [row][parity][column / 2][16], so that a tap is a
// constant offset again and a wave reads 64 consecutive floats (the plain image would have lanes 32 floats apart on the same
// bank pairs: a two-way conflict).
// db of a strided layer is one more accumulator per tile on wave 3 of the items of group 0, its A operand 1.0f; db of the
// transposed layer is four, the chains q[ky][kx] of the header over g under the taps (0,0), (0,1), (1,0), (1,1), on wave 3
// of the items of pass 0, added as ((q00 + q01) + q10) + q11.
// ------------------------------------------------------------------------------------------------
struct ConvBwWide {
    ConvBwArgs b;  // b.H, b.W: the SMALL frame, the one the segments lie over
    int HL, WL;    // the large frame
};

template <int KS, int S>
struct ConvBwGeo {
    static constexpr int RS = S == 1 ? 2 : 1;     // rows of the small frame a strip
    static constexpr int NB = KS <= 3 ? 4 : 1;    // tiles of the small tensor a pass (13 taps a wave at 7x7: one)
    static constexpr int P = S == 1 ? (KS - 1) / 2 : 0;
    static constexpr int TAPS = KS * KS, NT = (TAPS + 3) / 4;
    static constexpr int LH = (RS - 1) * S + KS, LWS = (CB_C - 1) * S + KS, LWH = CB_C + (KS - 1 + S - 1) / S;
    // the float offset of tap (i, j) in the image [LH][S][LWH][16] from the pixel under tap (0, 0)
    static __device__ __forceinline__ int tap_offset(int i, int j) { return ((i * S + j % S) * LWH + j / S) * 16; }
};

// dx of a 1x1 stride-2 layer: the chain's value at the even pixels, +0 elsewhere.  t: [B,H/2,W/2,Cin] dense
__global__ __launch_bounds__(256) void k_convb_spread(const float *__restrict__ t, float *__restrict__ dx, int H, int W, int Cin,
                                                      int dx_channels, int dx_offset, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long pixel = idx / Cin;
    const int c = (int)(idx - pixel * Cin);
    const int v = (int)(pixel % W), h = (int)(pixel / W % H);
    const long long b = pixel / W / H;
    const bool even = !((h | v) & 1);
    dx[pixel * dx_channels + dx_offset + c] = even ? t[((b * (H / 2) + h / 2) * (W / 2) + v / 2) * Cin + c] : 0.0f;
}

template <int KS, int S, bool TR, bool VEC>
__global__ __launch_bounds__(256, 2) void k_convb_dw_wide(ConvBwWide a, float *__restrict__ part, unsigned seg0, unsigned gl0) {
    typedef ConvBwGeo<KS, S> G;
    constexpr int RS = G::RS, NB = G::NB, TAPS = G::TAPS, NT = G::NT, LH = G::LH, LWS = G::LWS, LWH = G::LWH;
    constexpr int NDB = TR ? 4 : NB;
    __shared__ __attribute__((aligned(16))) float s_l[LH * S * LWH * 16];
    __shared__ __attribute__((aligned(16))) float s_s[NB * RS * CB_C * 16];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;  // A: row m, pixel kq; B: pixel kq, column m; D: column m, rows 4 kq ..+3
    const int Hs = a.b.H, Ws = a.b.W, HL = a.HL, WL = a.WL;
    const unsigned Cin = a.b.Cin, Cout = a.b.Cout;
    const int tiles = (TR ? Cin : Cout) / 16;
    int aoff[NT], boff[4];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int tap = min(wave + 4 * n, TAPS - 1);
        aoff[n] = G::tap_offset(tap / KS, tap % KS) + kq * 16 + m;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) boff[q] = TR ? G::tap_offset(q >> 1, q & 1) + kq * 16 + m : 0;
    // a work item is (segment, group, pass), one a block: the pass is the grid's x, the group its y from gl0 on, the segment
    // its z from seg0 on (the launch is repeated where a grid axis is too short).  A loop over a linear index, its 64-bit
    // divisions and signed sizes cost some twenty scalar registers more than there are.  Every pixel index is below 2^31,
    // the entry points' rule.
    const unsigned pass = blockIdx.x, gl = gl0 + blockIdx.y, seg = seg0 + blockIdx.z;
    {
        const unsigned sx = seg % (unsigned)a.b.segs_x, sy = seg / (unsigned)a.b.segs_x % (unsigned)a.b.segs_y;
        const unsigned fr = seg / (unsigned)a.b.segs_x / (unsigned)a.b.segs_y;
        const int h0 = sy * CB_R, v0 = sx * CB_C, n0 = pass * NB, nt = min(NB, tiles - n0);
        const int cols = min(CB_C, Ws - v0), steps = (cols + 3) / 4, whole = cols / 4;
        // x and g from the item's frame and its first channel on: the large tensor's group, the small tensor's pass
        const unsigned fs = fr * Hs * Ws, fl = fr * HL * WL;
        const float *xi = a.b.x + (size_t)(TR ? fs : fl) * Cin + (TR ? n0 : gl) * 16;
        ConvBwArgs b = a.b;
        b.dy += (size_t)(TR ? fl : fs) * b.dy_channels + (TR ? gl : n0) * 16;
        if (b.act == DTFILL_CONV_LEAKY) b.y += (size_t)(TR ? fl : fs) * b.y_channels + (TR ? gl : n0) * 16;
        auto load_x = [&](unsigned pixel, int c) {
            const float *src = xi + (size_t)pixel * Cin + c;
            return VEC ? *reinterpret_cast<const cv_f4 *>(src) : cv_f4{src[0], src[1], src[2], src[3]};
        };
        cv_f4 acc[NT][NB], accb[NDB];
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int k = 0; k < NB; ++k) acc[n][k] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < NDB; ++k) accb[k] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int h1 = h0; h1 < min(h0 + CB_R, Hs); h1 += RS) {
            // ---- the strip of the large tensor's group under every tap, +0 outside its frame ----
            for (int e = t; e < LH * LWS * 4; e += 256) {
                const int p = e >> 2, s = e & 3;
                const int r = p / LWS, lc = p - r * LWS;
                const int h = S * h1 - G::P + r, v = S * v0 - G::P + lc;
                cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
                if (h >= 0 && h < HL && v >= 0 && v < WL) {
                    const unsigned pixel = (unsigned)h * WL + v;
                    f = TR ? convb_g4(b, pixel, 4 * s, VEC) : load_x(pixel, 4 * s);
                }
                *reinterpret_cast<cv_f4 *>(s_l + ((r * S + lc % S) * LWH + lc / S) * 16 + 4 * s) = f;
            }
            // ---- the strip of the small tensor's nt tiles, [tile][pixel][16], +0 outside its frame ----
            for (int e = t; e < nt * RS * CB_C * 4; e += 256) {
                const int p = e >> 2, s = e & 3;  // p: (tile, row, column)
                const int n = p / (RS * CB_C), row = p / CB_C % RS, col = p % CB_C;
                const int h = h1 + row, v = v0 + col;
                cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
                if (h < Hs && v < Ws) {
                    const unsigned pixel = (unsigned)h * Ws + v;
                    f = TR ? load_x(pixel, n * 16 + 4 * s) : convb_g4(b, pixel, n * 16 + 4 * s, VEC);
                }
                *reinterpret_cast<cv_f4 *>(s_s + p * 16 + 4 * s) = f;
            }
            __syncthreads();
            // ---- the strip's links of every chain, in raster order (EDGE: as in k_convb_dw) ----
            const int rows = min(RS, Hs - h1);
            auto k_step = [&](auto edge, int row, int s) {
                const bool real = !decltype(edge)::value || v0 + 4 * s + kq < Ws;
                const int at = (row * S * S * LWH + 4 * s) * 16;
                float sv[NB];
#pragma unroll
                for (int k = 0; k < NB; ++k) sv[k] = s_s[((k * RS + row) * CB_C + 4 * s + kq) * 16 + m];
#pragma unroll
                for (int n = 0; n < NT; ++n)
                    if (wave + 4 * n < TAPS) {
                        const float lv = real ? s_l[at + aoff[n]] : 0.0f;
#pragma unroll
                        for (int k = 0; k < NB; ++k)
                            acc[n][k] = __builtin_amdgcn_mfma_f32_16x16x4f32(TR ? sv[k] : lv, TR ? lv : sv[k], acc[n][k], 0, 0, 0);
                    }
                if (wave == 3) {
                    const float one = real ? 1.0f : 0.0f;
#pragma unroll
                    for (int k = 0; k < NDB; ++k) {
                        if (TR)
                            accb[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(one, real ? s_l[at + boff[k]] : 0.0f, accb[k], 0, 0, 0);
                        else
                            accb[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(one, sv[k], accb[k], 0, 0, 0);
                    }
                }
            };
#pragma unroll 1
            for (int row = 0; row < rows; ++row) {
#pragma unroll 1
                for (int s = 0; s < whole; ++s) k_step(std::false_type{}, row, s);
                if (whole < steps) k_step(std::true_type{}, row, whole);
            }
            __syncthreads();  // the strips are rewritten by the next one
        }
        // ---- the segment's partials: [tap][Cin][Cout], then db ----
        float *ps = part + (size_t)seg * (((size_t)TAPS * Cin + 1) * Cout);
#pragma unroll
        for (int n = 0; n < NT; ++n)
            if (wave + 4 * n < TAPS) {
#pragma unroll
                for (int k = 0; k < NB; ++k)
                    if (k < nt) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int c = (TR ? n0 + k : gl) * 16 + 4 * kq + e, o = (TR ? gl : n0 + k) * 16 + m;
                            ps[((size_t)(wave + 4 * n) * Cin + c) * Cout + o] = acc[n][k][e];
                        }
                    }
            }
        if (wave == 3 && (TR ? pass == 0 : gl == 0) && kq == 0) {
#pragma clang fp contract(off)
            if (TR) {
                ps[(size_t)TAPS * Cin * Cout + gl * 16 + m] = ((accb[0][0] + accb[1][0]) + accb[2][0]) + accb[3][0];
            } else {
#pragma unroll
                for (int k = 0; k < NB; ++k)
                    if (k < nt) ps[(size_t)TAPS * Cin * Cout + (n0 + k) * 16 + m] = accb[k][0];
            }
        }
    }
}

template <int KS, int S, bool TR>
void convb_dw_wide_launch(hipStream_t st, const ConvBwWide &a, float *part, long long nseg) {
    const int groups = (TR ? a.b.Cout : a.b.Cin) / 16, tiles = (TR ? a.b.Cin : a.b.Cout) / 16;
    const int npass = (tiles + ConvBwGeo<KS, S>::NB - 1) / ConvBwGeo<KS, S>::NB;  // (< 2^24: a multiple of 16 below 2^31)
    const bool vec = a.b.xvec && a.b.gvec;  // x, dy and y all allow 16-byte loads
    for (long long seg0 = 0; seg0 < nseg; seg0 += 65535)
        for (int gl0 = 0; gl0 < groups; gl0 += 65535) {
            const dim3 grid((unsigned)npass, (unsigned)min(groups - gl0, 65535), (unsigned)min(nseg - seg0, 65535ll));
            (vec ? k_convb_dw_wide<KS, S, TR, true> : k_convb_dw_wide<KS, S, TR, false>)<<<grid, 256, 0, st>>>(a, part, (unsigned)seg0,
                                                                                                              (unsigned)gl0);
        }
}

// ------------------------------------------------------------------------------------------------
// The image layer: dw and db of dtfill_conv2d_image (CIN of 2, 3 or 4 into a multiple of 16 channels).  There is no dx: the
// image is data.  k_convb_dw_image is k_convb_dw's Cin == 1 form grown two ways.  The 16 rows of a tile are (tap, channel)
// pairs in dw's own order, row = tap CIN + c; there are KS KS CIN of them in CBI_NT(..) tiles, and the first free row, which
// always exists (KS KS is odd and CIN <= 4: the count is no multiple of 16), is the row of ones that makes db.  And there is
// an N loop: a work item is (segment, pass of CBI_NB tiles of 16 output channels), the pass fastest; the staged strip of x
// serves the pass's tiles, wave k holding tile k of the pass with one accumulator per row tile (13 at 7x7x4, 2 for the RGB
// stem: independent chains).  The strips are CBI_RS rows, g as [tile][pixel][16] and x plain, [row][column][CIN], read one
// float a lane at a constant offset a row tile.  Edge k-steps as in k_convb_dw.
// ------------------------------------------------------------------------------------------------
constexpr int CBI_NB = 4;  // N-tiles of a pass: one a wave
constexpr int CBI_RS = 2;  // rows of a strip
static_assert(CB_R % CBI_RS == 0, "a segment is whole strips");

template <int KS, int CIN>
__global__ __launch_bounds__(256, 2) void k_convb_dw_image(ConvBwArgs a, float *__restrict__ part, int npass, long long n_items) {
    constexpr int R = (KS - 1) / 2, ROWS = KS * KS * CIN, NT = (ROWS + 16) / 16, NB = CBI_NB, RS = CBI_RS;
    constexpr int LH = RS + KS - 1, LW = CB_C + KS - 1;
    static_assert(CIN >= 2 && CIN <= 4 && ROWS % 16 != 0, "the last tile has a free row for db");
    __shared__ __attribute__((aligned(16))) float s_x[LH * LW * CIN];
    __shared__ __attribute__((aligned(16))) float s_g[NB * RS * CB_C * 16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;  // A: row m, pixel kq; B: pixel kq, output channel m; D: channel m, rows 4 kq ..+3
    const int H = a.H, W = a.W, Cout = a.Cout;
    const size_t pstride = (size_t)(ROWS + 1) * Cout;
    // the lane's float offset into s_x of row tile n's operand, at the strip's first pixel (rows ROWS and beyond read nothing)
    int aoff[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int row = min(16 * n + m, ROWS - 1), tap = row / CIN;
        aoff[n] = ((tap / KS) * LW + tap % KS + kq) * CIN + row - tap * CIN;
    }
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int pass = (int)(item % npass);
        const long long seg = item / npass;
        const int sx = (int)(seg % a.segs_x), sy = (int)(seg / a.segs_x % a.segs_y), b = (int)(seg / a.segs_x / a.segs_y);
        const int h0 = sy * CB_R, v0 = sx * CB_C, n0 = pass * NB, nt = min(NB, Cout / 16 - n0);
        const size_t fb = (size_t)b * H * W;
        const float *xb = a.x + fb * CIN;
        ConvBwArgs g = a;  // dy and y from the item's frame and the pass's first channel on
        g.dy += fb * g.dy_channels + n0 * 16;
        if (g.act == DTFILL_CONV_LEAKY) g.y += fb * g.y_channels + n0 * 16;
        const int cols = min(CB_C, W - v0), steps = (cols + 3) / 4, whole = cols / 4;  // k-steps of a row; those wholly inside
        cv_f4 acc[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[n] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int h1 = h0; h1 < min(h0 + CB_R, H); h1 += RS) {
            // ---- the haloed strip of x, +0 outside the frame (a row of it is LW CIN consecutive floats of x) ----
            for (int e = t; e < LH * LW * CIN; e += 256) {
                const int r = e / (LW * CIN), rest = e - r * (LW * CIN);
                const int h = h1 + r - R, v = v0 + rest / CIN - R;
                s_x[e] = h >= 0 && h < H && v >= 0 && v < W ? xb[((size_t)h * W + (v0 - R)) * CIN + rest] : 0.0f;
            }
            // ---- the strip of g of the pass's nt tiles, [tile][pixel][16], +0 outside the frame ----
            for (int e = t; e < nt * RS * CB_C * 4; e += 256) {
                const int p = e >> 2, s = e & 3;  // p: (tile, row, column)
                const int n = p / (RS * CB_C), row = p / CB_C % RS, col = p % CB_C;
                const int h = h1 + row, v = v0 + col;
                cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
                if (h < H && v < W) f = convb_g4(g, (size_t)h * W + v, n * 16 + 4 * s, a.gvec);
                *reinterpret_cast<cv_f4 *>(s_g + p * 16 + 4 * s) = f;
            }
            __syncthreads();
            // ---- the strip's links of every chain, in raster order (EDGE: as in k_convb_dw) ----
            const int rows = min(RS, H - h1);
            auto k_step = [&](auto edge, int row, int s) {
                const bool real = !decltype(edge)::value || v0 + 4 * s + kq < W;
                const float gv = s_g[((wave * RS + row) * CB_C + 4 * s + kq) * 16 + m];
                const int at = (row * LW + 4 * s) * CIN;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int r = 16 * n + m;  // (only the last tile has rows beyond the chain's)
                    const float xv = n + 1 < NT || r < ROWS ? s_x[at + aoff[n]] : r == ROWS ? 1.0f : 0.0f;
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(real ? xv : 0.0f, gv, acc[n], 0, 0, 0);
                }
            };
            if (wave < nt) {
#pragma unroll 1
                for (int row = 0; row < rows; ++row) {
#pragma unroll 1
                    for (int s = 0; s < whole; ++s) k_step(std::false_type{}, row, s);
                    if (whole < steps) k_step(std::true_type{}, row, whole);
                }
            }
            __syncthreads();  // the strips are rewritten by the next one, or the next item
        }
        // ---- the segment's partials: [row][Cout] as dw is, then db ----
        if (wave < nt) {
            float *ps = part + (size_t)seg * pstride + (n0 + wave) * 16 + m;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 16 * n + 4 * kq + e;
                    if (r <= ROWS) ps[(size_t)r * Cout] = acc[n][e];
                }
        }
    }
}

template <int KS>
void convb_dw_image_launch(hipStream_t st, const ConvBwArgs &a, float *part, long long nseg) {
    const int npass = (a.Cout / 16 + CBI_NB - 1) / CBI_NB;  // (< 2^25: a multiple of 16 below 2^31)
    const long long n_items = nseg * npass;
    const int grid = (int)(n_items < CV_MAX_BLOCKS ? n_items : CV_MAX_BLOCKS);
    (a.Cin == 2 ? k_convb_dw_image<KS, 2> : a.Cin == 3 ? k_convb_dw_image<KS, 3> : k_convb_dw_image<KS, 4>)<<<grid, 256, 0, st>>>(a, part, npass,
                                                                                                                              n_items);
}

// ---- the host side: one layer record, one plan (dtfill.hip's convb_plan), one dispatch per gradient for all seven entry points ----
struct ConvBwLayer {  // a layer as its backward sees it: the forward's input [B,H,W,Cin] and what made its output
    int B, H, W, Cin, ksize, Cout, stride;
    bool transposed, narrow;  // narrow: dtfill_conv2d's domain (Cin 1/16/32/48/64, Cout 1/16, stride 1) and kernels; else the wide ones
    bool image = false;       // dtfill_conv2d_image's domain (Cin 2/3/4, Cout a multiple of 16, stride 1): weights only, its own kernel
    bool bf16 = false;        // a wide layer on the bf16 matrix cores (dtfill_convhb.hpp): ksize 1 or 3, the packed kernel in the workspace
};

struct ConvBwPlan {         // what convb_plan derives from a layer in its domain
    int Ho, Wo;             // dy's frame
    int Hs, Ws, HL, WL;     // the weight sum's SMALL frame, the one the segments lie over, and its LARGE one
    int segs_y, segs_x;     // segments of a small frame
    size_t wt, tmp, bytes;  // the bytes from g, at 0, to the repacked weights and to the 1x1 stride-2 chain's values; max(data, weights)
};

// dx.  b: dy's and y's view; the forward over g has the layer's Cout as its input channels and its Cin as its output channels
inline void convb_data_launch(hipStream_t st, const ConvBwLayer &l, const ConvBwPlan &p, const ConvBwArgs &b, const float *w, float *dx,
                              int dx_channels, int dx_offset, float *dres, void *workspace) {
    char *ws = static_cast<char *>(workspace);
    float *g = reinterpret_cast<float *>(ws), *wt = reinterpret_cast<float *>(ws + p.wt), *tmp = reinterpret_cast<float *>(ws + p.tmp);
    const long long total = (long long)l.B * p.Ho * p.Wo * l.Cout;
    const int taps = l.ksize * l.ksize, r = (l.ksize - 1) / 2;
    const bool blocked = l.Cout == 1 && l.Cin > 16;
    k_convb_g<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(b, g, dres, total);
    k_convb_flip<<<(taps * l.Cin * l.Cout + 255) / 256, 256, 0, st>>>(w, wt, taps, l.Cin, l.Cout, blocked, !l.transposed && l.stride == 1);
    ConvArgs a{g, wt, nullptr, nullptr, dx, l.B, p.Ho, p.Wo, l.Cout, l.Cin, l.H, l.W, 0, 0, dx_channels, dx_offset, DTFILL_CONV_LINEAR,
               0.0f};
    if (l.transposed) {
        conv_strided_launch(st, a, 3, 2);  // [2H,2W] -> [H,W], pt = pl = 0
    } else if (l.stride == 2 && l.ksize == 3) {
        conv_transpose_launch(st, a);  // [H/2,W/2] -> [H,W]
    } else if (l.stride == 2) {
        a.out = tmp, a.Ho = p.Ho, a.Wo = p.Wo, a.out_channels = l.Cin, a.out_offset = 0;
        conv_strided_launch(st, a, 1, 1);
        const long long n = (long long)l.B * l.H * l.W * l.Cin;
        k_convb_spread<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, dx, l.H, l.W, l.Cin, dx_channels, dx_offset, n);
    } else {
        a.pt = a.pl = r;
        if (blocked) {
            a.Cout = 16;
            for (int n = 0; n < l.Cin / 16; ++n) {
                a.w = wt + (size_t)n * taps * 16;
                a.out_offset = dx_offset + 16 * n;
                conv_launch(st, a, l.ksize);
            }
        } else if (l.narrow && l.Cin <= 16) {
            conv_launch(st, a, l.ksize);
        } else {
            conv_strided_launch(st, a, l.ksize, 1);
        }
    }
}

// dw and db: level 1 into the segments' partials (the workspace), then level 2
inline void convb_weights_launch(hipStream_t st, const ConvBwLayer &l, const ConvBwWide &a, float *dw, float *db, void *workspace) {
    float *part = static_cast<float *>(workspace);
    const int nseg = l.B * a.b.segs_y * a.b.segs_x;                      // (< 2^31: the small frames' pixels are)
    const int ndw = l.ksize * l.ksize * l.Cin * l.Cout, pstride = ndw + l.Cout;  // (< 2^31: the entry points' domain)
    if (l.image) {
        switch (l.ksize) {
            case 1: convb_dw_image_launch<1>(st, a.b, part, nseg); break;
            case 3: convb_dw_image_launch<3>(st, a.b, part, nseg); break;
            case 5: convb_dw_image_launch<5>(st, a.b, part, nseg); break;
            default: convb_dw_image_launch<7>(st, a.b, part, nseg); break;
        }
    } else if (l.Cout == 1) {
        k_convb_dw_lane<<<dim3((unsigned)nseg, (unsigned)((pstride + 255) / 256)), 256, 0, st>>>(a.b, l.ksize, part);
    } else if (l.narrow) {
        switch (l.ksize) {
            case 1: convb_dw_launch<1>(st, a.b, part, nseg); break;
            case 3: convb_dw_launch<3>(st, a.b, part, nseg); break;
            case 5: convb_dw_launch<5>(st, a.b, part, nseg); break;
            default: convb_dw_launch<7>(st, a.b, part, nseg); break;
        }
    } else if (l.transposed) {
        convb_dw_wide_launch<3, 2, true>(st, a, part, nseg);
    } else if (l.stride == 2) {
        (l.ksize == 1 ? convb_dw_wide_launch<1, 2, false> : convb_dw_wide_launch<3, 2, false>)(st, a, part, nseg);
    } else {
        switch (l.ksize) {
            case 1: convb_dw_wide_launch<1, 1, false>(st, a, part, nseg); break;
            case 3: convb_dw_wide_launch<3, 1, false>(st, a, part, nseg); break;
            case 5: convb_dw_wide_launch<5, 1, false>(st, a, part, nseg); break;
            default: convb_dw_wide_launch<7, 1, false>(st, a, part, nseg); break;
        }
    }
    k_convb_sum<<<(pstride + 255) / 256, 256, 0, st>>>(part, pstride, nseg, ndw, dw, db);
}
