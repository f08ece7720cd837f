// dtfill_convb.hpp -- the backward pass of dtfill_conv2d in a fixed summation order: dx, dw and db of the layers of
// SparsityCNN (solution_DeepNet/net.py:11-242), what train.py:232-254's tape needs of a convolution.  include/dtfill.h,
// dtfill_conv2d_backward_data() and dtfill_conv2d_backward_weights(), has the contracts.  Part of libdtfill.so; included by
// dtfill.hip inside its anonymous namespace, after dtfill_conv.hpp, whose kernels the input gradient runs on.
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

// g[n, o] of all n = B H W pixels, dense
__global__ __launch_bounds__(256) void k_convb_g(ConvBwArgs a, float *__restrict__ g, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long pixel = idx / a.Cout;
    const int o = (int)(idx - pixel * a.Cout);
    const float dy = a.dy[pixel * a.dy_channels + o];
    g[idx] = convb_g(dy, a.y ? a.y[pixel * a.y_channels + o] : 0.0f, a.act, a.alpha);
}

// wT[i, j, o, c] = w[ksize - 1 - i, ksize - 1 - j, c, o]; `blocked` (Cout == 1, Cin >= 32): [c / 16][tap][c % 16]
__global__ __launch_bounds__(256) void k_convb_flip(const float *__restrict__ w, float *__restrict__ wt, int taps, int Cin, int Cout,
                                                    bool blocked) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= taps * Cin * Cout) return;
    const int o = idx % Cout, c = idx / Cout % Cin, tap = idx / Cout / Cin;
    const int ft = taps - 1 - tap;  // (ksize - 1 - i) ksize + (ksize - 1 - j)
    wt[blocked ? ((c / 16) * taps + ft) * 16 + c % 16 : (ft * Cout + o) * Cin + c] = w[idx];
}

// dtfill_conv2d_backward_data: the workspace is g, then wT
inline void convb_data_launch(hipStream_t st, const ConvBwArgs &b, const float *w, int ksize, float *dx, int dx_channels, int dx_offset,
                              float *g, float *wt) {
    const long long total = (long long)b.B * b.H * b.W * b.Cout;
    const int taps = ksize * ksize, r = (ksize - 1) / 2;
    const bool blocked = b.Cout == 1 && b.Cin > 16;
    k_convb_g<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(b, g, total);
    k_convb_flip<<<(taps * b.Cin * b.Cout + 255) / 256, 256, 0, st>>>(w, wt, taps, b.Cin, b.Cout, blocked);
    ConvArgs a{g, wt, nullptr, nullptr, dx, b.B, b.H, b.W, b.Cout, b.Cin, b.H, b.W, r, r, dx_channels, dx_offset, DTFILL_CONV_LINEAR, 0.0f};
    if (blocked) {
        a.Cout = 16;
        for (int n = 0; n < b.Cin / 16; ++n) {
            a.w = wt + (size_t)n * taps * 16;
            a.out_offset = dx_offset + 16 * n;
            conv_launch(st, a, ksize);
        }
    } else if (b.Cin > 16) {
        conv_strided_launch(st, a, ksize, 1);
    } else {
        conv_launch(st, a, ksize);
    }
}

// what a strip of g is: rows h1 .. h1 + CB_RS - 1, columns v0 .. v0 + CB_C - 1 of frame fb, +0 outside the frame, [pixel][16]
__device__ __forceinline__ void convb_stage_g(float *s_g, const ConvBwArgs &a, size_t fb, int h1, int v0, int t) {
    for (int e = t; e < CB_RS * CB_C * 4; e += 256) {
        const int p = e >> 2, s = e & 3;  // channels 4 s .. 4 s + 3 of pixel p of the strip
        const int row = p / CB_C, col = p - row * CB_C;
        const int h = h1 + row, v = v0 + col;
        cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
        if (h < a.H && v < a.W) {
            const size_t pixel = fb + (size_t)h * a.W + v;
            const float *pd = a.dy + pixel * a.dy_channels + 4 * s;
            f = a.gvec ? *reinterpret_cast<const cv_f4 *>(pd) : cv_f4{pd[0], pd[1], pd[2], pd[3]};
            if (a.act == DTFILL_CONV_LEAKY) {
                const float *py = a.y + pixel * a.y_channels + 4 * s;
                const cv_f4 y = a.gvec ? *reinterpret_cast<const cv_f4 *>(py) : cv_f4{py[0], py[1], py[2], py[3]};
                f = cv_f4{convb_g(f.x, y.x, a.act, a.alpha), convb_g(f.y, y.y, a.act, a.alpha), convb_g(f.z, y.z, a.act, a.alpha),
                          convb_g(f.w, y.w, a.act, a.alpha)};
            }
        }
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

// dtfill_conv2d_backward_weights: the workspace is the partials
inline void convb_weights_launch(hipStream_t st, const ConvBwArgs &a, int ksize, float *dw, float *db, float *part) {
    const int nseg = a.B * a.segs_y * a.segs_x;  // (< 2^31: B H W is)
    const int ndw = ksize * ksize * a.Cin * a.Cout, pstride = ndw + a.Cout;
    if (a.Cout == 1) {
        k_convb_dw_lane<<<dim3((unsigned)nseg, (unsigned)((pstride + 255) / 256)), 256, 0, st>>>(a, ksize, part);
    } else {
        switch (ksize) {
            case 1: convb_dw_launch<1>(st, a, part, nseg); break;
            case 3: convb_dw_launch<3>(st, a, part, nseg); break;
            case 5: convb_dw_launch<5>(st, a, part, nseg); break;
            default: convb_dw_launch<7>(st, a, part, nseg); break;
        }
    }
    k_convb_sum<<<(pstride + 255) / 256, 256, 0, st>>>(part, pstride, nseg, ndw, dw, db);
}
