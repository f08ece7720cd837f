// dtfill_conv2.hpp -- the wide layers of ResNet18_NO_BN_l2 (solution_DeepNet/net.py:245-745) in dtfill_conv.hpp's fixed
// summation order: stride 1 and 2 with TensorFlow's 'same' rule, many output-channel tiles, a fused residual add, and the 3x3
// stride-2 transposed convolution.  include/dtfill.h, dtfill_conv2d_strided() and dtfill_conv2d_transpose(), has the
// contracts.  Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace, after dtfill_conv.hpp.
#pragma once

// ------------------------------------------------------------------------------------------------
// Both kernels are k_conv_mfma's implicit GEMM with an N loop: the haloed 16-channel tile staged in LDS for a group serves
// C2_NB output-channel tiles of 16 in one pass, so the 16-byte LDS read that feeds one M-tile's four k-steps feeds 4 C2_NB
// MFMAs, not 4.  A work item is (pixel tile, pass of 16 C2_NB output channels), the pass fastest, so that the blocks that
// share an input tile run together; a layer with Cout > 64 stages its input Cout / 64 times, not Cout / 16.
//   k_conv2_mfma       stride S.  S == 1: the block tile is 8 x 32 output pixels and a wave holds two rows as four M-tiles;
//                      S == 2: 4 x 32 and a wave holds one row as two M-tiles, so that the input tile (9 x 65 pixels for
//                      3x3) stays at 38 KB.  At stride 2 a lane's pixels are two input columns apart, so the tile is staged
//                      de-interleaved by column parity, [row][parity][column / 2]: tap j reads plane j & 1 at column
//                      m + (j >> 1), unit stride again.
//   k_conv2_transpose  four stride-1 correlations of the input grid, one per output parity, with 1, 2, 2 and 4 taps; the
//                      parity is part of the work item.  The tile is 8 x 32 INPUT pixels with one halo row above and one
//                      halo column to the left; a lane's stores go to output pixels two apart.
// The 16 channels of a pixel lie as k_conv_mfma has them, a 4 x 4 transpose whose quarters are exchanged so that no two lanes
// of a ds_read_b128 lane group meet on a bank; here the exchange goes by the pixel's linear index P in the LDS image, not by
// its column: the 16 lanes of a group are four sets {m, m + 4, m + 8, m + 12} with k quarters {k, k', k', k} (k' = k ^ 1), a
// set shares P mod 4 and so its four banks, and bit 2 of P alternates along it, which makes its quarters k ^ 2 b, k' ^ 2 ~b,
// k' ^ 2 b, k ^ 2 ~b: all four, for every base, row pitch and tap offset.
// The weight fragment of tap T, k-step s, N-tile n is w[T][16 g + 4 s + (lane >> 4)][n0 + 16 n + (lane & 15)]: 16 lanes read
// 64 consecutive bytes.  A tap's 4 C2_NB fragments are asked for one tap ahead of their use (64 MFMAs, 2048 cycles).
// Registers: 16 C2_NB accumulators, 8 C2_NB weights, 16 operands: two blocks a CU.
// ------------------------------------------------------------------------------------------------
constexpr int C2_NB = 4;  // N-tiles (16 output channels each) of a pass

struct Conv2Args {
    const float *x, *w, *bias, *res;
    float *out;
    int B, H, W, Cin, Cout, Ho, Wo, pt, pl, out_channels, out_offset, act;
    float alpha;
};

// float index of k quarter k of the pixel at linear index P of the LDS image
__device__ __forceinline__ int conv2_slot(int P, int k) { return P * CV_G + 4 * (k ^ ((P >> 1) & 2)); }

// the bias, the residual and the activation: two rounded adds, then y > 0 ? y : y * alpha
__device__ __forceinline__ float conv2_finish(float acc, const Conv2Args &a, int o, size_t pixel) {
#pragma clang fp contract(off)
    float y = acc;
    if (a.bias) y = y + a.bias[o];
    if (a.res) y = y + a.res[pixel * a.Cout + o];
    if (a.act == DTFILL_CONV_LEAKY) y = y > 0.0f ? y : y * a.alpha;
    return y;
}

// Stages input pixels (ih0 + r, iv0 + lc), r < LH, lc < LWS, channels 16 g .. 16 g + 15, +0 outside the frame, into the LDS
// image [LH][S planes][LWH]: column lc in plane lc % S at lc / S.
template <int S, int LH, int LWS, int LWH, bool VEC>
__device__ __forceinline__ void conv2_stage(float *s_x, const float *__restrict__ xb, int H, int W, int Cin, int g, int ih0, int iv0,
                                            int t) {
    for (int e = t; e < LH * LWS * 4; e += 256) {
        const int p = e >> 2, s = e & 3;  // channels 4 s .. 4 s + 3 of staged pixel p
        const int r = p / LWS, lc = p - r * LWS;
        const int h = ih0 + r, v = iv0 + lc;
        cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
        if (h >= 0 && h < H && v >= 0 && v < W) {
            const float *src = xb + ((size_t)h * W + v) * Cin + g * CV_G + 4 * s;
            if (VEC)
                f = *reinterpret_cast<const cv_f4 *>(src);
            else
                f = cv_f4{src[0], src[1], src[2], src[3]};
        }
        const int P = (r * S + lc % S) * LWH + lc / S;
        s_x[conv2_slot(P, 0) + s] = f.x;  // channel 4 s + k at position s of k's quarter
        s_x[conv2_slot(P, 1) + s] = f.y;
        s_x[conv2_slot(P, 2) + s] = f.z;
        s_x[conv2_slot(P, 3) + s] = f.w;
    }
}

// the weight fragments of one tap: d[4 s + n] = wt[(4 s) Cout + 16 n], wt = w + ((tap Cin + 16 g + kq) Cout + n0 + m)
__device__ __forceinline__ void conv2_weights(const float *__restrict__ wt, int Cout, int nt, float (&d)[4 * C2_NB]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int n = 0; n < C2_NB; ++n) d[4 * s + n] = n < nt ? wt[(size_t)4 * s * Cout + 16 * n] : 0.0f;
}

// one tap's links of the chain: the MT M-tiles' operands at LDS pixels P[q] + dP, four k-steps, nt N-tiles
template <int MT>
__device__ __forceinline__ void conv2_tap(const float *s_x, const int (&P)[MT], int dP, int kq, const float (&wr)[4 * C2_NB], int nt,
                                          cv_f4 (&acc)[MT][C2_NB]) {
    cv_f4 xv[MT];
#pragma unroll
    for (int q = 0; q < MT; ++q) xv[q] = *reinterpret_cast<const cv_f4 *>(s_x + conv2_slot(P[q] + dP, kq));
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int n = 0; n < C2_NB; ++n)
            if (n < nt) {
#pragma unroll
                for (int q = 0; q < MT; ++q) acc[q][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q][s], wr[4 * s + n], acc[q][n], 0, 0, 0);
            }
}

// Work item `item` of n_items = tiles x passes, in (frame, tile row, tile column, pass) order; a block takes the items
// blockIdx.x, blockIdx.x + gridDim.x, ...
template <int KS, int S, bool VEC>
__global__ __launch_bounds__(256, 2) void k_conv2_mfma(Conv2Args a, int tiles_x, int tiles_y, int npass, long long n_items) {
    constexpr int RW = S == 1 ? 2 : 1, TH = 4 * RW, MT = 2 * RW;  // rows of the tile a wave holds, the tile's rows, M-tiles a wave
    constexpr int UJ = KS <= 3 ? KS : 1;  // a row of taps is unrolled only where its weights fit the registers
    constexpr int LH = (TH - 1) * S + KS, LWS = (CV_TW - 1) * S + KS, LWH = CV_TW + (KS - 1 + S - 1) / S;
    __shared__ __attribute__((aligned(16))) float s_x[LH * S * LWH * CV_G];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
    const int groups = Cin / CV_G;
    int P[MT];  // the lane's pixel of M-tile q (row RW wave + (q >> 1), half q & 1) under tap (0, 0)
#pragma unroll
    for (int q = 0; q < MT; ++q) P[q] = (RW * wave + (q >> 1)) * S * S * LWH + CV_M * (q & 1) + m;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int pass = (int)(item % npass);
        const long long tile = item / npass;
        const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x % tiles_y), b = (int)(tile / tiles_x / tiles_y);
        const int h0 = ty * TH, v0 = tx * CV_TW, n0 = pass * 16 * C2_NB;
        const int nt = min(C2_NB, (Cout - n0) / 16);
        const float *xb = a.x + (size_t)b * H * W * Cin;
        cv_f4 acc[MT][C2_NB];
#pragma unroll
        for (int q = 0; q < MT; ++q)
#pragma unroll
            for (int n = 0; n < C2_NB; ++n) acc[q][n] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
            const float *wl = a.w + ((size_t)g * CV_G + kq) * Cout + n0 + m;
            const size_t wtap = (size_t)Cin * Cout;
            float wr[4 * C2_NB];  // the group's first tap is asked for before its tile is staged
            conv2_weights(wl, Cout, nt, wr);
            conv2_stage<S, LH, LWS, LWH, VEC>(s_x, xb, H, W, Cin, g, S * h0 - a.pt, S * v0 - a.pl, t);
            __syncthreads();
#pragma unroll 1
            for (int i = 0; i < KS; ++i) {
#pragma unroll UJ
                for (int j = 0; j < KS; ++j) {
                    float wn[4 * C2_NB];  // the next tap, asked for before this tap's MFMAs
                    const bool more = j + 1 < KS || i + 1 < KS;
                    if (more) conv2_weights(wl + (size_t)(i * KS + j + 1) * wtap, Cout, nt, wn);
                    conv2_tap<MT>(s_x, P, (i * S + j % S) * LWH + j / S, kq, wr, nt, acc);
                    if (more) {
#pragma unroll
                        for (int k = 0; k < 4 * C2_NB; ++k) wr[k] = wn[k];
                    }
                }
            }
            __syncthreads();  // the tile is rewritten by the next group, or the next item
        }
        // ---- bias, residual, activation, store: lane (channel m of each N-tile, pixels 4 kq .. 4 kq + 3 of the M-tile) ----
#pragma unroll
        for (int q = 0; q < MT; ++q) {
            const int h = h0 + RW * wave + (q >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = v0 + CV_M * (q & 1) + 4 * kq + e;
                if (h < a.Ho && v < a.Wo) {
                    const size_t pixel = ((size_t)b * a.Ho + h) * a.Wo + v;
#pragma unroll
                    for (int n = 0; n < C2_NB; ++n)
                        if (n < nt) {
                            const int o = n0 + 16 * n + m;
                            a.out[pixel * a.out_channels + a.out_offset + o] = conv2_finish(acc[q][n][e], a, o, pixel);
                        }
                }
            }
        }
    }
}

// Work item = (frame, tile row, tile column, output parity, pass); the tile is CV_TH x CV_TW input pixels, its outputs the
// pixels (2 h + py, 2 v + px).  a.H, a.W: the input frame; a.Ho = 2 H, a.Wo = 2 W.
template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_conv2_transpose(Conv2Args a, int tiles_x, int tiles_y, int npass, long long n_items) {
    constexpr int MT = 4, LH = CV_TH + 1, LWH = CV_TW + 1;
    __shared__ __attribute__((aligned(16))) float s_x[LH * LWH * CV_G];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
    const int groups = Cin / CV_G;
    int P[MT];  // the lane's input pixel of M-tile q in the haloed image
#pragma unroll
    for (int q = 0; q < MT; ++q) P[q] = (2 * wave + (q >> 1) + 1) * LWH + CV_M * (q & 1) + m + 1;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int pass = (int)(item % npass), par = (int)(item / npass & 3);
        const long long tile = item / npass / 4;
        const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x % tiles_y), b = (int)(tile / tiles_x / tiles_y);
        const int h0 = ty * CV_TH, v0 = tx * CV_TW, n0 = pass * 16 * C2_NB;
        const int nt = min(C2_NB, (Cout - n0) / 16);
        const int py = par >> 1, px = par & 1;
        // the taps of this parity in raster order: ky = 1 for an odd row, 0 then 2 for an even one; tap 2 reads the pixel before
        const int nkx = 2 - px, ntap = (2 - py) * nkx;
        const float *xb = a.x + (size_t)b * H * W * Cin;
        cv_f4 acc[MT][C2_NB];
#pragma unroll
        for (int q = 0; q < MT; ++q)
#pragma unroll
            for (int n = 0; n < C2_NB; ++n) acc[q][n] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
            const float *wl = a.w + ((size_t)g * CV_G + kq) * Cout + n0 + m;
            const size_t wtap = (size_t)Cin * Cout;
            float wr[4 * C2_NB];
            conv2_weights(wl + (size_t)(3 * py + px) * wtap, Cout, nt, wr);  // the first tap is (py, px)
            conv2_stage<1, LH, LWH, LWH, VEC>(s_x, xb, H, W, Cin, g, h0 - 1, v0 - 1, t);
            __syncthreads();
#pragma unroll 1
            for (int k = 0; k < ntap; ++k) {
                const int ay = k / nkx, ax = k - ay * nkx;  // tap (py + 2 ay, px + 2 ax): ay, ax pixels back
                float wn[4 * C2_NB];
                const bool more = k + 1 < ntap;
                if (more) {
                    const int by = (k + 1) / nkx, bx = k + 1 - by * nkx;
                    conv2_weights(wl + (size_t)(3 * (py + 2 * by) + px + 2 * bx) * wtap, Cout, nt, wn);
                }
                conv2_tap<MT>(s_x, P, -(ay * LWH + ax), kq, wr, nt, acc);
                if (more) {
#pragma unroll
                    for (int i = 0; i < 4 * C2_NB; ++i) wr[i] = wn[i];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < MT; ++q) {
            const int h = h0 + 2 * wave + (q >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = v0 + CV_M * (q & 1) + 4 * kq + e;
                if (h < H && v < W) {
                    const size_t pixel = ((size_t)b * a.Ho + 2 * h + py) * a.Wo + 2 * v + px;
#pragma unroll
                    for (int n = 0; n < C2_NB; ++n)
                        if (n < nt) {
                            const int o = n0 + 16 * n + m;
                            a.out[pixel * a.out_channels + a.out_offset + o] = conv2_finish(acc[q][n][e], a, o, pixel);
                        }
                }
            }
        }
    }
}

template <int KS, int S>
void conv2_mfma_launch(hipStream_t st, const Conv2Args &a) {
    constexpr int TH = S == 1 ? 8 : 4;
    const int tiles_x = (a.Wo + CV_TW - 1) / CV_TW, tiles_y = (a.Ho + TH - 1) / TH, npass = (a.Cout + 16 * C2_NB - 1) / (16 * C2_NB);
    const long long n_items = (long long)a.B * tiles_y * tiles_x * npass;
    const int grid = (int)(n_items < CV_MAX_BLOCKS ? n_items : CV_MAX_BLOCKS);
    if (((uintptr_t)a.x & 15) == 0)
        k_conv2_mfma<KS, S, true><<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, npass, n_items);
    else
        k_conv2_mfma<KS, S, false><<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, npass, n_items);
}

inline void conv2_launch(hipStream_t st, const Conv2Args &a, int ksize, int stride) {
    if (stride == 2) {
        if (ksize == 1)
            conv2_mfma_launch<1, 2>(st, a);
        else
            conv2_mfma_launch<3, 2>(st, a);
        return;
    }
    switch (ksize) {
        case 1: conv2_mfma_launch<1, 1>(st, a); break;
        case 3: conv2_mfma_launch<3, 1>(st, a); break;
        case 5: conv2_mfma_launch<5, 1>(st, a); break;
        default: conv2_mfma_launch<7, 1>(st, a); break;
    }
}

inline void conv2_transpose_launch(hipStream_t st, const Conv2Args &a) {
    const int tiles_x = (a.W + CV_TW - 1) / CV_TW, tiles_y = (a.H + CV_TH - 1) / CV_TH, npass = (a.Cout + 16 * C2_NB - 1) / (16 * C2_NB);
    const long long n_items = (long long)a.B * tiles_y * tiles_x * 4 * npass;
    const int grid = (int)(n_items < CV_MAX_BLOCKS ? n_items : CV_MAX_BLOCKS);
    if (((uintptr_t)a.x & 15) == 0)
        k_conv2_transpose<true><<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, npass, n_items);
    else
        k_conv2_transpose<false><<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, npass, n_items);
}
