// dtfill_conv.hpp -- stride-1 'same' float32 convolution in a fixed summation order, the layers of SparsityCNN
// (solution_DeepNet/net.py:11-242); include/dtfill.h, dtfill_conv2d(), has the contract.  Part of libdtfill.so; included by
// dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// The contract is one fmaf chain per output: groups of CV_G input channels outermost, then the taps in raster order, then
// the channels of the group.  v_mfma_f32_16x16x4_f32 adds its four k-products to C in k order with one rounding each, so a
// run of MFMAs whose k index walks the chain's order IS the chain, for 16 pixels x 16 output channels at once.
//   k_conv_mfma   Cout == 16.  Implicit GEMM: M = CV_M pixels of a row, N = the 16 output channels, K = the chain.
//                 A block takes a CV_TH x CV_TW pixel tile and, group by group, stages the haloed tile of the group's 16
//                 channels in LDS (34 KB for 7x7).  A wave holds two rows of the tile as four M-tiles: four independent
//                 accumulators that share one weight fragment per k-step (the 16x16x4 form has 40 cycles of dependent
//                 latency against a 32-cycle issue interval).
//                 Cin >= 16: a k-step is four consecutive channels of one tap, four k-steps a tap.  The 16 channels of a
//                 pixel lie in LDS as a 4 x 4 transpose, channel c at position c >> 2 of quarter c & 3, so that lane (pixel m, k
//                 quarter q) gets its operand of all four k-steps, channels q, 4 + q, 8 + q, 12 + q, by one 16-byte read; the
//                 quarters of a pixel are exchanged by its column (conv_quarter) so that no two lanes of a ds_read_b128 lane
//                 group meet on a bank.  The weight fragment of tap T, k-step s is w[T][16 g + 4 s + (lane >> 4)][lane & 15]
//                 = 64 consecutive floats from (T Cin + 16 g) 16 + 64 s: one coalesced dword load, straight from global
//                 memory (every wave of the device reads the same 50 KB a group), asked for a row of taps ahead of its use.
//                 Cin == 1: a k-step is four consecutive taps, the last step padded with zero operands on both sides (+0 *
//                 +0 added to the chain: only the sign of a zero can change); the weight fragment is again w[64 s + lane].
//   k_conv_chain  Cout == 1 (3x3x16 -> 1, 1x1x16 -> 1: under 0.3 % of the net's work): one lane per pixel, the chain literally, the
//                 channels of a tap by 16-byte loads where x allows.
// Padding taps are staged as +0.0f and multiplied like any other, in both kernels.
// ------------------------------------------------------------------------------------------------
constexpr int CV_TH = 8;   // the block tile: rows ...
constexpr int CV_TW = 32;  // ... and pixels of a row
constexpr int CV_M = 16;   // pixels of a row per MFMA tile
constexpr int CV_G = 16;   // input channels per group of the chain
static_assert(CV_TH == 2 * 4 && CV_TW == 2 * CV_M, "a wave holds two rows of the tile, two M-tiles each");

typedef float cv_f4 __attribute__((ext_vector_type(4)));

struct ConvArgs {
    const float *x, *w, *bias;
    float *out;
    int B, H, W, Cin, out_channels, out_offset, act;
    float alpha;
};

// the bias and the activation: one rounded add, then y > 0 ? y : y * alpha
__device__ __forceinline__ float conv_finish(float acc, const ConvArgs &a, int o) {
#pragma clang fp contract(off)
    float y = acc;
    if (a.bias) y = y + a.bias[o];
    if (a.act == DTFILL_CONV_LEAKY) y = y > 0.0f ? y : y * a.alpha;
    return y;
}

// Where the four channels q, 4 + q, 8 + q, 12 + q of the pixel in column c of the LDS image lie among the pixel's four 16-byte
// quarters.  ds_read_b128 serves a wave in four groups of 16 lanes that mix two k quarters ({0-3, 12-15, 20-27}, ...); with the
// quarters in place (q itself) two lanes of a group meet on every bank, with this exchange none do, for every tap offset.
__device__ __forceinline__ int conv_quarter(int q, int c) { return q ^ ((c >> 1) & 2); }

// the weight fragment of tap `tap`, its four k-steps: w[tap][16 g + 4 s + (lane >> 4)][lane & 15], wg = w + 256 g + lane
__device__ __forceinline__ void conv_weights(const float *__restrict__ wg, int tap, int Cin, float (&d)[4]) {
    const float *wt = wg + (size_t)tap * Cin * 16;
    d[0] = wt[0];
    d[1] = wt[64];
    d[2] = wt[128];
    d[3] = wt[192];
}

// Tiles of CV_TH x CV_TW pixels, tile `tile` of n_tiles in (frame, tile row, tile column) order; a block takes the tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...
template <int KS, bool CIN1, bool VEC>
__global__ __launch_bounds__(256) void k_conv_mfma(ConvArgs a, int tiles_x, int tiles_y, int n_tiles) {
    constexpr int R = (KS - 1) / 2, LH = CV_TH + KS - 1, LW = CV_TW + KS - 1, PC = CIN1 ? 1 : CV_G, TAPS = KS * KS;
    __shared__ __attribute__((aligned(16))) float s_x[LH * LW * PC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;  // A: pixel m, k index kq; B: k index kq, output channel m; D: channel m, pixels 4 kq ..+3
    const int H = a.H, W = a.W, Cin = a.Cin;
    const int groups = CIN1 ? 1 : Cin / CV_G;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)(tile / tiles_x % tiles_y), b = (int)(tile / tiles_x / tiles_y);
        const int h0 = ty * CV_TH, v0 = tx * CV_TW;
        const float *xb = a.x + (size_t)b * H * W * Cin;
        cv_f4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
            // the weight fragments of a row of taps, held in registers a row ahead: the group's first row is asked for before
            // its tile is staged, row i + 1 before row i's MFMAs
            const float *wg = a.w + (size_t)g * CV_G * 16 + lane;
            float wr[KS][4];
            if (!CIN1) {
#pragma unroll
                for (int j = 0; j < KS; ++j) conv_weights(wg, j, Cin, wr[j]);
            }
            // ---- the haloed tile of this group's channels, +0 outside the frame ----
            if (CIN1) {
                for (int p = t; p < LH * LW; p += 256) {
                    const int r = p / LW, c = p - r * LW;
                    const int h = h0 + r - R, v = v0 + c - R;
                    s_x[p] = h >= 0 && h < H && v >= 0 && v < W ? xb[(size_t)h * W + v] : 0.0f;
                }
            } else {
                for (int e = t; e < LH * LW * 4; e += 256) {
                    const int p = e >> 2, s = e & 3;  // channels 4 s .. 4 s + 3 of pixel p
                    const int r = p / LW, c = p - r * LW;
                    const int h = h0 + r - R, v = v0 + c - R;
                    cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
                    if (h >= 0 && h < H && v >= 0 && v < W) {
                        const float *src = xb + ((size_t)h * W + v) * Cin + g * CV_G + 4 * s;
                        if (VEC)
                            f = *reinterpret_cast<const cv_f4 *>(src);
                        else
                            f = cv_f4{src[0], src[1], src[2], src[3]};
                    }
                    float *d = s_x + p * CV_G + s;  // channel 4 s + k at position s of quarter conv_quarter(k, c)
                    d[4 * conv_quarter(0, c)] = f.x;
                    d[4 * conv_quarter(1, c)] = f.y;
                    d[4 * conv_quarter(2, c)] = f.z;
                    d[4 * conv_quarter(3, c)] = f.w;
                }
            }
            __syncthreads();
            // ---- the group's part of the chain ----
            const int row = 2 * wave;  // the wave's rows of the tile: row, row + 1; accumulator q: row + (q >> 1), half q & 1
            if (CIN1) {
                constexpr int STEPS = (TAPS + 3) / 4;
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const int tap = 4 * s + kq;
                    const bool real = tap < TAPS;
                    const int i = real ? tap / KS : 0, j = real ? tap - (tap / KS) * KS : 0;
                    const float wv = real ? a.w[tap * 16 + m] : 0.0f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float xv = s_x[(row + (q >> 1) + i) * LW + CV_M * (q & 1) + m + j];
                        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(real ? xv : 0.0f, wv, acc[q], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll 1
                for (int i = 0; i < KS; ++i) {
                    float wn[KS][4];  // the next row of taps, asked for before this row's MFMAs
                    if (i + 1 < KS) {
#pragma unroll
                        for (int j = 0; j < KS; ++j) conv_weights(wg, (i + 1) * KS + j, Cin, wn[j]);
                    }
#pragma unroll
                    for (int j = 0; j < KS; ++j) {
                        cv_f4 xv[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int c = CV_M * (q & 1) + m + j;
                            xv[q] = *reinterpret_cast<const cv_f4 *>(s_x + ((row + (q >> 1) + i) * LW + c) * CV_G + 4 * conv_quarter(kq, c));
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q].x, wr[j][0], acc[q], 0, 0, 0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q].y, wr[j][1], acc[q], 0, 0, 0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q].z, wr[j][2], acc[q], 0, 0, 0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q].w, wr[j][3], acc[q], 0, 0, 0);
                    }
                    if (i + 1 < KS) {
#pragma unroll
                        for (int j = 0; j < KS; ++j)
#pragma unroll
                            for (int k = 0; k < 4; ++k) wr[j][k] = wn[j][k];
                    }
                }
            }
            __syncthreads();  // the tile is rewritten by the next group, or the next tile
        }
        // ---- bias, activation, store: lane (channel m, pixels 4 kq .. 4 kq + 3 of the M-tile); 16 lanes store 64 contiguous bytes ----
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int h = h0 + 2 * wave + (q >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = v0 + CV_M * (q & 1) + 4 * kq + e;
                if (h < H && v < W)
                    a.out[(((size_t)b * H + h) * W + v) * a.out_channels + a.out_offset + m] = conv_finish(acc[q][e], a, m);
            }
        }
    }
}

// Cout == 1: pixel blockIdx.x * 256 + threadIdx.x of the n = B H W, the chain as the contract writes it.  VEC: Cin is a multiple of
// 4 and x is 16-byte aligned, the channels of a tap come by 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(256) void k_conv_chain(ConvArgs a, int ksize, int n) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int H = a.H, W = a.W, Cin = a.Cin, r = (ksize - 1) / 2;
    const int v = (int)(idx % W), h = (int)(idx / W % H), b = (int)(idx / W / H);
    const float *xb = a.x + (size_t)b * H * W * Cin;
    float acc = 0.0f;
    for (int c0 = 0; c0 < Cin; c0 += CV_G) {
        const int c1 = min(c0 + CV_G, Cin);
        for (int i = 0; i < ksize; ++i)
            for (int j = 0; j < ksize; ++j) {
                const int hh = h + i - r, vv = v + j - r;
                const bool inside = hh >= 0 && hh < H && vv >= 0 && vv < W;
                const float *px = xb + (inside ? ((size_t)hh * W + vv) * Cin : 0);
                const float *wt = a.w + (size_t)(i * ksize + j) * Cin;
                if (VEC) {
                    for (int c = c0; c < c1; c += 4) {
                        const cv_f4 f = inside ? *reinterpret_cast<const cv_f4 *>(px + c) : cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
                        acc = fmaf(f.x, wt[c], acc);
                        acc = fmaf(f.y, wt[c + 1], acc);
                        acc = fmaf(f.z, wt[c + 2], acc);
                        acc = fmaf(f.w, wt[c + 3], acc);
                    }
                } else {
                    for (int c = c0; c < c1; ++c) acc = fmaf(inside ? px[c] : 0.0f, wt[c], acc);
                }
            }
    }
    a.out[(size_t)idx * a.out_channels + a.out_offset] = conv_finish(acc, a, 0);
}

constexpr int CV_MAX_BLOCKS = 1 << 20;  // k_conv_mfma's grid: beyond it a block takes several tiles

template <int KS>
void conv_mfma_launch(hipStream_t st, const ConvArgs &a) {
    const int tiles_x = (a.W + CV_TW - 1) / CV_TW, tiles_y = (a.H + CV_TH - 1) / CV_TH;
    const long long n_tiles = (long long)a.B * tiles_y * tiles_x;  // (< 2^31: B H W is)
    const int grid = (int)(n_tiles < CV_MAX_BLOCKS ? n_tiles : CV_MAX_BLOCKS);
    if (a.Cin == 1)
        k_conv_mfma<KS, true, false><<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, (int)n_tiles);
    else if (((uintptr_t)a.x & 15) == 0)
        k_conv_mfma<KS, false, true><<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, (int)n_tiles);
    else
        k_conv_mfma<KS, false, false><<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, (int)n_tiles);
}

inline void conv_launch(hipStream_t st, const ConvArgs &a, int ksize, int Cout) {
    if (Cout == 1) {
        const int n = a.B * a.H * a.W;
        const unsigned grid = (unsigned)(((long long)n + 255) / 256);
        if (a.Cin % 4 == 0 && ((uintptr_t)a.x & 15) == 0)
            k_conv_chain<true><<<grid, 256, 0, st>>>(a, ksize, n);
        else
            k_conv_chain<false><<<grid, 256, 0, st>>>(a, ksize, n);
        return;
    }
    switch (ksize) {
        case 1: conv_mfma_launch<1>(st, a); break;
        case 3: conv_mfma_launch<3>(st, a); break;
        case 5: conv_mfma_launch<5>(st, a); break;
        default: conv_mfma_launch<7>(st, a); break;
    }
}
