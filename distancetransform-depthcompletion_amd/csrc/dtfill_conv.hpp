// dtfill_conv.hpp -- 'same' float32 convolutions in a fixed summation order on the matrix cores: the layers of SparsityCNN
// (solution_DeepNet/net.py:11-242) and the wide layers of ResNet18_NO_BN_l2 (net.py:245-745), stride 1 and 2 with TensorFlow's
// 'same' rule, many output-channel tiles, a fused residual add, and the 3x3 stride-2 transposed convolution; and the layer of
// ResNet18_NO_BN_l2_image that reads the image, 2 to 4 channels into many (k_conv_image, with its own note).  include/dtfill.h,
// dtfill_conv2d(), dtfill_conv2d_strided(), dtfill_conv2d_transpose() and dtfill_conv2d_image(), has the contracts.  Part of libdtfill.so; included
// by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// The contract is one fmaf chain per output: groups of CV_G input channels outermost, then the taps in raster order, then
// the channels of the group.  v_mfma_f32_16x16x4_f32 adds its four k-products to C in k order with one rounding each, so a
// run of MFMAs whose k index walks the chain's order IS the chain, for 16 pixels x 16 output channels at once.  Every MFMA
// kernel here is that implicit GEMM: M = CV_M pixels of a row, N = 16 output channels, K = the chain.  A block of four waves
// takes a tile of pixels and, group by group, stages the haloed tile of the group's 16 channels in LDS (conv_stage); a lane
// (pixel m, k index kq) reads its operand of a tap's four k-steps by one 16-byte read (conv_tap) and ends as (channel m,
// pixels 4 kq .. 4 kq + 3) of each accumulator.  Padding taps are staged as +0.0f and multiplied like any other.
// The epilogue (bounds by the geometry's inside(), output pixel by its at(), conv_store) is a loop nest over the accumulators
// written in each of the two kernel bodies, on purpose: in a function of its own the loops are unrolled before it is inlined,
// every index into acc[][] is then a constant, and the compiler's alloca-to-vector promotion makes the 8 or 16 accumulators one
// 32- or 64-float vector before they are split: the stride-2 kernels went from 87 and 181 VGPRs to 212 and 256 with spills.
//   k_conv_mfma   Cout == 16, stride 1.  The tile is CV_TH x CV_TW pixels, a wave holds two rows of it as four M-tiles: four
//                 independent accumulators that share one weight fragment per k-step (the 16x16x4 form has 40 cycles of
//                 dependent latency against a 32-cycle issue interval).  The weight fragments come straight from global
//                 memory (every wave of the device reads the same 50 KB a group), asked for a row of taps ahead of their use.
//                 Cin == 1: a k-step is four consecutive taps, the last step padded with zero operands on both sides (+0 *
//                 +0 added to the chain: only the sign of a zero can change); the tile is one channel, staged and walked
//                 here, and the weight fragment is w[64 s + lane].
//   k_conv_wide   the same with an N loop: the staged tile serves CV_NB output-channel tiles of 16 in one pass, so the 16-byte
//                 LDS read that feeds one M-tile's four k-steps feeds 4 CV_NB MFMAs, not 4.  A work item is (pixel tile, pass
//                 of 16 CV_NB output channels), the pass fastest, so that the blocks that share an input tile run together;
//                 a layer with Cout > 64 stages its input Cout / 64 times, not Cout / 16.  A tap's 4 CV_NB weight fragments
//                 are asked for one tap ahead of their use (64 MFMAs, 2048 cycles).  Registers: 16 CV_NB accumulators,
//                 8 CV_NB weights, 16 operands: two blocks a CU.  What a layer's geometry decides is a type:
//                   ConvPlain<KS, S>  stride S.  S == 1: the tile is 8 x 32 output pixels and a wave holds two rows as four
//                                     M-tiles; S == 2: 4 x 32 and a wave holds one row as two M-tiles, so that the input
//                                     tile (9 x 65 pixels for 3x3) stays at 38 KB.  At stride 2 a lane's pixels are two
//                                     input columns apart, so the tile is staged de-interleaved by column parity,
//                                     [row][parity][column / 2]: tap j reads plane j & 1 at column m + (j >> 1), unit
//                                     stride again.  k_conv_mfma has ConvPlain<KS, 1>'s tile and LDS extents.
//                   ConvTransposed    four stride-1 correlations of the input grid, one per output parity, with 1, 2, 2
//                                     and 4 taps; the parity is part of the work item.  The tile is 8 x 32 INPUT pixels
//                                     with one halo row above and one halo column to the left; a lane's
//                                     stores go to output pixels two apart.
//   k_conv_chain  Cout == 1 (3x3x16 -> 1, 1x1x16 -> 1: under 0.3 % of the net's work): one lane per pixel, the chain literally, the
//                 channels of a tap by 16-byte loads where x allows.
// The LDS image.  The 16 channels of a pixel lie as a 4 x 4 transpose, channel c at position c >> 2 of quarter c & 3, so that
// lane (pixel m, k quarter k) finds channels k, 4 + k, 8 + k, 12 + k in one quarter.  The quarters of the pixel at linear index P
// of the image are exchanged by bit 2 of P (conv_slot), the one bank rule: ds_read_b128 serves a wave in four groups of 16
// lanes that mix two k quarters ({0-3, 12-15, 20-27}, ...), four sets {m, m + 4, m + 8, m + 12} with k quarters {k, k', k', k}
// (k' = k ^ 1).  A set's pixels are P, P + 4, P + 8, P + 12, so it shares P mod 4 and with it its 16 banks, and sets differ
// in P mod 4; bit 2 of P alternates along a set, b, ~b, b, ~b, which makes its quarters k ^ 2 b, k' ^ 2 ~b, k' ^ 2 b, k ^ 2 ~b:
// all four.  So no two lanes of a group meet on a bank, for every base, row pitch and tap offset.  The argument uses only
// that the bit alternates along a set, which lies in one row of the image; bit 2 of P - K does as well, for any K that is the
// same along a row.  k_conv_mfma takes K = the row's first pixel, bit 2 of the column (conv_slot<true>), because with K = 0 the
// exchange differs between the two rows a wave holds and a tap takes two address registers where the column takes one:
// 82, 94 and 108 VGPRs against 74, 90 and 108, the 3x3 kernel a wave a SIMD short.
// The weight fragment of tap T, k-step s, N-tile n is w[T][16 g + 4 s + (lane >> 4)][n0 + 16 n + (lane & 15)]: 16 lanes read
// 64 consecutive bytes (Cout == 16: the 64 lanes 64 consecutive floats, w[(T Cin + 16 g) 16 + 64 s + lane]).
// ------------------------------------------------------------------------------------------------
constexpr int CV_TH = 8;   // the block tile: rows (4 at stride 2) ...
constexpr int CV_TW = 32;  // ... and pixels of a row
constexpr int CV_M = 16;   // pixels of a row per MFMA tile
constexpr int CV_G = 16;   // input channels per group of the chain
constexpr int CV_NB = 4;   // N-tiles (16 output channels each) of a pass of k_conv_wide
constexpr int CV_MAX_BLOCKS = 1 << 20;  // the grid of the MFMA kernels: beyond it a block takes several work items
static_assert(CV_TH == 2 * 4 && CV_TW == 2 * CV_M, "a wave holds two rows of the tile, two M-tiles each");

typedef float cv_f4 __attribute__((ext_vector_type(4)));

// H, W: the input frame; Ho, Wo: the output frame; pt, pl: the padding in front, rows and columns ('same' convolutions)
struct ConvArgs {
    const float *x, *w, *bias, *res;
    float *out;
    int B, H, W, Cin, Cout, Ho, Wo, pt, pl, out_channels, out_offset, act;
    float alpha;
};

// the bias, the residual and the activation: two rounded adds, then y > 0 ? y : y * alpha.  RES: the entry point has a residual
// argument (a kernel without one carries no code for it: its epilogue is what bounds the registers of the Cin == 1 kernels)
template <bool RES>
__device__ __forceinline__ float conv_finish(float acc, const ConvArgs &a, int o, size_t pixel) {
#pragma clang fp contract(off)
    float y = acc;
    if (a.bias) y = y + a.bias[o];
    if (RES && a.res) y = y + a.res[pixel * a.Cout + o];
    if (a.act == DTFILL_CONV_LEAKY) y = y > 0.0f ? y : y * a.alpha;
    return y;
}

// output channel o of output pixel `pixel`: finished and stored at out_offset of a tensor out_channels wide (a dword store for
// any alignment; the 16 lanes of an N-tile store 64 contiguous bytes)
template <bool RES>
__device__ __forceinline__ void conv_store(float acc, const ConvArgs &a, size_t pixel, int o) {
    a.out[pixel * a.out_channels + a.out_offset + o] = conv_finish<RES>(acc, a, o, pixel);
}

// float index of k quarter k of the pixel at linear index P of the LDS image
// (COL: the exchange goes by bit 2 of c, the pixel's place in its row of the image, not of P: k_conv_mfma's staging and reads)
template <bool COL = false>
__device__ __forceinline__ int conv_slot(int P, int k, int c = 0) { return P * CV_G + 4 * (k ^ (((COL ? c : P) >> 1) & 2)); }

// Stages input pixels (ih0 + r, iv0 + lc), r < LH, lc < LWS, channels 16 g .. 16 g + 15, +0 outside the frame, into the LDS
// image [LH][S planes][LWH]: column lc in plane lc % S at lc / S.
template <int S, int LH, int LWS, int LWH, bool VEC, bool COL = false>
__device__ __forceinline__ void conv_stage(float *s_x, const float *__restrict__ xb, int H, int W, int Cin, int g, int ih0, int iv0,
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
        s_x[conv_slot<COL>(P, 0, lc / S) + s] = f.x;  // channel 4 s + k at position s of k's quarter
        s_x[conv_slot<COL>(P, 1, lc / S) + s] = f.y;
        s_x[conv_slot<COL>(P, 2, lc / S) + s] = f.z;
        s_x[conv_slot<COL>(P, 3, lc / S) + s] = f.w;
    }
}

// The weight fragments of one tap: d[NB s + n] = wt[(4 s) Cout + 16 n + lo], where wt + lo = w + (tap Cin + 16 g + kq) Cout + n0 + m.
// k_conv_mfma gives the lane's part as lo = 16 kq + m = lane beside a wave-uniform wt, one address register for a row of taps;
// k_conv_wide has it inside wt (lo = 0), a 64-bit address a tap.  (Given the uniform form too, its 3x3 kernels drop from 219 and
// 181 VGPRs to 148 and 110 and spill 54 SGPRs: another schedule, a tuning change and not this header's business.)
template <int NB>
__device__ __forceinline__ void conv_weights(const float *__restrict__ wt, int lo, int Cout, int nt, float (&d)[4 * NB]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int n = 0; n < NB; ++n) d[NB * s + n] = n < nt ? (wt + (size_t)4 * s * Cout + 16 * n)[lo] : 0.0f;
}

// one tap's links of the chain: the MT M-tiles' operands at LDS pixels P[q] + dP, four k-steps, nt N-tiles
template <int MT, int NB>
__device__ __forceinline__ void conv_tap(const float *s_x, const int (&P)[MT], int dP, int kq, const float (&wr)[4 * NB], int nt,
                                         cv_f4 (&acc)[MT][NB]) {
    cv_f4 xv[MT];
#pragma unroll
    for (int q = 0; q < MT; ++q) xv[q] = *reinterpret_cast<const cv_f4 *>(s_x + conv_slot(P[q] + dP, kq));
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int n = 0; n < NB; ++n)
            if (n < nt) {
#pragma unroll
                for (int q = 0; q < MT; ++q) acc[q][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q][s], wr[NB * s + n], acc[q][n], 0, 0, 0);
            }
}

// conv_tap with the next tap's fragments (at wnext, if there is one) asked for before this tap's MFMAs
template <int MT>
__device__ __forceinline__ void conv_tap_ahead(const float *s_x, const int (&P)[MT], int dP, int kq, const float *__restrict__ wnext,
                                               bool more, int Cout, int nt, float (&wr)[4 * CV_NB], cv_f4 (&acc)[MT][CV_NB]) {
    float wn[4 * CV_NB];
    if (more) conv_weights<CV_NB>(wnext, 0, Cout, nt, wn);
    conv_tap<MT, CV_NB>(s_x, P, dP, kq, wr, nt, acc);
    if (more) {
#pragma unroll
        for (int k = 0; k < 4 * CV_NB; ++k) wr[k] = wn[k];
    }
}

template <int MT, int NB>
__device__ __forceinline__ void conv_zero(cv_f4 (&acc)[MT][NB]) {
#pragma unroll
    for (int q = 0; q < MT; ++q)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[q][n] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
}

// Work item `item` of B x tiles_y x tiles_x x NPAR x npass in (frame, tile row, tile column, parity, pass) order; a block takes
// the items blockIdx.x, blockIdx.x + gridDim.x, ...
struct ConvItem {
    int b, ty, tx, par, pass;
};
template <int NPAR>
__device__ __forceinline__ ConvItem conv_item(long long item, int tiles_x, int tiles_y, int npass) {
    const long long rest = item / npass, tile = rest / NPAR;
    return {(int)(tile / tiles_x / tiles_y), (int)(tile / tiles_x % tiles_y), (int)(tile % tiles_x), (int)(rest % NPAR), (int)(item % npass)};
}

// What a geometry says: the tile (RW rows a wave, TH rows, MT M-tiles a wave), the LDS image ([LH][S planes][LWH] of LH x LWS
// staged pixels from input pixel (row0, col0)), the lane's LDS pixel of M-tile q under offset 0, the taps of the chain in order as
// (index into w, LDS offset) with tap(k) the index of the k-th, and for row h, column v of the tile grid whether it has an output
// pixel (inside) and which (at).
template <int KS, int S>
struct ConvPlain {
    static constexpr int NPAR = 1, STRIDE = S, RW = S == 1 ? 2 : 1, TH = 4 * RW, MT = 2 * RW;
    static constexpr int LH = (TH - 1) * S + KS, LWS = (CV_TW - 1) * S + KS, LWH = CV_TW + (KS - 1 + S - 1) / S;
    static constexpr int UJ = KS <= 3 ? KS : 1;  // a row of taps is unrolled only where its weights fit the registers
    __device__ __forceinline__ ConvPlain(int) {}
    static __device__ __forceinline__ int lane_pixel(int wave, int m, int q) { return (RW * wave + (q >> 1)) * S * S * LWH + CV_M * (q & 1) + m; }
    __device__ __forceinline__ int row0(const ConvArgs &a, int h0) const { return S * h0 - a.pt; }
    __device__ __forceinline__ int col0(const ConvArgs &a, int v0) const { return S * v0 - a.pl; }
    __device__ __forceinline__ int tap(int k) const { return k; }
    __device__ __forceinline__ void walk(const float *s_x, const int (&P)[MT], int kq, const float *__restrict__ wl, size_t wtap, int Cout,
                                         int nt, float (&wr)[4 * CV_NB], cv_f4 (&acc)[MT][CV_NB]) const {
#pragma unroll 1
        for (int i = 0; i < KS; ++i) {
#pragma unroll UJ
            for (int j = 0; j < KS; ++j)
                conv_tap_ahead<MT>(s_x, P, (i * S + j % S) * LWH + j / S, kq, wl + (size_t)(i * KS + j + 1) * wtap, j + 1 < KS || i + 1 < KS, Cout,
                                   nt, wr, acc);
        }
    }
    __device__ __forceinline__ bool inside(const ConvArgs &a, int h, int v) const { return h < a.Ho && v < a.Wo; }
    __device__ __forceinline__ size_t at(const ConvArgs &a, int b, int h, int v) const { return ((size_t)b * a.Ho + h) * a.Wo + v; }
};

// The tile grid is the input frame a.H x a.W, its outputs the pixels (2 h + py, 2 v + px) of a.Ho = 2 H, a.Wo = 2 W.
struct ConvTransposed {
    static constexpr int NPAR = 4, STRIDE = 1, RW = 2, TH = CV_TH, MT = 4, LH = CV_TH + 1, LWS = CV_TW + 1, LWH = CV_TW + 1;
    // the taps of this parity in raster order: ky = 1 for an odd row, 0 then 2 for an even one; tap 2 reads the pixel before
    const int py, px, nkx, ntap;
    __device__ __forceinline__ ConvTransposed(int par) : py(par >> 1), px(par & 1), nkx(2 - px), ntap((2 - py) * nkx) {}
    static __device__ __forceinline__ int lane_pixel(int wave, int m, int q) { return (RW * wave + (q >> 1) + 1) * LWH + CV_M * (q & 1) + m + 1; }
    __device__ __forceinline__ int row0(const ConvArgs &, int h0) const { return h0 - 1; }
    __device__ __forceinline__ int col0(const ConvArgs &, int v0) const { return v0 - 1; }
    __device__ __forceinline__ int tap(int k) const {
        const int ay = px ? k : k >> 1, ax = px ? 0 : k & 1;  // k = nkx ay + ax; tap (py + 2 ay, px + 2 ax): ay, ax pixels back
        return 3 * (py + 2 * ay) + px + 2 * ax;
    }
    __device__ __forceinline__ void walk(const float *s_x, const int (&P)[MT], int kq, const float *__restrict__ wl, size_t wtap, int Cout,
                                         int nt, float (&wr)[4 * CV_NB], cv_f4 (&acc)[MT][CV_NB]) const {
#pragma unroll 1
        for (int k = 0; k < ntap; ++k) {
            const int ay = px ? k : k >> 1, ax = px ? 0 : k & 1;
            const bool more = k + 1 < ntap;
            conv_tap_ahead<MT>(s_x, P, -(ay * LWH + ax), kq, wl + (size_t)(more ? tap(k + 1) : 0) * wtap, more, Cout, nt, wr, acc);
        }
    }
    __device__ __forceinline__ bool inside(const ConvArgs &a, int h, int v) const { return h < a.H && v < a.W; }
    __device__ __forceinline__ size_t at(const ConvArgs &a, int b, int h, int v) const {
        return ((size_t)b * a.Ho + 2 * h + py) * a.Wo + 2 * v + px;
    }
};

template <class G, bool VEC>
__global__ __launch_bounds__(256, 2) void k_conv_wide(ConvArgs a, int tiles_x, int tiles_y, int npass, long long n_items) {
    constexpr int S = G::STRIDE, MT = G::MT;
    __shared__ __attribute__((aligned(16))) float s_x[G::LH * S * G::LWH * CV_G];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;  // A: pixel m, k index kq; B: k index kq, output channel m; D: channel m, pixels 4 kq ..+3
    const int Cin = a.Cin, Cout = a.Cout;
    const int groups = Cin / CV_G;
    int P[MT];
#pragma unroll
    for (int q = 0; q < MT; ++q) P[q] = G::lane_pixel(wave, m, q);
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const ConvItem it = conv_item<G::NPAR>(item, tiles_x, tiles_y, npass);
        const G geo(it.par);
        const int h0 = it.ty * G::TH, v0 = it.tx * CV_TW, n0 = it.pass * 16 * CV_NB;
        const int nt = min(CV_NB, (Cout - n0) / 16);
        const float *xb = a.x + (size_t)it.b * a.H * a.W * Cin;
        cv_f4 acc[MT][CV_NB];
        conv_zero(acc);
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
            const float *wl = a.w + ((size_t)g * CV_G + kq) * Cout + n0 + m;
            const size_t wtap = (size_t)Cin * Cout;
            float wr[4 * CV_NB];  // the group's first tap is asked for before its tile is staged
            conv_weights<CV_NB>(wl + (size_t)geo.tap(0) * wtap, 0, Cout, nt, wr);
            conv_stage<S, G::LH, G::LWS, G::LWH, VEC>(s_x, xb, a.H, a.W, Cin, g, geo.row0(a, h0), geo.col0(a, v0), t);
            __syncthreads();
            geo.walk(s_x, P, kq, wl, wtap, Cout, nt, wr, acc);
            __syncthreads();  // the tile is rewritten by the next group, or the next item
        }
        // ---- the epilogue (see the note above): M-tile q is the half q & 1 of the wave's row q >> 1 ----
#pragma unroll
        for (int q = 0; q < MT; ++q) {
            const int h = h0 + G::RW * wave + (q >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = v0 + CV_M * (q & 1) + 4 * kq + e;
                if (geo.inside(a, h, v)) {
                    const size_t pixel = geo.at(a, it.b, h, v);
#pragma unroll
                    for (int n = 0; n < CV_NB; ++n)
                        if (n < nt) conv_store<true>(acc[q][n][e], a, pixel, n0 + 16 * n + m);
                }
            }
        }
    }
}

// Cout == 16, stride 1: one N-tile, one pass; ConvPlain<KS, 1>'s tile, the exchange by the column, and a walk, tap reads and an
// output index of its own: through conv_tap's P[] the compiler kept a register for each of the wave's two rows and issued a
// tap's reads in pairs (the 7x7x64 layer 2 % slower), and the geometry's 64-bit at() cost the 1x1 kernel a wave a SIMD.
template <int KS, bool CIN1, bool VEC>
__global__ __launch_bounds__(256) void k_conv_mfma(ConvArgs a, int tiles_x, int tiles_y, int /* npass: 1 */, long long n_items) {
    typedef ConvPlain<KS, 1> G;
    constexpr int R = (KS - 1) / 2, LH = G::LH, LW = G::LWH, PC = CIN1 ? 1 : CV_G, TAPS = KS * KS;
    static_assert(G::TH == CV_TH && G::MT == 4 && G::LWS == LW, "two rows of the tile a wave, two M-tiles each");
    __shared__ __attribute__((aligned(16))) float s_x[LH * LW * PC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int H = a.H, W = a.W, Cin = a.Cin;
    const int groups = CIN1 ? 1 : Cin / CV_G;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const ConvItem it = conv_item<1>(item, tiles_x, tiles_y, 1);
        const int h0 = it.ty * CV_TH, v0 = it.tx * CV_TW;
        const float *xb = a.x + (size_t)it.b * H * W * Cin;
        cv_f4 acc[4][1];
        conv_zero(acc);
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
            // the weight fragments of a row of taps, held in registers a row ahead: the group's first row is asked for before
            // its tile is staged, row i + 1 before row i's MFMAs
            const float *wg = a.w + (size_t)g * CV_G * 16;
            const size_t wtap = (size_t)Cin * 16;
            float wr[KS][4];
            if (!CIN1) {
#pragma unroll
                for (int j = 0; j < KS; ++j) conv_weights<1>(wg + j * wtap, lane, 16, 1, wr[j]);
            }
            // ---- the haloed tile of this group's channels, +0 outside the frame ----
            if (CIN1) {
                for (int p = t; p < LH * LW; p += 256) {
                    const int r = p / LW, c = p - r * LW;
                    const int h = h0 + r - R, v = v0 + c - R;
                    s_x[p] = h >= 0 && h < H && v >= 0 && v < W ? xb[(size_t)h * W + v] : 0.0f;
                }
            } else {
                conv_stage<1, LH, LW, LW, VEC, true>(s_x, xb, H, W, Cin, g, h0 - R, v0 - R, t);
            }
            __syncthreads();
            // ---- the group's part of the chain ----
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
                        const float xv = s_x[(2 * wave + (q >> 1) + i) * LW + CV_M * (q & 1) + m + j];
                        acc[q][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(real ? xv : 0.0f, wv, acc[q][0], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll 1
                for (int i = 0; i < KS; ++i) {
                    float wn[KS][4];  // the next row of taps, asked for before this row's MFMAs
                    if (i + 1 < KS) {
#pragma unroll
                        for (int j = 0; j < KS; ++j) conv_weights<1>(wg + ((i + 1) * KS + j) * wtap, lane, 16, 1, wn[j]);
                    }
#pragma unroll
                    for (int j = 0; j < KS; ++j) {
                        // the tap's four reads, written from the lane's own numbers: one address register and four immediate
                        // offsets (the halves 1 KB apart, the rows a pitch apart), issued together
                        cv_f4 xv[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int c = CV_M * (q & 1) + m + j;
                            xv[q] = *reinterpret_cast<const cv_f4 *>(s_x + conv_slot<true>((2 * wave + (q >> 1) + i) * LW + c, kq, c));
                        }
#pragma unroll
                        for (int s = 0; s < 4; ++s)
#pragma unroll
                            for (int q = 0; q < 4; ++q) acc[q][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q][s], wr[j][s], acc[q][0], 0, 0, 0);
                    }
                    if (i + 1 < KS) {
#pragma unroll
                        for (int j = 0; j < KS; ++j)
#pragma unroll
                            for (int k = 0; k < 4; ++k) wr[j][k] = wn[j][k];
                    }
                }
            }
            __syncthreads();  // the tile is rewritten by the next group, or the next item
        }
        // ---- the epilogue (see the note above), one N-tile ----
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int h = h0 + 2 * wave + (q >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = v0 + CV_M * (q & 1) + 4 * kq + e;
                if (h < H && v < W) conv_store<false>(acc[q][0][e], a, ((size_t)it.b * H + h) * W + v, m);
            }
        }
    }
}

// dtfill_conv2d_image: CIN of 2, 3 or 4 (the RGB stem img_conv, net.py:3407) into many output channels.  One group, so the
// chain is the taps in raster order and within a tap the channels: KS KS CIN links laid flat, link l = tap CIN + c, and k-step
// s holds the links 4 s .. 4 s + 3, whichever taps they belong to.  The count is no multiple of 4 in general (27 for the stem):
// the links past the chain's end in the last step have +0 on BOTH sides, the x operand never read, so that only the sign of a
// zero can change and no zero meets a non-finite partner.  The tile is ConvPlain<KS, 1>'s, four M-tiles a wave, and a work
// item is k_conv_wide's (pixel tile, pass of CV_NB N-tiles): one LDS operand read feeds CV_NB MFMAs.  The LDS image is plain,
// [row][column][CIN] as x itself is, so the links of a tile row's window are consecutive floats: link l of the pixel at
// float P CIN lies at P CIN + l + (l / (KS CIN)) (LW - KS) CIN, and w[l][o] is w's own layout.  A lane reads one float a step
// (ds_read_b32, banks of 32 lanes: pixels CIN floats apart, two-way conflicts at CIN 3 and 4; the kernel is bound by its stores).
// The weights of a step are asked for a step ahead of their use.
template <int KS, int CIN>
__global__ __launch_bounds__(256, 2) void k_conv_image(ConvArgs a, int tiles_x, int tiles_y, int npass, long long n_items) {
    typedef ConvPlain<KS, 1> G;
    constexpr int R = (KS - 1) / 2, LH = G::LH, LW = G::LWH, LINKS = KS * KS * CIN, STEPS = (LINKS + 3) / 4, ROW = KS * CIN;
    constexpr int UN = KS <= 3 ? STEPS : 1;  // the short chains are unrolled whole
    static_assert(CIN >= 2 && CIN <= 4 && G::TH == CV_TH && G::MT == 4 && G::LWS == LW, "ConvPlain<KS, 1>'s tile, fewer channels than a k-step");
    __shared__ __attribute__((aligned(16))) float s_x[LH * LW * CIN];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int H = a.H, W = a.W, Cout = a.Cout;
    int P[4];  // the float offset of M-tile q's pixel under tap (0, 0)
#pragma unroll
    for (int q = 0; q < 4; ++q) P[q] = ((2 * wave + (q >> 1)) * LW + CV_M * (q & 1) + m) * CIN;
    // the lane's link of step s, 4 s + kq: whether it is one of the chain's, and where its operands lie
    auto link = [&](int s, bool &real, int &xoff, int &woff) {
        const int l = 4 * s + kq;
        real = l < LINKS;
        xoff = real ? l + (l / ROW) * (LW - KS) * CIN : 0;
        woff = real ? l * Cout : 0;
    };
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const ConvItem it = conv_item<1>(item, tiles_x, tiles_y, npass);
        const int h0 = it.ty * CV_TH, v0 = it.tx * CV_TW, n0 = it.pass * 16 * CV_NB;
        const int nt = min(CV_NB, (Cout - n0) / 16);
        const float *xb = a.x + (size_t)it.b * H * W * CIN;
        const float *wl = a.w + n0 + m;
        // ---- the haloed tile, +0 outside the frame: a row of it is LW CIN consecutive floats of x ----
        for (int e = t; e < LH * LW * CIN; e += 256) {
            const int r = e / (LW * CIN), rest = e - r * (LW * CIN);
            const int h = h0 + r - R, v = v0 + rest / CIN - R;
            s_x[e] = h >= 0 && h < H && v >= 0 && v < W ? xb[((size_t)h * W + (v0 - R)) * CIN + rest] : 0.0f;
        }
        cv_f4 acc[4][CV_NB];
        conv_zero(acc);
        bool real;
        int xoff, woff;
        float wr[CV_NB];
        link(0, real, xoff, woff);
#pragma unroll
        for (int n = 0; n < CV_NB; ++n) wr[n] = real && n < nt ? wl[woff + 16 * n] : 0.0f;
        __syncthreads();
#pragma unroll UN
        for (int s = 0; s < STEPS; ++s) {
            float xv[4], wn[CV_NB];
#pragma unroll
            for (int q = 0; q < 4; ++q) xv[q] = real ? s_x[P[q] + xoff] : 0.0f;
            if (s + 1 < STEPS) {
                link(s + 1, real, xoff, woff);
#pragma unroll
                for (int n = 0; n < CV_NB; ++n) wn[n] = real && n < nt ? wl[woff + 16 * n] : 0.0f;
            }
#pragma unroll
            for (int n = 0; n < CV_NB; ++n)
                if (n < nt) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[q], wr[n], acc[q][n], 0, 0, 0);
                }
            if (s + 1 < STEPS) {
#pragma unroll
                for (int n = 0; n < CV_NB; ++n) wr[n] = wn[n];
            }
        }
        __syncthreads();  // the tile is rewritten by the next item
        // ---- the epilogue (see the note above): M-tile q is the half q & 1 of the wave's row q >> 1 ----
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int h = h0 + 2 * wave + (q >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = v0 + CV_M * (q & 1) + 4 * kq + e;
                if (h < H && v < W) {
                    const size_t pixel = ((size_t)it.b * H + h) * W + v;
#pragma unroll
                    for (int n = 0; n < CV_NB; ++n)
                        if (n < nt) conv_store<false>(acc[q][n][e], a, pixel, n0 + 16 * n + m);
                }
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
    a.out[(size_t)idx * a.out_channels + a.out_offset] = conv_finish<false>(acc, a, 0, (size_t)idx);
}

// The grid of an MFMA kernel: the frame h x w in tiles of tile_h x CV_TW, npar parities and the passes of a.Cout a tile;
// `vec` where x allows 16-byte loads.
typedef void (*conv_kernel)(ConvArgs, int, int, int, long long);
inline void conv_launch_items(hipStream_t st, const ConvArgs &a, int h, int w, int tile_h, int npar, conv_kernel vec, conv_kernel any) {
    const int tiles_x = (w + CV_TW - 1) / CV_TW, tiles_y = (h + tile_h - 1) / tile_h, npass = (a.Cout + 16 * CV_NB - 1) / (16 * CV_NB);
    const long long n_items = (long long)a.B * tiles_y * tiles_x * npar * npass;  // (tiles < 2^31: B H W is)
    const int grid = (int)(n_items < CV_MAX_BLOCKS ? n_items : CV_MAX_BLOCKS);
    (((uintptr_t)a.x & 15) == 0 ? vec : any)<<<grid, 256, 0, st>>>(a, tiles_x, tiles_y, npass, n_items);
}

template <int KS, int S>
void conv_wide_launch(hipStream_t st, const ConvArgs &a) {
    typedef ConvPlain<KS, S> G;
    conv_launch_items(st, a, a.Ho, a.Wo, G::TH, G::NPAR, k_conv_wide<G, true>, k_conv_wide<G, false>);
}

template <int KS>
void conv_mfma_launch(hipStream_t st, const ConvArgs &a) {
    if (a.Cin == 1)
        conv_launch_items(st, a, a.Ho, a.Wo, CV_TH, 1, k_conv_mfma<KS, true, false>, k_conv_mfma<KS, true, false>);
    else
        conv_launch_items(st, a, a.Ho, a.Wo, CV_TH, 1, k_conv_mfma<KS, false, true>, k_conv_mfma<KS, false, false>);
}

// dtfill_conv2d_strided
inline void conv_strided_launch(hipStream_t st, const ConvArgs &a, int ksize, int stride) {
    if (stride == 2) {
        if (ksize == 1)
            conv_wide_launch<1, 2>(st, a);
        else
            conv_wide_launch<3, 2>(st, a);
        return;
    }
    switch (ksize) {
        case 1: conv_wide_launch<1, 1>(st, a); break;
        case 3: conv_wide_launch<3, 1>(st, a); break;
        case 5: conv_wide_launch<5, 1>(st, a); break;
        default: conv_wide_launch<7, 1>(st, a); break;
    }
}

// dtfill_conv2d_transpose
inline void conv_transpose_launch(hipStream_t st, const ConvArgs &a) {
    conv_launch_items(st, a, a.H, a.W, ConvTransposed::TH, ConvTransposed::NPAR, k_conv_wide<ConvTransposed, true>,
                      k_conv_wide<ConvTransposed, false>);
}

// dtfill_conv2d: Cout is 1 or 16
inline void conv_launch(hipStream_t st, const ConvArgs &a, int ksize) {
    if (a.Cout == 1) {
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

// dtfill_conv2d_image: Cin is 2, 3 or 4, Cout a multiple of 16
template <int KS>
void conv_image_launch_k(hipStream_t st, const ConvArgs &a) {
    const conv_kernel k = a.Cin == 2 ? k_conv_image<KS, 2> : a.Cin == 3 ? k_conv_image<KS, 3> : k_conv_image<KS, 4>;
    conv_launch_items(st, a, a.Ho, a.Wo, CV_TH, 1, k, k);  // (scalar loads of x: one kernel for any alignment)
}

inline void conv_image_launch(hipStream_t st, const ConvArgs &a, int ksize) {
    switch (ksize) {
        case 1: conv_image_launch_k<1>(st, a); break;
        case 3: conv_image_launch_k<3>(st, a); break;
        case 5: conv_image_launch_k<5>(st, a); break;
        default: conv_image_launch_k<7>(st, a); break;
    }
}
