// dtfill_convh.hpp -- the wide and transposed convolutions of dtfill_conv.hpp on the bf16 matrix cores with float32
// accumulation: the opt-in inference precision of the three ResNets.  include/dtfill.h, dtfill_conv2d_strided_bf16(),
// dtfill_conv2d_transpose_bf16() and dtfill_conv2d_pack_bf16(), has the contract.  Part of libdtfill.so; included by dtfill.hip
// inside its anonymous namespace, behind dtfill_conv.hpp, whose geometry types (ConvPlain<KS, S>, ConvTransposed), work-item
// order (conv_item), ConvArgs, finish (conv_store) and launch (conv_launch_items) it uses as they are.
#pragma once

// ------------------------------------------------------------------------------------------------
// k_convh_wide is k_conv_wide on v_mfma_f32_16x16x32_bf16: M = CV_M pixels of a row, N = 16 output channels, and ONE k-step
// is a whole group of CH_G = 32 input channels under one tap, where the float32 kernel takes four k-steps for 16.  Lane (m, kq)
// holds A[pixel m][channels 8 kq .. 8 kq + 7] and B[channels 8 kq .. 8 kq + 7][output channel m], 16 bytes each; C/D is the
// float32 form's (channel m, pixels 4 kq .. 4 kq + 3), so the epilogue is k_conv_wide's.  Per output the MFMAs come in a fixed
// order: groups outermost, then the taps in the geometry's raster order, one MFMA per (group, tap).  x stays float32 in
// memory: convh_stage reads it by 16-byte loads, rounds to bf16 in registers (v_cvt_pk_bf16_f32: to nearest even, NaN kept,
// overflow to inf) and writes the haloed 32-channel tile to LDS as bf16.  A group of 32 channels of 2 bytes is as many bytes as a
// group of 16 of 4, so every LDS extent is the float32 kernel's, from the same constants.  A trailing half group (Cin = 16 or
// 48 mod 32) is staged as +0 and packed as +0.
// The LDS image.  A pixel is 64 bytes: four quarters of 8 channels, quarter k = channels 8 k .. 8 k + 7 in their own order (the
// bf16 fragment wants consecutive k, so there is no 4 x 4 transpose here).  Lane (pixel m, quarter kq) reads its tap operand by
// one ds_read_b128.  The bank rule is dtfill_conv.hpp's, for the same reason: a pixel is 16 banks and four pixels are the 64,
// ds_read_b128 serves a wave in four groups of 16 lanes that mix two quarters ({0-3, 12-15, 20-27}, ...), i.e. four sets of
// pixels {P, P + 4, P + 8, P + 12} with quarters {k, k', k', k} (k' = k ^ 1).  A set shares P mod 4 and with it its 16 banks,
// and sets differ in P mod 4.  The quarters of pixel P are exchanged by bit 2 of P (ch_slot), which alternates along a set:
// k ^ 2 b, k' ^ 2 ~b, k' ^ 2 b, k ^ 2 ~b, all four.  So no two lanes of a group meet on a bank, for every base, row pitch and
// tap offset.  convh_stage writes a pixel's quarter by one 16-byte store; eight lanes write two whole pixels, 128 distinct bytes.
// The packed weights (dtfill_conv2d_pack_bf16) are the B fragments as the wave reads them: [tap][group][N-tile][lane][8], the
// fragment of (tap T, group g, N-tile n) 1024 consecutive bytes, lane (kq, m) at 16 (16 kq + m): w[T][32 g + 8 kq + j][16 n + m],
// j = 0 .. 7, +0 where the channel is past Cin.  A tap's CV_NB fragments are asked for one tap ahead of their use, from global
// memory, as k_conv_wide's are.  Registers: 16 CV_NB accumulators, 8 CV_NB weights (this tap's and the next's), 16 operands.
// ------------------------------------------------------------------------------------------------
constexpr int CH_G = 2 * CV_G;         // input channels per group: one k-step of the 16x16x32 MFMA
constexpr int CH_Q = CH_G / 4;         // channels of a lane's fragment: 8 bf16, 16 bytes
constexpr int CH_FRAG = 64;            // ch_b8 elements of a B fragment, one per lane
static_assert(CH_G * 2 == CV_G * 4, "a group's pixel is as many bytes as the float32 kernel's, so the LDS extents carry over");

typedef __bf16 ch_b8 __attribute__((ext_vector_type(8)));
typedef float ch_f8 __attribute__((ext_vector_type(8)));

// float32 -> bf16, to nearest even; NaN stays NaN, overflow goes to inf
__device__ __forceinline__ ch_b8 ch_round(ch_f8 f) { return __builtin_convertvector(f, ch_b8); }

// index (in 16-byte quarters) of quarter k of the pixel at linear index P of the LDS image
__device__ __forceinline__ int ch_slot(int P, int k) { return P * 4 + (k ^ ((P >> 1) & 2)); }

// Stages input pixels (ih0 + r, iv0 + lc), r < LH, lc < LWS, channels 32 g .. 32 g + 31, rounded to bf16, +0 outside the frame
// and past Cin, into the LDS image [LH][S planes][LWH]: column lc in plane lc % S at lc / S (conv_stage's image).
template <int S, int LH, int LWS, int LWH, bool VEC>
__device__ __forceinline__ void convh_stage(ch_b8 *s_x, const float *__restrict__ xb, int H, int W, int Cin, int g, int ih0, int iv0,
                                            int t) {
    for (int e = t; e < LH * LWS * 4; e += 256) {
        const int p = e >> 2, s = e & 3;  // quarter s of staged pixel p
        const int r = p / LWS, lc = p - r * LWS;
        const int h = ih0 + r, v = iv0 + lc, c = g * CH_G + CH_Q * s;
        ch_f8 f{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (h >= 0 && h < H && v >= 0 && v < W && c < Cin) {  // (Cin is a multiple of 16: a quarter is inside or past it whole)
            const float *src = xb + ((size_t)h * W + v) * Cin + c;
            if (VEC) {
                const cv_f4 lo = *reinterpret_cast<const cv_f4 *>(src), hi = *reinterpret_cast<const cv_f4 *>(src + 4);
                f = ch_f8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            } else {
                f = ch_f8{src[0], src[1], src[2], src[3], src[4], src[5], src[6], src[7]};
            }
        }
        s_x[ch_slot((r * S + lc % S) * LWH + lc / S, s)] = ch_round(f);
    }
}

// The weight fragments of one tap: d[n] = the fragment of N-tile n at wt (which holds the lane's own 16 bytes)
__device__ __forceinline__ void convh_weights(const ch_b8 *__restrict__ wt, int nt, ch_b8 (&d)[CV_NB]) {
#pragma unroll
    for (int n = 0; n < CV_NB; ++n) d[n] = n < nt ? wt[n * CH_FRAG] : ch_round(ch_f8{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f});
}

// one (group, tap): the MT M-tiles' operands at LDS pixels P[q] + dP, one k-step, nt N-tiles; the next tap's fragments (at
// wnext, if there is one) are asked for before this tap's MFMAs
template <int MT>
__device__ __forceinline__ void convh_tap_ahead(const ch_b8 *s_x, const int (&P)[MT], int dP, int kq, const ch_b8 *__restrict__ wnext,
                                                bool more, int nt, ch_b8 (&wr)[CV_NB], cv_f4 (&acc)[MT][CV_NB]) {
    ch_b8 wn[CV_NB], xv[MT];
    if (more) convh_weights(wnext, nt, wn);
#pragma unroll
    for (int q = 0; q < MT; ++q) xv[q] = s_x[ch_slot(P[q] + dP, kq)];
#pragma unroll
    for (int n = 0; n < CV_NB; ++n)
        if (n < nt) {
#pragma unroll
            for (int q = 0; q < MT; ++q) acc[q][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xv[q], wr[n], acc[q][n], 0, 0, 0);
        }
    if (more) {
#pragma unroll
        for (int n = 0; n < CV_NB; ++n) wr[n] = wn[n];
    }
}

// A group's taps in the geometry's order, at the geometry's LDS offsets: G::walk over one k-step a tap.  wl: the lane's
// fragment of tap 0, wtap: ch_b8 elements between two taps.
template <int KS, int S>
__device__ __forceinline__ void convh_walk(const ConvPlain<KS, S> &, const ch_b8 *s_x, const int (&P)[ConvPlain<KS, S>::MT], int kq,
                                           const ch_b8 *__restrict__ wl, size_t wtap, int nt, ch_b8 (&wr)[CV_NB],
                                           cv_f4 (&acc)[ConvPlain<KS, S>::MT][CV_NB]) {
    typedef ConvPlain<KS, S> G;
#pragma unroll
    for (int i = 0; i < KS; ++i) {
#pragma unroll
        for (int j = 0; j < KS; ++j)
            convh_tap_ahead<G::MT>(s_x, P, (i * S + j % S) * G::LWH + j / S, kq, wl + (size_t)(i * KS + j + 1) * wtap, j + 1 < KS || i + 1 < KS,
                                   nt, wr, acc);
    }
}

__device__ __forceinline__ void convh_walk(const ConvTransposed &geo, const ch_b8 *s_x, const int (&P)[ConvTransposed::MT], int kq,
                                           const ch_b8 *__restrict__ wl, size_t wtap, int nt, ch_b8 (&wr)[CV_NB],
                                           cv_f4 (&acc)[ConvTransposed::MT][CV_NB]) {
#pragma unroll 1
    for (int k = 0; k < geo.ntap; ++k) {
        const int ay = geo.px ? k : k >> 1, ax = geo.px ? 0 : k & 1;  // tap k lies ay rows and ax columns back (ConvTransposed::tap)
        const bool more = k + 1 < geo.ntap;
        convh_tap_ahead<ConvTransposed::MT>(s_x, P, -(ay * ConvTransposed::LWH + ax), kq, wl + (size_t)(more ? geo.tap(k + 1) : 0) * wtap, more,
                                            nt, wr, acc);
    }
}

template <class G, bool VEC>
__global__ __launch_bounds__(256, 2) void k_convh_wide(ConvArgs a, int tiles_x, int tiles_y, int npass, long long n_items) {
    constexpr int S = G::STRIDE, MT = G::MT;
    __shared__ ch_b8 s_x[G::LH * S * G::LWH * (CH_G / CH_Q)];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m = lane & 15, kq = lane >> 4;  // A: pixel m, channels 8 kq ..+7; B: channels 8 kq ..+7, output channel m; D: as k_conv_wide
    const int Cin = a.Cin, Cout = a.Cout;
    const int groups = (Cin + CH_G - 1) / CH_G, ntiles = Cout / 16;
    const size_t wtap = (size_t)groups * ntiles * CH_FRAG;
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
            const ch_b8 *wl = reinterpret_cast<const ch_b8 *>(a.w) + ((size_t)g * ntiles + n0 / 16) * CH_FRAG + lane;
            ch_b8 wr[CV_NB];  // the group's first tap is asked for before its tile is staged
            convh_weights(wl + (size_t)geo.tap(0) * wtap, nt, wr);
            convh_stage<S, G::LH, G::LWS, G::LWH, VEC>(s_x, xb, a.H, a.W, Cin, g, geo.row0(a, h0), geo.col0(a, v0), t);
            __syncthreads();
            convh_walk(geo, s_x, P, kq, wl, wtap, nt, wr, acc);
            __syncthreads();  // the tile is rewritten by the next group, or the next item
        }
        // ---- the epilogue, k_conv_wide's (see dtfill_conv.hpp on why it is written out): M-tile q is the half q & 1 of the wave's row q >> 1 ----
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

// dtfill_conv2d_pack_bf16: one lane per 16 bytes of the packed array, n_quads of them
template <int = 0>
__global__ __launch_bounds__(256) void k_convh_pack(const float *__restrict__ w, int Cin, int Cout, ch_b8 *__restrict__ out, long long n_quads) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_quads) return;
    const int groups = (Cin + CH_G - 1) / CH_G, ntiles = Cout / 16;
    const int lane = (int)(idx % CH_FRAG), n = (int)(idx / CH_FRAG % ntiles), g = (int)(idx / CH_FRAG / ntiles % groups);
    const long long T = idx / CH_FRAG / ntiles / groups;
    const int c = g * CH_G + CH_Q * (lane >> 4), o = 16 * n + (lane & 15);
    ch_f8 f{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (c < Cin) {
#pragma unroll
        for (int j = 0; j < CH_Q; ++j) f[j] = w[((size_t)T * Cin + c + j) * Cout + o];
    }
    out[idx] = ch_round(f);
}

// The launches are templates so that the kernels above are asked for where the entry points are, at the end of dtfill.hip, and
// lie behind every older kernel in the code object (dtfill_adam.hpp has the reason).
template <int KS, int S>
void convh_wide_launch(hipStream_t st, const ConvArgs &a) {
    typedef ConvPlain<KS, S> G;
    conv_launch_items(st, a, a.Ho, a.Wo, G::TH, G::NPAR, k_convh_wide<G, true>, k_convh_wide<G, false>);
}

// dtfill_conv2d_strided_bf16: ksize 1 or 3, stride 1 or 2
template <int = 0>
void convh_strided_launch(hipStream_t st, const ConvArgs &a, int ksize, int stride) {
    if (stride == 2)
        ksize == 1 ? convh_wide_launch<1, 2>(st, a) : convh_wide_launch<3, 2>(st, a);
    else
        ksize == 1 ? convh_wide_launch<1, 1>(st, a) : convh_wide_launch<3, 1>(st, a);
}

// dtfill_conv2d_transpose_bf16
template <int = 0>
void convh_transpose_launch(hipStream_t st, const ConvArgs &a) {
    conv_launch_items(st, a, a.H, a.W, ConvTransposed::TH, ConvTransposed::NPAR, k_convh_wide<ConvTransposed, true>,
                      k_convh_wide<ConvTransposed, false>);
}

// the ch_b8 elements (16 bytes each) of the packed weights
inline long long convh_packed_quads(int ksize, int Cin, int Cout) {
    return (long long)ksize * ksize * ((Cin + CH_G - 1) / CH_G) * (Cout / 16) * CH_FRAG;
}
