// dtfill_convhb.hpp -- the backward of the wide and transposed convolutions on the bf16 matrix cores with float32
// accumulation: what precision = "bf16" trains with.  include/dtfill.h, dtfill_conv2d_strided_backward_data_bf16() and its three
// siblings, has the contracts.  Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace, behind
// dtfill_convh.hpp.  It uses as they are: dtfill_convb.hpp's k_convb_g, k_convb_spread, k_convb_sum, convb_g4, ConvBwWide,
// ConvBwGeo, the partials' layout and the launch grid; dtfill_convh.hpp's k_convh_wide and its launches.
#pragma once

// ------------------------------------------------------------------------------------------------
// dx is dtfill_convb.hpp's: a forward over g under the flipped (stride 1) or the exchanged (stride 2, transposed) kernel, here
// on k_convh_wide.  k_convhb_pack writes that kernel straight into dtfill_conv2d_pack_bf16's layout, the index map of
// k_convb_flip folded in: the forward over g has the layer's Cout as its input channels, so a lane's 8 k-values
// wT[T][32 g + 8 kq + j][16 n + m] = w[T'][16 n + m][32 g + 8 kq + j] (T' = taps - 1 - T with flip) are 8 CONSECUTIVE floats of w.
// One launch and no float32 copy of wT, against k_convb_flip + k_convh_pack.
//
// dw and db: k_convhb_dw_wide is k_convb_dw_wide on v_mfma_f32_16x16x32_bf16.  The work item, the grid, the frames, the strips
// (ConvBwGeo), the accumulators per (tap of the wave, tile) and the partials are the float32 kernel's.  A k-step is 32
// consecutive pixels of a row of the small frame, where the float32 kernel takes 4.
// The operand.  Lane l of the MFMA holds A[row l & 15][k = 8 (l >> 4) .. + 7] (and B likewise): EIGHT PIXELS of ONE channel, from
// channels-last tensors.  Both strips are staged as bf16 [pixel][16 channels], 32-byte rows (the stride-2 strip of the large
// tensor split by column parity, [row][parity][column / 2][16], as in the float32 kernel), rounded in registers while staging,
// and a fragment is two ds_read_b64_tr_b16: each 16-lane group reads a block of 4 pixels x 16 channels and every lane
// receives one channel of the 4 pixels.  Group q takes the pixels 4 q .. 4 q + 3 of the k-step with its first read and
// 16 + 4 q .. 16 + 4 q + 3 with its second, 512 bytes on (one base register, one immediate).  So k index 8 q + e of the MFMA is
// pixel 4 q + e (e < 4) or 16 + 4 q + e - 4 of the k-step, on BOTH operands: the product sum is over the 32 pixels either way.
// Lane 16 q + 4 r + p supplies the address of pixel 4 q + r, channels 4 p .. 4 p + 3: byte 32 (4 q + r) + 8 p = 8 l from the
// k-step's first pixel.  The lane's offset is its own index in 8-byte units, whatever the tap.
// Banks ((a / 4) mod 64 per 32-lane half).  A half's 32 lanes read bytes 8 l .. 8 l + 7 for 32 consecutive l: 256 consecutive
// bytes from a 32-byte-aligned base, 64 distinct dwords, hence all 64 banks once.  A tap, a row or the second read moves the
// whole block by a multiple of 32 bytes, which rotates the banks.  No conflict for any tap, pitch or k-step.  (Pixels 8 q ..
// 8 q + 7 for group q, the MFMA's own k order, would put groups 0 and 1 256 bytes apart on the same 32 banks: two-way.)
// Every address is a multiple of 8: rows are 32 bytes, a tap is whole rows.
// EXEC.  The reads stand in wave-uniform code only (the wave index is read with readfirstlane); the edge k-step, whose lanes
// can lie past the frame, reads everything and zeroes by select, so EXEC is all ones at every transposed read.  The strip of
// the small tensor is staged +0 past its frame, and the large operand of the pixels past it is made +0 in registers, as in the
// float32 kernel: +0 on both sides.  CB_C is two whole k-steps, so no k-step crosses a segment.
// ------------------------------------------------------------------------------------------------
constexpr int CHB_K = 32;  // pixels of a k-step
static_assert(CB_C % CHB_K == 0, "a segment's row is whole k-steps");

typedef __bf16 chb_b4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) chb_b4 chb_lds4;

__device__ __forceinline__ chb_b4 chb_round(cv_f4 f) { return __builtin_convertvector(f, chb_b4); }

// the lane's fragment of the k-step whose first pixel is at 8-byte index `at` (4 per pixel) of the LDS image s
__device__ __forceinline__ ch_b8 chb_fragment(const chb_b4 *s, int at, int lane) {
    chb_lds4 *p = (chb_lds4 *)(s + at + lane);
    const chb_b4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p), hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p + 64);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// the pixels of a k-step from `left` on are +0: left = the pixels of the step that lie inside the frame
__device__ __forceinline__ ch_b8 chb_inside(ch_b8 v, int left, int lane) {
    const int q4 = 4 * (lane >> 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = q4 + (e < 4 ? e : 12 + e) < left ? v[e] : (__bf16)0.0f;
    return v;
}

// dtfill_conv2d_pack_bf16's array of the kernel the data gradient runs under: one lane per 16 bytes
template <int = 0>
__global__ __launch_bounds__(256) void k_convhb_pack(const float *__restrict__ w, int taps, int Cin, int Cout, bool flip,
                                                     ch_b8 *__restrict__ out, long long n_quads) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_quads) return;
    const int groups = (Cout + CH_G - 1) / CH_G, ntiles = Cin / 16;  // of the forward over g: Cout in, Cin out
    const int lane = (int)(idx % CH_FRAG), n = (int)(idx / CH_FRAG % ntiles), g = (int)(idx / CH_FRAG / ntiles % groups);
    const int T = (int)(idx / CH_FRAG / ntiles / groups);
    const int o = g * CH_G + CH_Q * (lane >> 4), c = 16 * n + (lane & 15);
    ch_f8 f{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (o < Cout) {
        const float *src = w + ((size_t)(flip ? taps - 1 - T : T) * Cin + c) * Cout + o;
#pragma unroll
        for (int j = 0; j < CH_Q; ++j) f[j] = src[j];
    }
    out[idx] = ch_round(f);
}

template <int KS, int S, bool TR, bool VEC>
__global__ __launch_bounds__(256, 2) void k_convhb_dw_wide(ConvBwWide a, float *__restrict__ part, unsigned seg0, unsigned gl0) {
    typedef ConvBwGeo<KS, S> G;
    constexpr int RS = G::RS, NB = G::NB, TAPS = G::TAPS, NT = G::NT, LH = G::LH, LWS = G::LWS, LWH = G::LWH;
    constexpr int NDB = TR ? 4 : NB;
    static_assert(KS <= 3, "the bf16 domain");
    __shared__ __attribute__((aligned(16))) chb_b4 s_l[LH * S * LWH * 4];
    __shared__ __attribute__((aligned(16))) chb_b4 s_s[NB * RS * CB_C * 4];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int m = lane & 15, kq = lane >> 4;  // D: column m, rows 4 kq ..+3, as the float32 form
    const int Hs = a.b.H, Ws = a.b.W, HL = a.HL, WL = a.WL;
    const unsigned Cin = a.b.Cin, Cout = a.b.Cout;
    const int tiles = (TR ? Cin : Cout) / 16;
    const ch_b8 ones = ch_round(ch_f8{1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f});
    // a work item is (segment, group, pass), one a block, on k_convb_dw_wide's grid
    const unsigned pass = blockIdx.x, gl = gl0 + blockIdx.y, seg = seg0 + blockIdx.z;
    const unsigned sx = seg % (unsigned)a.b.segs_x, sy = seg / (unsigned)a.b.segs_x % (unsigned)a.b.segs_y;
    const unsigned fr = seg / (unsigned)a.b.segs_x / (unsigned)a.b.segs_y;
    const int h0 = sy * CB_R, v0 = sx * CB_C, n0 = pass * NB, nt = min(NB, tiles - n0);
    const int cols = min(CB_C, Ws - v0), steps = (cols + CHB_K - 1) / CHB_K, whole = cols / CHB_K;
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
        // ---- the strip of the large tensor's group under every tap, bf16, +0 outside its frame ----
        for (int e = t; e < LH * LWS * 4; e += 256) {
            const int p = e >> 2, s = e & 3;
            const int r = p / LWS, lc = p - r * LWS;
            const int h = S * h1 - G::P + r, v = S * v0 - G::P + lc;
            cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
            if (h >= 0 && h < HL && v >= 0 && v < WL) {
                const unsigned pixel = (unsigned)h * WL + v;
                f = TR ? convb_g4(b, pixel, 4 * s, VEC) : load_x(pixel, 4 * s);
            }
            s_l[((r * S + lc % S) * LWH + lc / S) * 4 + s] = chb_round(f);
        }
        // ---- the strip of the small tensor's nt tiles, [tile][pixel][16], bf16, +0 outside its frame ----
        for (int e = t; e < nt * RS * CB_C * 4; e += 256) {
            const int p = e >> 2, s = e & 3;  // p: (tile, row, column)
            const int n = p / (RS * CB_C), row = p / CB_C % RS, col = p % CB_C;
            const int h = h1 + row, v = v0 + col;
            cv_f4 f{0.0f, 0.0f, 0.0f, 0.0f};
            if (h < Hs && v < Ws) {
                const unsigned pixel = (unsigned)h * Ws + v;
                f = TR ? load_x(pixel, n * 16 + 4 * s) : convb_g4(b, pixel, n * 16 + 4 * s, VEC);
            }
            s_s[p * 4 + s] = chb_round(f);
        }
        __syncthreads();
        // ---- the strip's k-steps, rows in order, steps in order; EDGE: the row's last step where the frame ends inside it ----
        const int rows = min(RS, Hs - h1);
        auto k_step = [&](auto edge, int row, int s) {
            constexpr bool EDGE = decltype(edge)::value;
            const int left = Ws - v0 - CHB_K * s;  // (EDGE: 1 .. 31)
            const int at = (row * S * S * LWH + CHB_K * s) * 4;
            ch_b8 sv[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) sv[k] = chb_fragment(s_s, ((k * RS + row) * CB_C + CHB_K * s) * 4, lane);
#pragma unroll
            for (int n = 0; n < NT; ++n)
                if (wave + 4 * n < TAPS) {
                    const int tap = wave + 4 * n;
                    ch_b8 lv = chb_fragment(s_l, at + G::tap_offset(tap / KS, tap % KS) / 4, lane);
                    if (EDGE) lv = chb_inside(lv, left, lane);
#pragma unroll
                    for (int k = 0; k < NB; ++k)
                        acc[n][k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(TR ? sv[k] : lv, TR ? lv : sv[k], acc[n][k], 0, 0, 0);
                }
            if (wave == 3) {
#pragma unroll
                for (int k = 0; k < NDB; ++k) {
                    if (TR) {
                        ch_b8 lv = chb_fragment(s_l, at + G::tap_offset(k >> 1, k & 1) / 4, lane);
                        if (EDGE) lv = chb_inside(lv, left, lane);
                        accb[k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, lv, accb[k], 0, 0, 0);
                    } else {
                        accb[k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, sv[k], accb[k], 0, 0, 0);
                    }
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
    // ---- the segment's partials: [tap][Cin][Cout], then db: k_convb_dw_wide's ----
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

template <int KS, int S, bool TR>
void convhb_dw_wide_launch(hipStream_t st, const ConvBwWide &a, float *part, long long nseg) {
    const int groups = (TR ? a.b.Cout : a.b.Cin) / 16, tiles = (TR ? a.b.Cin : a.b.Cout) / 16;
    const int npass = (tiles + ConvBwGeo<KS, S>::NB - 1) / ConvBwGeo<KS, S>::NB;
    const bool vec = a.b.xvec && a.b.gvec;  // x, dy and y all allow 16-byte loads
    for (long long seg0 = 0; seg0 < nseg; seg0 += 65535)
        for (int gl0 = 0; gl0 < groups; gl0 += 65535) {
            const dim3 grid((unsigned)npass, (unsigned)min(groups - gl0, 65535), (unsigned)min(nseg - seg0, 65535ll));
            (vec ? k_convhb_dw_wide<KS, S, TR, true> : k_convhb_dw_wide<KS, S, TR, false>)<<<grid, 256, 0, st>>>(a, part, (unsigned)seg0,
                                                                                                                (unsigned)gl0);
        }
}

// ---- the host side: convb_data's and convb_weights' launches under ConvBwLayer::bf16 (dtfill.hip hands them in) ----
// dx: g, then the packed kernel, then dtfill_convb.hpp's case list on k_convh_wide
template <int = 0>
void convhb_data_launch(hipStream_t st, const ConvBwLayer &l, const ConvBwPlan &p, const ConvBwArgs &b, const float *w, float *dx,
                        int dx_channels, int dx_offset, float *dres, void *workspace) {
    char *ws = static_cast<char *>(workspace);
    float *g = reinterpret_cast<float *>(ws), *tmp = reinterpret_cast<float *>(ws + p.tmp);
    ch_b8 *wt = reinterpret_cast<ch_b8 *>(ws + p.wt);
    const long long total = (long long)l.B * p.Ho * p.Wo * l.Cout;
    const long long quads = convh_packed_quads(l.ksize, l.Cout, l.Cin);
    k_convb_g<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(b, g, dres, total);
    k_convhb_pack<><<<(unsigned)((quads + 255) / 256), 256, 0, st>>>(w, l.ksize * l.ksize, l.Cin, l.Cout, !l.transposed && l.stride == 1, wt,
                                                                    quads);
    ConvArgs a{g, reinterpret_cast<const float *>(wt), nullptr, nullptr, dx, l.B, p.Ho, p.Wo, l.Cout, l.Cin, l.H, l.W, 0, 0, dx_channels,
               dx_offset, DTFILL_CONV_LINEAR, 0.0f};
    if (l.transposed) {
        convh_strided_launch<>(st, a, 3, 2);  // [2H,2W] -> [H,W], pt = pl = 0
    } else if (l.stride == 2 && l.ksize == 3) {
        convh_transpose_launch<>(st, a);  // [H/2,W/2] -> [H,W]
    } else if (l.stride == 2) {
        a.out = tmp, a.Ho = p.Ho, a.Wo = p.Wo, a.out_channels = l.Cin, a.out_offset = 0;
        convh_strided_launch<>(st, a, 1, 1);
        const long long n = (long long)l.B * l.H * l.W * l.Cin;
        k_convb_spread<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, dx, l.H, l.W, l.Cin, dx_channels, dx_offset, n);
    } else {
        a.pt = a.pl = (l.ksize - 1) / 2;
        convh_strided_launch<>(st, a, l.ksize, 1);
    }
}

// dw and db: level 1 on the bf16 matrix cores into the segments' partials, then k_convb_sum
template <int = 0>
void convhb_weights_launch(hipStream_t st, const ConvBwLayer &l, const ConvBwWide &a, float *dw, float *db, void *workspace) {
    float *part = static_cast<float *>(workspace);
    const int nseg = l.B * a.b.segs_y * a.b.segs_x;
    const int ndw = l.ksize * l.ksize * l.Cin * l.Cout, pstride = ndw + l.Cout;
    if (l.transposed)
        convhb_dw_wide_launch<3, 2, true>(st, a, part, nseg);
    else if (l.stride == 2)
        (l.ksize == 1 ? convhb_dw_wide_launch<1, 2, false> : convhb_dw_wide_launch<3, 2, false>)(st, a, part, nseg);
    else
        (l.ksize == 1 ? convhb_dw_wide_launch<1, 1, false> : convhb_dw_wide_launch<3, 1, false>)(st, a, part, nseg);
    k_convb_sum<<<(pstride + 255) / 256, 256, 0, st>>>(part, pstride, nseg, ndw, dw, db);
}
