// dtfill_nyu.hpp -- the per-sample work of the reference's NYU loaders (data_read.py:278-371 and its two copies): the
// anti-aliased resize of the stored image and depth (a Gaussian pre-filter, then a linear resample), the loader's * 255, the
// drivers' / 255, and the sparse sampling gt * Mask (include/dtfill.h has the contract, dtfill_nyu_read).
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit), after dtfill_rgb.hpp.
#pragma once

// ------------------------------------------------------------------------------------------------
// Launches:
//   k_nyu_clear   zeroes the per-frame bit masks in the workspace (one bit per output pixel) and frame_status.
//   k_nyu_mark    one thread per sample: sets the pixel's bit, or the frame's DTFILL_NYU_INDEX_ERROR bit for a sample outside.
//   k_nyu_tile<T, R>  T = u8 (the image, every channel of a tile in one block) or float (the depth); R = NY_FAST_R: both
//                 radii known at compile time, else -1: from the arguments.  A block takes tiles of
//                 th x tw output pixels (16 x 32 unless the factor is so large that the tile's source does not fit NY_LDS).
//                 Per tile, once: TABLES  for each of the 2 th filtered rows and 2 tw filtered columns the resample samples
//                             (m(i0), m(i0 + 1) of each output row / column) the places of its 2 r + 1 mirrored taps in the
//                             staged range, and the resample's weight of every output row and column: the mirror's modulo
//                             and the coordinate's floor are paid per tile, not per tap.
//                 Per tile and channel, everything in LDS:
//                   STAGE     the source rows and columns the tile's taps reach, as stored (u8 / float): at most
//                             ceil((tile - 1) f) + 2 r + 5 per axis, the mirrored indices included; nothing else is read.
//                   VERTICAL  for the 2 th filtered rows the resample samples (rows m(i0), m(i0 + 1) of each output row; a
//                             filtered row no output row samples is not computed) and every staged column: the axis-0 pass.
//                   HORIZONTAL for those rows and the 2 tw filtered columns the resample samples: the axis-1 pass.
//                   RESAMPLE  one thread per output pixel: its 2 x 2 filtered samples are adjacent in sH, the two of a row
//                             one 16-byte read; the four products; the epilogue.
//                 NHWC image rows leave through an LDS image of the tile so that a row's tw * C floats are stored in order.
// The float64 arithmetic is plain operators under `#pragma clang fp contract(off)` in every function that holds any (hipcc
// contracts a * b + c into an FMA by default, and HIP's __dmul_rn / __dadd_rn are plain operators that do not stop it:
// dtfill_post.hpp).  An FMA anywhere in a pass or in the coordinate (j + 0.5) f - 0.5 changes the bits.
// LDS banks: the passes read and write consecutive elements in consecutive lanes (the staged image and sV along a row; sH's
// slots of neighbouring outputs are neighbours), and the resample reads 16 bytes a lane: a lane-per-double read of every
// second double would use half the banks of a double-wide row.
// ------------------------------------------------------------------------------------------------
constexpr int NY_THREADS = 256;
constexpr int NY_TH = 16, NY_TW = 32;  // the tile, unless it has to shrink (ny_pick_tile)
constexpr int NY_LDS = 64 << 10;       // dynamic LDS a block may take: two blocks or more per CU
constexpr int NY_MAX_BLOCKS = 1 << 20; // blocks along grid x; a block strides over the tiles beyond
constexpr int NY_FAST_R = 2;           // both radii 2 (factors 1.75 to 2.25: both NYU geometries): the tap loops unrolled

struct NyAxis {
    double f;                           // n_in / n_out
    double w[DTFILL_NYU_MAX_RADIUS + 1];  // the half kernel, w[0] the centre
    int n_in, n_out, r, tile, ext;      // ext: the most source rows / columns a tile stages (host: ny_ext_bound)
};

struct NyArgs {
    const void *src;  // u8 [B, C, hin, win] or float [B, hin, win]
    NyAxis y, x;
    int C, normalize, layout, tiles_x;
    long long ntiles;
    const u32 *mask;  // [B, words], nullable: no sample
    size_t words;
    float *out_rgb, *out_gt, *out_lidar;
};

// scipy's 'mirror': period 2 (n - 1), the edge sample not repeated, any number of reflections
__device__ __forceinline__ int ny_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i = (i < 0 ? -i : i) % p;
    return i >= n ? p - i : i;
}

// output index j -> i0 = floor(c), t = c - i0, c = (j + 0.5) f - 0.5
__device__ __forceinline__ void ny_coord(int j, double f, int &i0, double &t) {
#pragma clang fp contract(off)
    const double h = (double)j + 0.5;
    const double p = h * f;
    const double c = p - 0.5;
    const double fl = floor(c);
    i0 = (int)fl;
    t = c - fl;
}

struct NyRange { int lo, n; };

// The source indices [lo, lo + n) that outputs [j0, j1) of an axis reach: resample neighbours a = i0(j0) .. b = i0(j1 - 1) + 1,
// r taps either side, and where that leaves [0, n_in) its mirror image (all of [0, n_in) once it reflects more than once).
__device__ __forceinline__ NyRange ny_range(int j0, int j1, const NyAxis &ax) {
    int a, b;
    double t;
    ny_coord(j0, ax.f, a, t);
    ny_coord(j1 - 1, ax.f, b, t);
    const int last = ax.n_in - 1, lo_u = a - ax.r, hi_u = b + 1 + ax.r;
    int lo = max(lo_u, 0), hi = min(hi_u, last);
    if (lo_u < 0) hi = max(hi, min(last, -lo_u));
    if (hi_u > last) lo = min(lo, max(0, 2 * last - hi_u));
    return NyRange{lo, min(hi - lo + 1, ax.ext)};
}

__device__ __forceinline__ double ny_load(const u8 *p) {
#pragma clang fp contract(off)
    const double v = (double)*p;
    return v * (1.0 / 255.0);  // img_as_float's multiply by the reciprocal
}
__device__ __forceinline__ double ny_load(const float *p) { return (double)*p; }
__device__ __forceinline__ double ny_load(const double *p) { return *p; }

// source index k of an axis -> its place in the staged range (the clamp never binds: ny_range)
__device__ __forceinline__ int ny_at(int k, int n_in, NyRange rg) { return min(max(ny_mirror(k, n_in) - rg.lo, 0), rg.n - 1); }

// One output of a filter pass: the centre, then the pairs from the outermost inwards (scipy's correlate1d for symmetric
// weights), accumulated in double; rounded to float where the array is float32 (F32).  tab[r + k], k = -r .. r: the places of
// the output's taps m(i + k) in the staged range (the tile's table: no mirror, no coordinate in this loop).  R >= 0: the radius at
// compile time (NY_FAST_R: the loop unrolls, the reads of all taps are in flight together); R < 0: ax.r.
template <bool F32, int R, typename S>
__device__ __forceinline__ double ny_pass(const S *base, int stride, const int *tab, const NyAxis &ax) {
#pragma clang fp contract(off)
    const int r = R >= 0 ? R : ax.r;
    const double x0 = ny_load(base + tab[r] * stride);
    if (r == 0) return x0;
    double acc = x0 * ax.w[0];
#pragma unroll
    for (int k = r; k >= 1; --k) {
        const double lo = ny_load(base + tab[r - k] * stride);
        const double hi = ny_load(base + tab[r + k] * stride);
        const double s = lo + hi;
        const double p = s * ax.w[k];
        acc = acc + p;
    }
    return F32 ? (double)(float)acc : acc;
}

// The tap table of one axis for outputs [j_beg, j_beg + n): row q = 2 lj + d is filtered index m(i0(lj) + d), entry r + k its
// tap m(. + k) as a place in the staged range rg.  The resample's weight t of every output goes to `wt`.
__device__ __forceinline__ void ny_fill_tab(int *tab, double *wt, int j_beg, int n, NyRange rg, const NyAxis &ax, int tid) {
    const int K = 2 * ax.r + 1;
    for (int e = tid; e < 2 * n * K; e += NY_THREADS) {
        const int q = e / K, k = e - q * K - ax.r;
        int i0;
        double t;
        ny_coord(j_beg + (q >> 1), ax.f, i0, t);
        tab[e] = ny_at(ny_mirror(i0 + (q & 1), ax.n_in) + k, ax.n_in, rg);
        if (k == 0 && !(q & 1)) wt[q >> 1] = t;
    }
}

// scipy's zoom(order=1): from 0.0 on, each sample times its row weight times its column weight, 00, 01, 10, 11
__device__ __forceinline__ double ny_bilinear(double x00, double x01, double x10, double x11, double tr, double tc) {
#pragma clang fp contract(off)
    const double ur = 1.0 - tr, uc = 1.0 - tc;
    double p = x00 * ur;
    p = p * uc;
    double t = 0.0 + p;
    p = x01 * ur;
    p = p * tc;
    t = t + p;
    p = x10 * tr;
    p = p * uc;
    t = t + p;
    p = x11 * tr;
    p = p * tc;
    t = t + p;
    return t;
}

// the loader's float32(r * 255) and, with normalize, the drivers' float32(float64(that) / 255.0)
__device__ __forceinline__ float ny_rgb_value(double r, bool normalize) {
#pragma clang fp contract(off)
    const float o = (float)(r * 255.0);
    return normalize ? (float)((double)o / 255.0) : o;
}

__global__ __launch_bounds__(256) void k_nyu_clear(u32 *__restrict__ mask, size_t nwords, int32_t *__restrict__ frame_status, int B) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nwords) mask[i] = 0;
    if (frame_status && i < (size_t)B) frame_status[i] = 0;
}

__global__ __launch_bounds__(256) void k_nyu_mark(const int32_t *__restrict__ samples, int B, int n, int H, int W, size_t words,
                                                  u32 *__restrict__ mask, int32_t *__restrict__ frame_status) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= (size_t)B * n) return;
    const int b = (int)(s / n), r = samples[2 * s], c = samples[2 * s + 1];
    if (r >= 0 && r < H && c >= 0 && c < W) {
        const size_t p = (size_t)r * W + c;
        atomicOr(&mask[b * words + (p >> 5)], 1u << (p & 31));
    } else if (frame_status) {
        atomicOr(&frame_status[b], DTFILL_NYU_INDEX_ERROR);
    }
}

template <typename T, int R>
__global__ __launch_bounds__(NY_THREADS) void k_nyu_tile(const NyArgs a) {
    constexpr bool RGB = std::is_same<T, u8>::value;
    extern __shared__ __attribute__((aligned(16))) unsigned char ny_lds[];
    const int th = a.y.tile, tw = a.x.tile, eW = a.x.ext;  // (sIn's a.y.ext rows are the last piece)
    const int hin = a.y.n_in, win = a.x.n_in, H = a.y.n_out, W = a.x.n_out, C = a.C;
    const int KY = 2 * a.y.r + 1, KX = 2 * a.x.r + 1;
    double *sV = reinterpret_cast<double *>(ny_lds);         // [2 th][eW]    axis 0 filtered, the sampled rows
    double *sH = sV + 2 * th * eW;                           // [2 th][2 tw]  both axes filtered, the sampled rows and columns
    double *sTr = sH + 4 * th * tw, *sTc = sTr + th;         // [th], [tw]    the resample's weights
    float *sOut = reinterpret_cast<float *>(sTc + tw);       // [th][tw * C]  the NHWC image of the tile (RGB only)
    int *tabY = reinterpret_cast<int *>(sOut + (RGB ? th * tw * C : 0));  // [2 th][KY], [2 tw][KX]: ny_fill_tab
    int *tabX = tabY + 2 * th * KY;
    T *sIn = reinterpret_cast<T *>(tabX + 2 * tw * KX);      // [eH][eW]      the staged source
    const int b = blockIdx.y, tid = threadIdx.x;
    const bool nhwc = RGB && a.layout == DTFILL_RGB_NHWC && C > 1;
    const T *src = static_cast<const T *>(a.src) + (size_t)b * C * hin * win;
    const u32 *maskb = a.mask ? a.mask + b * a.words : nullptr;
    for (long long t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int ty = (int)(t / a.tiles_x), tx = (int)(t - (long long)ty * a.tiles_x);
        const int i_beg = ty * th, nh = min(H - i_beg, th), j_beg = tx * tw, nw = min(W - j_beg, tw);
        const NyRange ry = ny_range(i_beg, i_beg + nh, a.y), rx = ny_range(j_beg, j_beg + nw, a.x);
        __syncthreads();  // the tile before has read the tables, the weights and sOut
        ny_fill_tab(tabY, sTr, i_beg, nh, ry, a.y, tid);
        ny_fill_tab(tabX, sTc, j_beg, nw, rx, a.x, tid);
        for (int c = 0; c < C; ++c) {
            const T *plane = src + (size_t)c * hin * win;
            // (no barrier here: two lie between the last reader of sIn, sV or sH in the channel before and its next writer)
            for (int e = tid; e < ry.n * rx.n; e += NY_THREADS) {
                const int yy = e / rx.n, xx = e - yy * rx.n;
                sIn[yy * eW + xx] = plane[(size_t)(ry.lo + yy) * win + (rx.lo + xx)];
            }
            __syncthreads();  // (the first channel's: the tables too)
            for (int e = tid; e < 2 * nh * rx.n; e += NY_THREADS) {
                const int s = e / rx.n, xx = e - s * rx.n;
                sV[s * eW + xx] = ny_pass<!RGB, R>(sIn + xx, eW, tabY + s * KY, a.y);
            }
            __syncthreads();
            for (int e = tid; e < 4 * nh * nw; e += NY_THREADS) {
                const int s = e / (2 * nw), q = e - s * (2 * nw);
                sH[s * 2 * tw + q] = ny_pass<!RGB, R>(sV + s * eW, 1, tabX + q * KX, a.x);
            }
            __syncthreads();
            for (int e = tid; e < nh * nw; e += NY_THREADS) {
                const int li = e / nw, lj = e - li * nw;
                const double tr = sTr[li], tc = sTc[lj];
                const double2 top = *reinterpret_cast<const double2 *>(sH + (2 * li) * 2 * tw + 2 * lj);
                const double2 bot = *reinterpret_cast<const double2 *>(sH + (2 * li + 1) * 2 * tw + 2 * lj);
                const double v = ny_bilinear(top.x, top.y, bot.x, bot.y, tr, tc);
                const size_t p = (size_t)(i_beg + li) * W + (j_beg + lj);  // the pixel in its frame
                if (RGB) {
                    const float o = ny_rgb_value(v, a.normalize != 0);
                    if (nhwc)
                        sOut[(li * tw + lj) * C + c] = o;
                    else
                        a.out_rgb[((size_t)b * C + c) * H * W + p] = o;  // (C == 1: both layouts)
                } else {
                    const float gt = (float)v;
                    const size_t o = (size_t)b * H * W + p;
                    if (a.out_gt) a.out_gt[o] = gt;
                    if (a.out_lidar) {
                        const bool marked = maskb && (maskb[p >> 5] >> (p & 31) & 1u);
                        a.out_lidar[o] = marked ? gt : gt * 0.0f;  // the product as it stands: -0.0 and NaN as gt * Mask gives them
                    }
                }
            }
        }
        if (nhwc) {
            __syncthreads();
            for (int e = tid; e < nh * nw * C; e += NY_THREADS) {
                const int li = e / (nw * C), k = e - li * (nw * C);
                a.out_rgb[(((size_t)b * H + (i_beg + li)) * W + j_beg) * C + k] = sOut[li * tw * C + k];
            }
        }
    }
}

// the most source indices of an axis a tile of `tile` outputs stages (ny_range: ceil((tile - 1) f) + 1 between the first
// and last resample neighbour, r either side, one more where the last neighbour mirrors, one for the rounding of the ceil)
inline int ny_ext_bound(int tile, double f, int r, int n_in) {
    const double e = ceil((tile - 1) * f) + 2.0 * r + 5.0;
    return e < (double)n_in ? (int)e : n_in;
}

// k_nyu_tile's pieces in its order: sV, sH, sTr, sTc; sOut (RGB); tabY, tabX; sIn
inline size_t ny_lds_bytes(const NyAxis &y, const NyAxis &x, int C, bool rgb) {
    return sizeof(double) * ((size_t)2 * y.tile * x.ext + (size_t)4 * y.tile * x.tile + y.tile + x.tile) +
           (rgb ? sizeof(float) * (size_t)y.tile * x.tile * C : 0) +
           sizeof(int) * ((size_t)2 * y.tile * (2 * y.r + 1) + (size_t)2 * x.tile * (2 * x.r + 1)) +
           (rgb ? sizeof(u8) : sizeof(float)) * (size_t)y.ext * x.ext;
}

// The largest tile whose LDS fits NY_LDS: 16 x 32, then halved (the wider side first) for factors that large; 1 x 1 always
// fits (at most 2 r + 5 <= 21 rows and columns, two tables of 34 entries).
inline size_t ny_pick_tile(NyAxis &y, NyAxis &x, int C, bool rgb) {
    y.tile = NY_TH;
    x.tile = NY_TW;
    for (;;) {
        y.ext = ny_ext_bound(y.tile, y.f, y.r, y.n_in);
        x.ext = ny_ext_bound(x.tile, x.f, x.r, x.n_in);
        const size_t bytes = ny_lds_bytes(y, x, C, rgb);
        if (bytes <= (size_t)NY_LDS || (y.tile == 1 && x.tile == 1)) return bytes;
        if (x.tile > y.tile || y.tile == 1)
            x.tile >>= 1;
        else
            y.tile >>= 1;
    }
}

template <typename T>
void nyu_launch(hipStream_t st, NyArgs a, int B) {
    constexpr bool RGB = std::is_same<T, u8>::value;
    const size_t lds = ny_pick_tile(a.y, a.x, a.C, RGB);
    a.tiles_x = (a.x.n_out + a.x.tile - 1) / a.x.tile;
    a.ntiles = (long long)a.tiles_x * ((a.y.n_out + a.y.tile - 1) / a.y.tile);
    const dim3 grid((unsigned)(a.ntiles < NY_MAX_BLOCKS ? a.ntiles : NY_MAX_BLOCKS), B);
    if (a.y.r == NY_FAST_R && a.x.r == NY_FAST_R)
        k_nyu_tile<T, NY_FAST_R><<<grid, NY_THREADS, lds, st>>>(a);
    else
        k_nyu_tile<T, -1><<<grid, NY_THREADS, lds, st>>>(a);
}
