// dtfill_unproj.hpp -- back-projection: depth frames to ordered point clouds (get_all_points, and get_all_points ->
// calculate_angle -> sample, of subsample_Lidar_{train,val}.py), the inverse of dtfill_proj.hpp, and its backward pass
// (include/dtfill.h has the contract).  Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one
// translation unit).  The calibration record, the point, its pitch and the frame's range are dtfill_lines.hpp's statements.
#pragma once

// ------------------------------------------------------------------------------------------------
// Forward, four launches (five with keep_every >= 1); the launch boundaries are the only hand-offs between workgroups:
//   k_lines_calib     the inverses of K and E -> the frame record.
//   k_lines_range     keep mode only: the frame's pitch range, as partial slots.
//   k_unproj_count    one block per tile of LS_TILE pixels: how many of the tile's pixels are selected.
//   k_unproj_scan     one block per frame: the exclusive prefix sum of its tile counts, in place; counts and status.
//   k_unproj_write    one block per tile: selects again with the same code, places record k of the tile at
//                     frame base + tile base + k, k its rank in raster order.
// A lane holds UP_PER = 8 consecutive pixels of its tile, so the rank of a pixel is a prefix sum over lanes in lane order:
// placement is counts and prefix sums only, no atomics anywhere.  The selected pixels are compacted into an LDS list before any
// float64 work, so that a sparse frame computes on full waves; with keep_every == 0 the count launch is a popcount and the
// list is built once, in the write launch.  Records leave through an LDS stage of UP_CHUNK records as coalesced dwords, for
// either stride.
// Backward, four launches: k_lines_calib; k_unprojb_clear zeroes the gradients and the frame flags; k_unprojb_check validates
// counts and the pixel lists (integer OR into the flags); k_unprojb_scatter, one lane per record, stores each gradient at
// its pixel.  Zero-fill and validation are complete before the scatter starts: a bad frame stays all zero.
// ------------------------------------------------------------------------------------------------
constexpr int UP_CHUNK = 256;          // records staged per round of k_unproj_write
constexpr int UB_BLOCK = 8 * 256;      // records per block of the backward's check and scatter
static_assert(DTFILL_UNPROJ_NO_POINTS == DTFILL_LINES_NO_POINTS && DTFILL_UNPROJ_BAD_INTERVAL == DTFILL_LINES_BAD_INTERVAL &&
                  DTFILL_UNPROJ_SINGULAR == DTFILL_LINES_SINGULAR,
              "ls_frame_range's status is stored as it is");

struct UpLds {
    float x[LS_TILE];    // the tile as loaded
    float val[LS_TILE];  // the list: depth ...
    u16 idx[LS_TILE];    // ... and pixel within the tile, in raster order
    u8 keep[LS_TILE];    // keep mode: the label's verdict, by pixel within the tile
    int w[8];            // the waves' counts of two prefix sums
};

// The tile's pixels by coalesced loads through LDS; lane t then holds pixels 8 t .. 8 t + 7 of the tile.  Beyond the frame:
// NaN, valid under no threshold.
template <bool VEC>
__device__ __forceinline__ void up_load(const float *__restrict__ xf, int base, int HW, float *s_x, float (&v)[LS_PER]) {
    const int t = threadIdx.x;
    const float pad = __builtin_nanf("");
    if (VEC) {
#pragma unroll
        for (int q = 0; q < LS_PER / 4; ++q) {
            const int o = 4 * (t + 256 * q);
            *reinterpret_cast<float4 *>(s_x + o) =
                base + o < HW ? *reinterpret_cast<const float4 *>(xf + base + o) : make_float4(pad, pad, pad, pad);
        }
    } else {
#pragma unroll
        for (int j = 0; j < LS_PER; ++j) {
            const int o = t + 256 * j;
            s_x[o] = base + o < HW ? xf[base + o] : pad;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LS_PER / 4; ++q) {
        const float4 f = *reinterpret_cast<const float4 *>(s_x + LS_PER * t + 4 * q);
        v[4 * q] = f.x;
        v[4 * q + 1] = f.y;
        v[4 * q + 2] = f.z;
        v[4 * q + 3] = f.w;
    }
}

// The number of selected pixels in the lanes before this one, given the lane's own count c, and the block's total.  s_w: 4
// ints no other prefix sum of this tile uses.
__device__ __forceinline__ int up_rank(int c, int *s_w, int &total) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = s_w[k];
        before += k < w ? n : 0;
        total += n;
    }
    return before + incl - c;
}

// the lane's pixels of mask m to the list, from position pos on
__device__ __forceinline__ void up_list(unsigned m, const float (&v)[LS_PER], int pos, UpLds &s) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < LS_PER; ++j)
        if (m & (1u << j)) {
            s.idx[pos] = (u16)(LS_PER * t + j);
            s.val[pos] = v[j];
            ++pos;
        }
}

__device__ __forceinline__ unsigned up_valid(const float (&v)[LS_PER], float thr) {
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < LS_PER; ++j) m |= (v[j] > thr ? 1u : 0u) << j;
    return m;
}

// keep mode: what every block needs of its frame, worked out by its first wave from k_lines_range's partials
struct UpFrame {
    double lo, iv;
    int status;
};

__device__ __forceinline__ void up_frame(const double2 *__restrict__ part, int nb, int b, int n_bins,
                                         const double *__restrict__ rec, UpFrame *s_f) {
    if (threadIdx.x < 64) {
        double lo, iv;
        const int st = ls_frame_range(part, nb, b, n_bins, rec, lo, iv);
        if (threadIdx.x == 0) *s_f = UpFrame{lo, iv, st};
    }
    __syncthreads();
}

// The selected pixels of tile `tile` of frame b as the list s.idx / s.val[0, n), in raster order; returns n.  KEEP: the valid
// pixels are listed first, their labels decided on the list (k_lines_keep's expression), and the kept ones listed again.
template <bool VEC, bool KEEP>
__device__ __forceinline__ int up_select(const float *__restrict__ xf, int tile, int W, int HW, float thr, const double *c,
                                         const UpFrame &f, double ke, UpLds &s) {
    const int t = threadIdx.x, base = tile * LS_TILE;
    float v[LS_PER];
    up_load<VEC>(xf, base, HW, s.x, v);
    unsigned m = up_valid(v, thr);
    int n;
    int pos = up_rank(__popc(m), s.w, n);
    up_list(m, v, pos, s);
    __syncthreads();
    if (KEEP) {
#pragma unroll 1
        for (int k = t; k < n; k += 256) {
            const int loc = s.idx[k], i = base + loc;
            const int row = i / W;
            const double q = (ls_pitch(c, i - row * W, row, (double)s.val[k]) - f.lo) / f.iv;
            s.keep[loc] = fmod(ceil(q), ke) == 0.0 ? 1 : 0;  // the label is not clamped
        }
        __syncthreads();
        unsigned m2 = 0;
#pragma unroll
        for (int j = 0; j < LS_PER; ++j)
            if ((m & (1u << j)) && s.keep[LS_PER * t + j]) m2 |= 1u << j;
        pos = up_rank(__popc(m2), s.w + 4, n);  // (its barrier: every lane has read the list's verdicts)
        up_list(m2, v, pos, s);
        __syncthreads();
    }
    return n;
}

// tile blockIdx.x of frame blockIdx.y: its number of selected pixels -> tcnt[b * T + tile].  Without KEEP a singular frame's
// valid pixels are counted too: k_unproj_scan tells an empty frame by them.
template <bool VEC, bool KEEP>
__global__ __launch_bounds__(256) void k_unproj_count(const float *__restrict__ x, int W, int HW, float thr, int n_bins,
                                                      int keep_every, const double *__restrict__ rec,
                                                      const double2 *__restrict__ part, int nb, int *__restrict__ tcnt) {
    __shared__ UpLds s;
    __shared__ UpFrame s_f;
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    const float *xf = x + (size_t)b * HW;
    int n = 0;
    if (KEEP) {
        up_frame(part, nb, b, n_bins, rec, &s_f);
        const UpFrame f = s_f;
        if (f.status == 0) {
            double c[LS_SING];
#pragma unroll
            for (int k = 0; k < LS_SING; ++k) c[k] = rec[(size_t)b * LS_REC + k];
            n = up_select<VEC, true>(xf, tile, W, HW, thr, c, f, (double)keep_every, s);
        }
    } else {
        float v[LS_PER];
        up_load<VEC>(xf, tile * LS_TILE, HW, s.x, v);
        up_rank(__popc(up_valid(v, thr)), s.w, n);
    }
    if (t == 0) tcnt[(size_t)b * gridDim.x + tile] = n;
}

// frame blockIdx.x: tcnt[b * T ..+T) becomes its exclusive prefix sum; the frame's counts and status
template <bool KEEP>
__global__ __launch_bounds__(256) void k_unproj_scan(int *__restrict__ tcnt, int T, int N, int n_bins,
                                                     const double *__restrict__ rec, const double2 *__restrict__ part, int nb,
                                                     int32_t *__restrict__ counts, int32_t *__restrict__ frame_status) {
    __shared__ int s_w[8];
    __shared__ UpFrame s_f;
    const int t = threadIdx.x, b = blockIdx.x;
    int *tc = tcnt + (size_t)b * T;
    int carry = 0;
    for (int c0 = 0; c0 < T; c0 += 256) {
        const int i = c0 + t;
        const int v = i < T ? tc[i] : 0;
        int tot;
        const int before = up_rank(v, s_w + ((c0 >> 8) & 1) * 4, tot);  // (alternating slots: one barrier a round is enough)
        if (i < T) tc[i] = carry + before;
        carry += tot;
    }
    int st;
    if (KEEP) {
        up_frame(part, nb, b, n_bins, rec, &s_f);
        st = s_f.status;  // (a frame with a status bit counted nothing)
    } else {
        const bool sing = rec[(size_t)b * LS_REC + LS_SING] != 0.0;
        st = (carry == 0 ? DTFILL_UNPROJ_NO_POINTS : 0) | (sing ? DTFILL_UNPROJ_SINGULAR : 0);
        if (sing) carry = 0;
    }
    if (t == 0) {
        if (carry > N) st |= DTFILL_UNPROJ_OVERFLOW;
        counts[2 * b + DTFILL_UNPROJ_WRITTEN] = min(carry, N);
        counts[2 * b + DTFILL_UNPROJ_TOTAL] = carry;
        if (frame_status) frame_status[b] = st;
    }
}

// tile blockIdx.x of frame blockIdx.y: its records, pitches and pixels, as far as they lie below N
template <bool VEC, bool KEEP>
__global__ __launch_bounds__(256) void k_unproj_write(const float *__restrict__ x, const float *__restrict__ payload, int W, int HW,
                                                      float thr, int n_bins, int keep_every, const double *__restrict__ rec,
                                                      const double2 *__restrict__ part, int nb, const int *__restrict__ tcnt,
                                                      int N, int stride, float *__restrict__ points, double *__restrict__ pitch,
                                                      int32_t *__restrict__ pixel) {
    __shared__ UpLds s;
    __shared__ UpFrame s_f;
    __shared__ float s_rec[UP_CHUNK * 4];
    const int t = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    const int tb = tcnt[(size_t)b * gridDim.x + tile];
    if (tb >= N) return;  // (block-uniform, before any barrier)
    if (rec[(size_t)b * LS_REC + LS_SING] != 0.0) return;
    UpFrame f{0.0, 0.0, 0};
    if (KEEP) {
        up_frame(part, nb, b, n_bins, rec, &s_f);
        f = s_f;
        if (f.status != 0) return;
    }
    double c[LS_SING];  // the frame record: uniform loads, held in SGPRs
#pragma unroll
    for (int k = 0; k < LS_SING; ++k) c[k] = rec[(size_t)b * LS_REC + k];
    const float *xf = x + (size_t)b * HW;
    const int base = tile * LS_TILE;
    const int n = min(up_select<VEC, KEEP>(xf, tile, W, HW, thr, c, f, (double)keep_every, s), N - tb);
    const size_t first = (size_t)b * N + tb;  // the tile's first record
    for (int c0 = 0; c0 < n; c0 += UP_CHUNK) {
        const int k = c0 + t, cnt = min(UP_CHUNK, n - c0);
        if (k < n) {
            const int i = base + s.idx[k];
            const int row = i / W;
            double px, py, pz;
            ls_point(c, i - row * W, row, (double)s.val[k], px, py, pz);
            s_rec[t * stride] = (float)px;
            s_rec[t * stride + 1] = (float)py;
            s_rec[t * stride + 2] = (float)pz;
            if (stride == 4) s_rec[t * 4 + 3] = payload ? payload[(size_t)b * HW + i] : 0.0f;
            if (pitch) pitch[first + k] = ls_point_pitch(px, py, pz);
            if (pixel) pixel[first + k] = i;
        }
        __syncthreads();
        float *dst = points + (first + c0) * stride;
        for (int j = t; j < cnt * stride; j += 256) dst[j] = s_rec[j];
        __syncthreads();  // the stage is rewritten by the next round
    }
}

// ---- backward ----
// frame b's record count: counts[b].WRITTEN, -1 outside [0, N]
__device__ __forceinline__ int ub_count(const int32_t *__restrict__ counts, int b, int N) {
    const int n = counts[2 * b + DTFILL_UNPROJ_WRITTEN];
    return n < 0 || n > N ? -1 : n;
}

__global__ __launch_bounds__(256) void k_unprojb_clear(float *__restrict__ gx, float *__restrict__ gp, size_t n,
                                                       int *__restrict__ flags, int B) {
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 < (size_t)B) flags[i0] = 0;
    for (size_t i = i0; i < n; i += (size_t)gridDim.x * 256) {
        gx[i] = 0.0f;
        if (gp) gp[i] = 0.0f;
    }
}

// records [blockIdx.x * UB_BLOCK, +UB_BLOCK) of frame blockIdx.y: each pixel inside the frame and above its predecessor
__global__ __launch_bounds__(256) void k_unprojb_check(const int32_t *__restrict__ pixel, const int32_t *__restrict__ counts,
                                                       int N, int HW, int *__restrict__ flags) {
    const int t = threadIdx.x, b = blockIdx.y;
    const int nb = ub_count(counts, b, N);
    if (nb < 0) {
        if (blockIdx.x == 0 && t == 0) atomicOr(flags + b, DTFILL_UNPROJ_BAD_COUNT);
        return;
    }
    const int first = blockIdx.x * UB_BLOCK, last = min(nb, first + UB_BLOCK);
    const int32_t *p = pixel + (size_t)b * N;
    bool bad = false;
    for (int i = first + t; i < last; i += 256) {
        const int cur = p[i], prev = i > 0 ? p[i - 1] : -1;
        bad |= cur < 0 || cur >= HW || prev >= cur;
    }
    if (bad) atomicOr(flags + b, DTFILL_UNPROJ_BAD_PIXEL);
}

// records [blockIdx.x * UB_BLOCK, +UB_BLOCK) of frame blockIdx.y, 256 at a time: one lane per record
__global__ __launch_bounds__(256) void k_unprojb_scatter(const float *__restrict__ gpts, const int32_t *__restrict__ pixel,
                                                         const int32_t *__restrict__ counts, int N, int stride, int W, int HW,
                                                         const double *__restrict__ rec, const int *__restrict__ flags,
                                                         float *__restrict__ gx, float *__restrict__ gp,
                                                         int32_t *__restrict__ frame_status) {
#pragma clang fp contract(off)
    __shared__ float s_rec[256 * 4];
    const int t = threadIdx.x, b = blockIdx.y;
    const bool sing = rec[(size_t)b * LS_REC + LS_SING] != 0.0;
    const int flag = flags[b];
    if (blockIdx.x == 0 && t == 0 && frame_status) frame_status[b] = flag | (sing ? DTFILL_UNPROJ_SINGULAR : 0);
    if (flag || sing) return;
    const int nb = ub_count(counts, b, N);  // (in range: the flag is clear)
    const int first = blockIdx.x * UB_BLOCK, last = min(nb, first + UB_BLOCK);
    if (first >= last) return;
    double c[LS_SING];
#pragma unroll
    for (int k = 0; k < LS_SING; ++k) c[k] = rec[(size_t)b * LS_REC + k];
    for (int r0 = first; r0 < last; r0 += 256) {
        const int cnt = min(256, last - r0);
        const float *src = gpts + ((size_t)b * N + r0) * stride;
        for (int j = t; j < cnt * stride; j += 256) s_rec[j] = src[j];
        __syncthreads();
        if (t < cnt) {
            const int i = pixel[(size_t)b * N + r0 + t];
            const int row = i / W;
            const double du = (double)(i - row * W), dv = (double)row;
            const double k0 = c[0] * du + c[1] * dv + c[2];
            const double k1 = c[3] * du + c[4] * dv + c[5];
            const double k2 = c[6] * du + c[7] * dv + c[8];
            const double j0 = c[9] * k0 + c[10] * k1 + c[11] * k2;
            const double j1 = c[13] * k0 + c[14] * k1 + c[15] * k2;
            const double j2 = c[17] * k0 + c[18] * k1 + c[19] * k2;
            const double gX = (double)s_rec[t * stride], gY = (double)s_rec[t * stride + 1], gZ = (double)s_rec[t * stride + 2];
            gx[(size_t)b * HW + i] = (float)(gX * j0 + gY * j1 + gZ * j2);
            if (gp && stride == 4) gp[(size_t)b * HW + i] = s_rec[t * 4 + 3];
        }
        __syncthreads();  // the stage is rewritten by the next round
    }
}

// the tiles of a frame, and the pieces of the forward's workspace: the frame records, k_lines_range's partials, the tile counts
struct UpWs {
    double *rec;
    double2 *part;
    int *tcnt;
};
inline int up_tiles(int H, int W) { return (int)(((long long)H * W + LS_TILE - 1) / LS_TILE); }

template <bool VEC, bool KEEP>
void unproj_launch(hipStream_t st, const float *x, const float *payload, int B, int H, int W, float thr, const double *K,
                   const double *E, int n_bins, int keep_every, int N, int stride, float *points, double *pitch, int32_t *pixel,
                   int32_t *counts, int32_t *frame_status, const UpWs &ws, int tpb, int nb) {
    const int HW = H * W, T = up_tiles(H, W);
    const dim3 tiles(T, B);
    k_lines_calib<<<B, 64, 0, st>>>(K, E, ws.rec);
    if (KEEP) k_lines_range<VEC><<<dim3(nb, B), 256, 0, st>>>(x, thr, W, HW, tpb, ws.rec, ws.part);
    k_unproj_count<VEC, KEEP><<<tiles, 256, 0, st>>>(x, W, HW, thr, n_bins, keep_every, ws.rec, ws.part, nb, ws.tcnt);
    k_unproj_scan<KEEP><<<B, 256, 0, st>>>(ws.tcnt, T, N, n_bins, ws.rec, ws.part, nb, counts, frame_status);
    k_unproj_write<VEC, KEEP><<<tiles, 256, 0, st>>>(x, payload, W, HW, thr, n_bins, keep_every, ws.rec, ws.part, nb, ws.tcnt, N,
                                                     stride, points, pitch, pixel);
}
