// dtfill_lines.hpp -- scan-line subsampling of a projected LiDAR frame (the 64 -> 32 / 16 line inputs of
// subsample_Lidar_{train,val}.py): back-project every valid pixel through K^-1 and E^-1, bin the frame's pitch range into
// n_bins equal bins, keep a pixel iff its bin label is a multiple of keep_every (include/dtfill.h has the contract).
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// Three launches, because every label depends on the frame's pitch minimum and maximum:
//   k_lines_calib  one wave per frame: the inverses of K and E (float64, partial pivoting, in registers) -> the frame record.
//   k_lines_range  per block: the pitch of every valid pixel of its tiles, and its (min, max) -> partial slot in the
//                  workspace.
//   k_lines_keep   per block: reduces its frame's partials, then recomputes the pitch of every valid pixel of its tiles with
//                  the same code, decides the label, and stores every pixel of the tiles (input value or +0.0f).
// The launch boundaries are the only hand-offs between workgroups: no flags, no atomics on global memory, nothing to
// initialise per call.  (Inverting in every block of k_lines_range, one lane on an LDS scratch, cost 54 us instead of the
// launch's streaming time: every block waited for the serial chain before its first pitch.)  Min and max are exact, so the result does not depend on the order of anything.
// A tile is LS_TILE contiguous pixels of a frame, LS_PER per lane.  The valid pixels of a tile are compacted into LDS first,
// so that the float64 work (about a hundred operations and an asin per pixel) runs on full waves even in a frame with a few
// percent of valid pixels.
// ------------------------------------------------------------------------------------------------
constexpr int LS_PER = 8, LS_TILE = 256 * LS_PER;
constexpr int LS_MAXNB = 128;  // blocks (and partial slots) per frame at most
constexpr int LS_REC = 32;     // doubles per frame record: K^-1 (9), rows 0..2 of E^-1 (12), singular flag
constexpr int LS_SING = 21;

// NaN-propagating min / max: numpy's np.min / np.max of a frame with a NaN pitch is NaN
__device__ __forceinline__ double ls_min(double a, double b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ double ls_max(double a, double b) { return (a > b || a != a) ? a : b; }

// Gauss-Jordan inverse with partial pivoting of the N x N row-major matrix at m, in float64, in one lane's registers (every
// index a constant: the row swap is a select per row).  Rows 0..ROWS-1 of the inverse go to inv (row-major).  false on an
// exactly zero pivot (np.linalg.inv: LinAlgError); the inverse is then meaningless.
template <int N, int ROWS>
__device__ __forceinline__ bool ls_invert(const double *__restrict__ m, double *__restrict__ inv) {
    double a[N][2 * N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < 2 * N; ++j) a[i][j] = j < N ? m[i * N + j] : (j - N == i ? 1.0 : 0.0);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        double best = fabs(a[k][k]);
#pragma unroll
        for (int r = k + 1; r < N; ++r)
            if (fabs(a[r][k]) > best) {
                best = fabs(a[r][k]);
                p = r;
            }
        ok &= best != 0.0;
#pragma unroll
        for (int r = k + 1; r < N; ++r)
            if (r == p)
#pragma unroll
                for (int j = 0; j < 2 * N; ++j) {
                    const double t = a[k][j];
                    a[k][j] = a[r][j];
                    a[r][j] = t;
                }
        const double piv = a[k][k];
#pragma unroll
        for (int j = 0; j < 2 * N; ++j) a[k][j] /= piv;
#pragma unroll
        for (int r = 0; r < N; ++r)
            if (r != k) {
                const double f = a[r][k];
#pragma unroll
                for (int j = 0; j < 2 * N; ++j) a[r][j] -= f * a[k][j];
            }
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) inv[i * N + j] = a[i][N + j];
    return ok;
}

// k_lines_calib: frame blockIdx.x's record: lane 0 inverts K, lane 1 E (rows 0..2), lane 2 writes the singular flag
__global__ __launch_bounds__(64) void k_lines_calib(const double *__restrict__ K, const double *__restrict__ E,
                                                    double *__restrict__ rec) {
    __shared__ int s_ok[2];
    const int t = threadIdx.x, b = blockIdx.x;
    double *r = rec + (size_t)b * LS_REC;
    if (t == 0) s_ok[0] = ls_invert<3, 3>(K + (size_t)b * 9, r);
    if (t == 1) s_ok[1] = ls_invert<4, 3>(E + (size_t)b * 16, r + 9);
    __syncthreads();
    if (t == 2) r[LS_SING] = s_ok[0] && s_ok[1] ? 0.0 : 1.0;
}

// The point of pixel (row v, column u) at depth d: p_cam = K^-1 [u v 1]^T d, p = (E^-1 [p_cam; 1])[0:3], and its pitch
// asin(p.z / |p|).  c: the frame record.  Every operation rounded on its own (no contraction), in the order the contract
// writes them, so that every launch (the range, the labels, dtfill_unproject's records) computes the same bits for the same
// pixel.
__device__ __forceinline__ void ls_point(const double *c, int u, int v, double d, double &px, double &py, double &pz) {
#pragma clang fp contract(off)
    const double du = (double)u, dv = (double)v;
    const double cx = (c[0] * du + c[1] * dv + c[2]) * d;
    const double cy = (c[3] * du + c[4] * dv + c[5]) * d;
    const double cz = (c[6] * du + c[7] * dv + c[8]) * d;
    px = c[9] * cx + c[10] * cy + c[11] * cz + c[12];
    py = c[13] * cx + c[14] * cy + c[15] * cz + c[16];
    pz = c[17] * cx + c[18] * cy + c[19] * cz + c[20];
}

__device__ __forceinline__ double ls_point_pitch(double px, double py, double pz) {
#pragma clang fp contract(off)
    return asin(pz / sqrt(px * px + py * py + pz * pz));
}

__device__ __forceinline__ double ls_pitch(const double *c, int u, int v, double d) {
    double px, py, pz;
    ls_point(c, u, v, d, px, py, pz);
    return ls_point_pitch(px, py, pz);
}

// Lane t's LS_PER pixels of a tile: VEC (16-byte aligned frames) two float4 at 4 (t + 256 j), else one float at t + 256 j.
template <bool VEC>
__device__ __forceinline__ int ls_loc(int t, int j) {
    return VEC ? 4 * (t + 256 * (j >> 2)) + (j & 3) : t + 256 * j;
}

template <bool VEC>
__device__ __forceinline__ void ls_load(const float *__restrict__ xf, int base, int HW, float (&v)[LS_PER]) {
    const int t = threadIdx.x;
    const float pad = __builtin_nanf("");  // beyond the frame: valid under no threshold
    if (VEC) {
#pragma unroll
        for (int q = 0; q < LS_PER / 4; ++q) {
            const int i = base + 4 * (t + 256 * q);
            const float4 f = i < HW ? *reinterpret_cast<const float4 *>(xf + i) : make_float4(pad, pad, pad, pad);
            v[4 * q] = f.x;
            v[4 * q + 1] = f.y;
            v[4 * q + 2] = f.z;
            v[4 * q + 3] = f.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LS_PER; ++j) {
            const int i = base + t + 256 * j;
            v[j] = i < HW ? xf[i] : pad;
        }
    }
}

// Appends the lane's valid pixels (x > thr, float32 as numpy compares; the padding's NaN is never valid) to the tile's
// list: a wave-wide prefix sum of the lanes' counts, one LDS atomic per wave.  Returns the lane's valid mask.
template <bool VEC>
__device__ __forceinline__ unsigned ls_compact(const float (&v)[LS_PER], float thr, int *s_n, u16 *s_idx, float *s_val) {
    const int t = threadIdx.x, lane = t & 63;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < LS_PER; ++j) m |= (v[j] > thr ? 1u : 0u) << j;
    const int c = __popc(m);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    int base = 0;
    if (lane == 63 && incl) base = atomicAdd(s_n, incl);
    int pos = __shfl(base, 63, 64) + incl - c;
#pragma unroll
    for (int j = 0; j < LS_PER; ++j)
        if (m & (1u << j)) {
            s_idx[pos] = (u16)ls_loc<VEC>(t, j);
            s_val[pos] = v[j];
            ++pos;
        }
    return m;
}

// tiles [blockIdx.x * tpb, min(T, (blockIdx.x + 1) * tpb)) of frame blockIdx.y, T = ceil(HW / LS_TILE)
template <bool VEC>
__global__ __launch_bounds__(256) void k_lines_range(const float *__restrict__ x, float thr, int W, int HW, int tpb,
                                                     const double *__restrict__ rec, double2 *__restrict__ part) {
    __shared__ u16 s_idx[LS_TILE];
    __shared__ float s_val[LS_TILE];
    __shared__ double2 s_red[4];
    __shared__ int s_n[2];
    const int t = threadIdx.x, b = blockIdx.y;
    const float *xf = x + (size_t)b * HW;
    const int T = (HW + LS_TILE - 1) / LS_TILE;
    const int tile0 = blockIdx.x * tpb, tile1 = min(T, tile0 + tpb);
    double c[LS_SING];  // the frame record: uniform loads, held in SGPRs
#pragma unroll
    for (int k = 0; k < LS_SING; ++k) c[k] = rec[(size_t)b * LS_REC + k];
    // a singular frame has no pitch; its valid pixels still count as points (status bit 1 stays clear)
    const bool sing = rec[(size_t)b * LS_REC + LS_SING] != 0.0;
    if (t == 0) s_n[0] = s_n[1] = 0;
    __syncthreads();
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int tile = tile0; tile < tile1; ++tile) {
        const int par = (tile - tile0) & 1;
        float v[LS_PER];
        ls_load<VEC>(xf, tile * LS_TILE, HW, v);
        ls_compact<VEC>(v, thr, &s_n[par], s_idx, s_val);
        __syncthreads();
        const int n = s_n[par];
        if (t == 0) s_n[par ^ 1] = 0;  // the next tile's counter: its last reader passed the previous tile's barrier
#pragma unroll 1
        for (int k = t; k < n; k += 256) {
            const int i = tile * LS_TILE + s_idx[k];
            const int row = i / W;
            const double p = sing ? 0.0 : ls_pitch(c, i - row * W, row, (double)s_val[k]);
            lo = ls_min(lo, p);
            hi = ls_max(hi, p);
        }
        __syncthreads();  // the list is rewritten by the next tile
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = ls_min(lo, __shfl_xor(lo, o, 64));
        hi = ls_max(hi, __shfl_xor(hi, o, 64));
    }
    if ((t & 63) == 0) s_red[t >> 6] = make_double2(lo, hi);
    __syncthreads();
    if (t == 0) {
        double2 r = s_red[0];
        for (int w = 1; w < 4; ++w) r = make_double2(ls_min(r.x, s_red[w].x), ls_max(r.y, s_red[w].y));
        part[(size_t)b * gridDim.x + blockIdx.x] = r;
    }
}

// The frame's pitch range from k_lines_range's nb partials, its bin interval and its DTFILL_LINES_* status; called by the 64
// lanes of one wave, the same result in each.
__device__ __forceinline__ int ls_frame_range(const double2 *__restrict__ part, int nb, int b, int n_bins,
                                              const double *__restrict__ rec, double &lo, double &iv) {
    const int t = threadIdx.x & 63;
    lo = __builtin_inf();
    double hi = -__builtin_inf();
    for (int k = t; k < nb; k += 64) {
        const double2 r = part[(size_t)b * nb + k];
        lo = ls_min(lo, r.x);
        hi = ls_max(hi, r.y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = ls_min(lo, __shfl_xor(lo, o, 64));
        hi = ls_max(hi, __shfl_xor(hi, o, 64));
    }
    iv = (hi - lo) / (double)n_bins;
    const bool sing = rec[(size_t)b * LS_REC + LS_SING] != 0.0;
    const bool empty = lo == __builtin_inf();  // a valid pixel's pitch is finite or NaN
    int st = (empty ? DTFILL_LINES_NO_POINTS : 0) | (sing ? DTFILL_LINES_SINGULAR : 0);
    if (!empty && !sing && !(iv > 0.0 && iv < __builtin_inf())) st |= DTFILL_LINES_BAD_INTERVAL;
    return st;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_lines_keep(const float *__restrict__ x, int W, int HW, int n_bins, int keep_every,
                                                    int tpb, const double *__restrict__ rec, const double2 *__restrict__ part,
                                                    float *__restrict__ out, int32_t *__restrict__ frame_status) {
    __shared__ u16 s_idx[LS_TILE];
    __shared__ float s_val[LS_TILE];
    __shared__ u8 s_keep[LS_TILE];
    __shared__ double s_lo, s_iv;
    __shared__ int s_n[2], s_status;
    const int t = threadIdx.x, b = blockIdx.y;
    const float *xf = x + (size_t)b * HW;
    float *of = out + (size_t)b * HW;
    const int T = (HW + LS_TILE - 1) / LS_TILE;
    const int tile0 = blockIdx.x * tpb, tile1 = min(T, tile0 + tpb);
    if (t < 64) {
        double lo, iv;
        const int st = ls_frame_range(part, (int)gridDim.x, b, n_bins, rec, lo, iv);
        if (t == 0) {
            s_lo = lo;
            s_iv = iv;
            s_status = st;
            s_n[0] = s_n[1] = 0;
        }
    }
    __syncthreads();
    const int status = s_status;
    if (blockIdx.x == 0 && t == 0) frame_status[b] = status;
    if (status != 0) {  // nothing is kept: zeros over the block's tiles
        for (int i = tile0 * LS_TILE + (VEC ? 4 * t : t); i < min(tile1 * LS_TILE, HW); i += VEC ? 1024 : 256) {
            if (VEC)
                *reinterpret_cast<float4 *>(of + i) = make_float4(0.f, 0.f, 0.f, 0.f);
            else
                of[i] = 0.0f;
        }
        return;
    }
    const double lo = s_lo, iv = s_iv, ke = (double)keep_every;
    double c[LS_SING];  // the frame record: uniform loads, held in SGPRs
#pragma unroll
    for (int k = 0; k < LS_SING; ++k) c[k] = rec[(size_t)b * LS_REC + k];
    for (int tile = tile0; tile < tile1; ++tile) {
        const int par = (tile - tile0) & 1, base = tile * LS_TILE;
        float v[LS_PER];
        ls_load<VEC>(xf, base, HW, v);
        const unsigned m = ls_compact<VEC>(v, 0.1f, &s_n[par], s_idx, s_val);
        __syncthreads();
        const int n = s_n[par];
        if (t == 0) s_n[par ^ 1] = 0;
#pragma unroll 1
        for (int k = t; k < n; k += 256) {
            const int loc = s_idx[k], i = base + loc;
            const int row = i / W;
            const double q = (ls_pitch(c, i - row * W, row, (double)s_val[k]) - lo) / iv;
            s_keep[loc] = fmod(ceil(q), ke) == 0.0 ? 1 : 0;  // the label is not clamped (q of the maximum is n_bins or just above)
        }
        __syncthreads();
        float o[LS_PER];
#pragma unroll
        for (int j = 0; j < LS_PER; ++j) o[j] = ((m >> j) & 1u) && s_keep[ls_loc<VEC>(t, j)] ? v[j] : 0.0f;
        if (VEC) {
#pragma unroll
            for (int q = 0; q < LS_PER / 4; ++q) {
                const int i = base + 4 * (t + 256 * q);
                if (i < HW) *reinterpret_cast<float4 *>(of + i) = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < LS_PER; ++j) {
                const int i = base + t + 256 * j;
                if (i < HW) of[i] = o[j];
            }
        }
        __syncthreads();  // the list and the keep bytes are rewritten by the next tile
    }
}
