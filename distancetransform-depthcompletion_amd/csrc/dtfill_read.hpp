// dtfill_read.hpp -- depth_read() of the reference's loader (data_read.py:81-99) on decoded 16-bit PNG values: the
// "max > 255" check over the whole source, /256 and Pillow's NEAREST resize to H x W (include/dtfill.h has the contract).
// Part of libdtfill.so; included by dtfill.hip inside its anonymous namespace (one translation unit).
#pragma once

// ------------------------------------------------------------------------------------------------
// Two launches:
//   k_read_maps    one block per frame, one wave per axis: Pillow's running double sum (ImagingScaleAffine's
//                  xo = 0.5 * a; idx = (int)xo; xo += a) -> ry [B,H] / rx [B,W] in the workspace.  The sum is one dependent chain: every
//                  lane of the wave runs it, lane l from step l on, and the wave stores 64 indices every 64 steps.  Zeroes the
//                  frame's status word.
//   k_read_gather  frames along grid x, bands of rpb output rows along y, lanes along columns.  Block k scans the source rows
//                  [ry[i0-1] + 1, ry[i1-1] + 1) (the first block from 0, the last to h): every source row exactly once over
//                  the frame's blocks, those no output row samples included, and in the same block as (most of) the output
//                  rows that sample it, so the gather's reads hit the cache the scan filled.  Then it stores its rows,
//                  float4 where W % 4 == 0.  Each block adds "done, and whether a value > 255 was seen" to the frame's word
//                  by one relaxed agent-scope atomic add; the block whose add completes the count writes frame_status.
// The frame's word is the only thing two workgroups share in a launch, and only atomics touch it there; the map kernel's
// plain zeroing store is handed on by the launch boundary.
// ------------------------------------------------------------------------------------------------
constexpr int DR_ROWS = 8;        // output rows per gather block (more when H > 65535 * 8: grid y is 16 bits)
constexpr int DR_THREADS = 256;

// (h, w) of frame b: dims[b] or the pitch; false for dims outside [1, hmax] x [1, wmax]
__device__ __forceinline__ bool dr_dims(const int32_t *__restrict__ dims, int b, int hmax, int wmax, int &h, int &w) {
    h = hmax;
    w = wmax;
    if (dims) {
        h = dims[2 * b];
        w = dims[2 * b + 1];
    }
    return h >= 1 && h <= hmax && w >= 1 && w <= wmax;
}

__global__ __launch_bounds__(128) void k_read_maps(const int32_t *__restrict__ dims, int hmax, int wmax, int H, int W,
                                                   int *__restrict__ ry, int *__restrict__ rx, u32 *__restrict__ fw) {
    const int b = blockIdx.x, axis = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) fw[b] = 0u;
    int h, w;
    if (!dr_dims(dims, b, hmax, wmax, h, w)) return;  // k_read_gather stores zeros and reads no map
    const int n = axis ? W : H, in = axis ? w : h;
    int *m = axis ? rx + (size_t)b * W : ry + (size_t)b * H;
    const double a = (double)in / (double)n;  // IEEE division, as Pillow's box size / output size
    const double last = (double)(in - 1);
    // lane l runs the same chain from y_0 to y_l first (l masked steps), then 64 steps per store: y_l, y_(l+64), ... are
    // bit for bit the chain's values, and the loop body is the dependent add alone
    double y = 0.5 * a;
    for (int t = 0; t < 63; ++t) y = t < lane ? y + a : y;
    for (int base = 0; base < n; base += 64) {
        // trunc(min(y, in - 1)) == min((int)y, in - 1): the clamp only binds where H or W >= 2^26 lets the running sum's
        // rounding reach the edge, and keeps every read inside the frame
        if (base + lane < n) m[base + lane] = (int)fmin(y, last);
#pragma unroll 16
        for (int t = 0; t < 64; ++t) y += a;  // a plain add: nothing to contract
    }
}

// OR of the values p[0..w) of one source row: 16-byte loads between the first and last 16-byte boundary inside the row,
// single elements before and after it, so no byte outside the row is read
__device__ __forceinline__ void dr_row_split(const u16 *p, int w, int &head, int &nv, int &tail0) {
    const uintptr_t a = (uintptr_t)p;
    head = min(w, (a & 1) ? w : (int)(((16u - (u32)(a & 15)) & 15u) >> 1));
    nv = (w - head) >> 3;
    tail0 = head + nv * 8;
}

__device__ __forceinline__ u32 dr_or_row(const u16 *__restrict__ p, int w, int tid) {
    int head, nv, tail0;
    dr_row_split(p, w, head, nv, tail0);
    const uint4 *v = reinterpret_cast<const uint4 *>(p + head);
    u32 acc = 0;
    for (int k = tid; k < nv; k += DR_THREADS) {
        const uint4 t = v[k];
        acc |= t.x | t.y | t.z | t.w;
    }
    for (int j = tid; j < head; j += DR_THREADS) acc |= p[j];  // head < 8 unless p is odd-aligned
    if (tid < w - tail0) acc |= p[tail0 + tid];             // < 8 elements
    return acc;
}

// ... the same for rows of 16 to DR_W1 values at an even address, without a branch: every lane issues one 16-byte load (a
// chunk, or chunk 0 again) and one 2-byte load (a head or tail element, or element 0 again) inside the row, so that the loads
// of several rows are in flight together
constexpr int DR_W1 = 8 * (DR_THREADS - 16);
__device__ __forceinline__ u32 dr_or_row1(const u16 *__restrict__ p, int w, int tid) {
    int head, nv, tail0;
    dr_row_split(p, w, head, nv, tail0);  // w >= 16: nv >= 1
    const uint4 t = reinterpret_cast<const uint4 *>(p + head)[tid < nv ? tid : 0];
    const int e = tid - nv;  // head elements, then tail elements
    const bool in_head = e >= 0 && e < head, in_tail = e >= head && e - head < w - tail0;
    const u32 x = p[in_head ? e : in_tail ? tail0 + e - head : 0];
    return (tid < nv ? t.x | t.y | t.z | t.w : 0u) | (in_head || in_tail ? x : 0u);
}

template <bool VEC>
__global__ __launch_bounds__(DR_THREADS) void k_read_gather(const u16 *__restrict__ raw, const int32_t *__restrict__ dims,
                                                            int hmax, int wmax, int H, int W, int rpb,
                                                            const int *__restrict__ ry, const int *__restrict__ rx,
                                                            u32 *__restrict__ fw, float *__restrict__ out,
                                                            int32_t *__restrict__ frame_status) {
    const int b = blockIdx.x, k = blockIdx.y, nb = gridDim.y, tid = threadIdx.x;
    const int i0 = k * rpb, i1 = min(H, i0 + rpb);
    int h, w;
    const bool ok = dr_dims(dims, b, hmax, wmax, h, w);  // block-uniform
    const int *ryb = ry + (size_t)b * H;
    const int *rxb = rx + (size_t)b * W;
    const u16 *src = raw + (size_t)b * hmax * wmax;
    float *o = out + (size_t)b * H * W;
    const float s = 0.00390625f;  // 2^-8: v / 256 is exact in float32 for every 16-bit v
    u32 acc = 0;
    if (ok) {
        const int r0 = k == 0 ? 0 : ryb[i0 - 1] + 1;
        const int r1 = k == nb - 1 ? h : ryb[i1 - 1] + 1;
        if (w >= 16 && w <= DR_W1 && !((uintptr_t)raw & 1)) {  // (an odd-aligned raw reads element by element)
            for (int r = r0; r < r1; r += 4) {
                u32 t[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) t[u] = dr_or_row1(src + (size_t)min(r + u, r1 - 1) * wmax, w, tid);  // (a row twice)
                acc |= t[0] | t[1] | t[2] | t[3];
            }
        } else {
            for (int r = r0; r < r1; ++r) acc |= dr_or_row(src + (size_t)r * wmax, w, tid);
        }
        // the gather, DR_ROWS output rows at a time: their loads are issued before their stores
        for (int ib = i0; ib < i1; ib += DR_ROWS) {
            const u16 *row[DR_ROWS];
#pragma unroll
            for (int u = 0; u < DR_ROWS; ++u) row[u] = src + (size_t)ryb[min(ib + u, i1 - 1)] * wmax;
            if (VEC) {
                for (int q = tid; q < (W >> 2); q += DR_THREADS) {
                    const int4 c = reinterpret_cast<const int4 *>(rxb)[q];
                    float4 v[DR_ROWS];
#pragma unroll
                    for (int u = 0; u < DR_ROWS; ++u)
                        v[u] = make_float4((float)row[u][c.x] * s, (float)row[u][c.y] * s, (float)row[u][c.z] * s,
                                           (float)row[u][c.w] * s);
#pragma unroll
                    for (int u = 0; u < DR_ROWS; ++u)
                        if (ib + u < i1) reinterpret_cast<float4 *>(o + (size_t)(ib + u) * W)[q] = v[u];
                }
            } else {
                for (int j = tid; j < W; j += DR_THREADS) {
                    const int c = rxb[j];
                    float v[DR_ROWS];
#pragma unroll
                    for (int u = 0; u < DR_ROWS; ++u) v[u] = (float)row[u][c] * s;
#pragma unroll
                    for (int u = 0; u < DR_ROWS; ++u)
                        if (ib + u < i1) o[(size_t)(ib + u) * W + j] = v[u];
                }
            }
        }
    } else {
        for (int i = i0; i < i1; ++i)
            for (int j = tid; j < W; j += DR_THREADS) o[(size_t)i * W + j] = 0.0f;
    }
    if (!frame_status) return;  // block-uniform
    const int high = __syncthreads_or((acc & 0xFF00FF00u) != 0u);  // a value > 255 in the block's rows
    if (tid == 0) {
        // one word per frame: blocks done in the low half, blocks that saw a value > 255 in the high half (nb <= 65535).  A
        // relaxed RMW on one word sees every earlier one, so the block that completes the count knows the frame's total
        // without a fence (an acq_rel counter puts a buffer_wbl2, a write-back of the XCD's L2, in front of every block's add)
        const u32 inc = 1u + (high ? 0x10000u : 0u);
        const u32 now = __hip_atomic_fetch_add(&fw[b], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + inc;
        if ((now & 0xFFFFu) == (u32)nb) frame_status[b] = !ok ? DTFILL_READ_BAD_DIMS : (now >> 16) ? 0 : DTFILL_READ_NOT_16BIT;
    }
}
