// lslam_dist.h — the exact distance field of each robot's occupancy grid, and its read under a
// revolution.  The definitions are the comments on lslam_grid_distance and lslam_field_score in
// include/lidarslam.h; tests/dist_ref.py and tests/fieldscore_ref.py are their NumPy forms; the two
// 1-D passes of the transform are lslam_dist_core.h (plain C++, also compiled on the CPU).
//
// dist_kernel<CELLS>: one 512-thread workgroup per (robot, band of rows).  The column pass and the
// row pass are fused: the intermediate g never leaves LDS, logodds is read once and d2 written once,
// and there is no scratch in device memory.
//   1. the source bitmap of the band's rows and of the hal = min(d_max, grid_w) - 1 rows on either
//      side of it (clipped to the map), one bit per cell, 32 rows of a column to a word, words of one
//      row block side by side (bits[block][x]: a wave reading a row block at consecutive x reads
//      consecutive banks).  A thread takes a block of 32 rows of 8 columns: 32 loads of 16 bytes (8
//      cells, CELLS = 8: grid_w a multiple of 8, logodds and d2 on 16-byte boundaries), eight in flight,
//      thresholded into eight words kept in registers and stored as two 16-byte LDS writes; the lanes
//      of a wave read 1 KiB of a row side by side.  Otherwise (CELLS = 1) a lane per column, 2-byte
//      loads.  No atomics on the bitmap.  The words' set bits are counted on the way: those of the
//      band's own rows are the robot's n_src (global atomicAdd onto the zeroed count; a band that holds
//      a source clears the preset LSLAM_DIST_EMPTY), all of them say whether the band can skip step 2.
//   2. rows of the band, eight at a time, one per wave.
//      a. column pass: lane x takes g[y][x] from the words of column x by count-trailing/leading-zeros
//         (dist_column_g), at most d_max / 32 + 2 words per direction, into the wave's row of bytes.
//         The ballots of g < d_max, 64 columns each, are the row's unsaturated columns as a bit mask.
//      b. row pass: lane x searches outwards over that row of g with the exit r^2 >= best
//         (dist_row_d2), at most min(d_max, grid_w) - 1 steps of two byte reads, starting at the
//         nearest unsaturated column (dist_nearest_col on the mask): the saturated stretch around a
//         cell, all of a room's outside and most of a sparse map, is skipped, and a cell with no such
//         column within d_max stores the cap.  A row whose g is saturated everywhere, and a band
//         without a source bit, store the cap without searching.  NOT_FREE mode takes the minimum
//         with the border's b^2.
//      c. the row of d2 leaves through the wave's row of uint16 in LDS as 16-byte stores (CELLS = 8).
//      Two workgroup barriers per eight rows separate a, b and c.
// LDS: 16 B of counters + 4 grid_w nblk B of bitmap (nblk = ceil(min(grid_w, band + 2 hal) / 32)) +
// 8 waves x (roundup(grid_w, 16) x 3 B of rows + 256 B of mask): at the defaults (grid_w 512, d_max 64,
// a band of 512 rows) 16 + 32768 + 12288 + 2048 = 47,120 B, three workgroups to a CU's 160 KiB.  The launcher shrinks the
// band until a workgroup's LDS is at most 80 KiB (two to a CU), then until it fits 160 KiB; at grid_w
// above 1757 the largest d_max that fits is below 255 (grid_w 2048: 205) and the call returns
// LSLAM_ERR_UNSUPPORTED beyond.  With few robots the band also shrinks so that the bands fill the
// chip (launch_mapmatch's rule, at most 16 bands per robot); a band reads its halo rows again.
//
// fieldscore_kernel: one 256-thread workgroup per (robot, slice of its points), a lane per point:
// steps 0 and 1 of lslam_grid_update, one 2-byte gather from d2, a wave reduction of four 64-bit sums
// and one global atomicAdd per wave and sum (integers: any order).  rot, clear2 and flags are written
// by the robot's slice 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_dist_core.h"
#include "lslam_grid.h"
#include "lslam_mapmatch.h"
#include "lslam_wave.h"

namespace lslam {

constexpr int DIST_TPB = 512;
constexpr int DIST_NW = DIST_TPB / 64;       // rows in flight: one per wave
constexpr int DIST_MASK_WORDS = 32;           // 64-column words of a row's mask: grid_w <= 2048
constexpr int DIST_LDS_TWO = 80 * 1024;      // two workgroups to a CU
constexpr int DIST_LDS_MAX = 160 * 1024;     // a CU's LDS
constexpr int DIST_MAX_SLICES = 16;
constexpr int FIELDSCORE_TPB = 256;
constexpr int FIELDSCORE_MAX_SLICES = 16;

struct DistArgs {
    lslam_dist_batch b;
    int grid_w, d_max, thr;  // a cell is a source iff L >= thr
    int not_free;            // the border term of LSLAM_DIST_NOT_FREE
    int band, n_slices;      // rows per workgroup, workgroups per robot
    int hal;                 // rows of the bitmap on either side of a band
    int nblk;                // most 32-row blocks of a band's bitmap
};

__host__ __device__ static inline int dist_row_pitch(int W) { return (W + 15) & ~15; }
// 32-row blocks of the bitmap of a band of `band` rows
static inline int dist_blocks(int W, int band, int hal) {
    const int rows = band + 2 * hal < W ? band + 2 * hal : W;
    return (rows + 31) >> 5;
}
// LDS bytes: counters, bitmap, the waves' rows of d2 and of g
static inline int dist_lds_bytes(int W, int nblk) {
    return 16 + ((4 * W * nblk + 15) & ~15) + DIST_NW * (dist_row_pitch(W) * 3 + DIST_MASK_WORDS * 8);
}

__device__ __forceinline__ int dist_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int CELLS>
__global__ __launch_bounds__(DIST_TPB) void dist_kernel(const DistArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = a.grid_w, d_max = a.d_max, thr = a.thr;
    const int r = (int)blockIdx.x / a.n_slices, slice = (int)blockIdx.x - r * a.n_slices;
    const int y0 = slice * a.band, y1 = min(W, y0 + a.band);
    if (y0 >= W) return;  // (n_slices is ceil(grid_w / band): no such workgroup is launched)
    const int base = max(0, y0 - a.hal), top = min(W, y1 + a.hal);
    const int nblk = (top - base + 31) >> 5;  // <= a.nblk
    const int pitch = dist_row_pitch(W);
    int *cnt = (int *)smem;  // [0]: source cells in the band's own rows; [1]: in all the rows loaded
    uint32_t *bits = (uint32_t *)(smem + 16);
    uint16_t *ob = (uint16_t *)(smem + 16 + ((4 * W * a.nblk + 15) & ~15)) + wv * pitch;
    uint8_t *gb = smem + 16 + ((4 * W * a.nblk + 15) & ~15) + DIST_NW * pitch * 2 + wv * pitch;
    uint64_t *mk = (uint64_t *)(smem + 16 + ((4 * W * a.nblk + 15) & ~15) + DIST_NW * pitch * 3) + wv * DIST_MASK_WORDS;
    const int16_t *L = a.b.logodds + (int64_t)r * W * W;
    uint16_t *D = a.b.d2 + (int64_t)r * W * W;

    // ---- 1. the bitmap ----
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();
    {
        constexpr int GW = CELLS;  // columns per task
        const int ngrp = W / GW, ntask = nblk * ngrp;
        int n_band = 0, n_all = 0;
        for (int t = tid; t < ntask; t += DIST_TPB) {
            const int blk = t / ngrp, c = t - blk * ngrp, yb = base + 32 * blk;
            const int nrow = min(32, top - yb);  // >= 1
            uint32_t w[GW];
#pragma unroll
            for (int k = 0; k < GW; k++) w[k] = 0u;
            if constexpr (CELLS == 8) {
                const uint4 *L4 = (const uint4 *)(L + (int64_t)yb * W + 8 * c);
                const int W8 = W >> 3;
                for (int j0 = 0; j0 < 32; j0 += 8) {
                    uint4 v[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) v[u] = L4[(int64_t)min(j0 + u, nrow - 1) * W8];  // (a row past the block's end loads its last row)
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const uint32_t on = j0 + u < nrow ? 1u : 0u;
                        const uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int l0 = (int)(int16_t)(d[i] & 0xffffu), l1 = (int)d[i] >> 16;  // (the low half is the lower address)
                            w[2 * i] |= (l0 >= thr ? on : 0u) << (j0 + u);
                            w[2 * i + 1] |= (l1 >= thr ? on : 0u) << (j0 + u);
                        }
                    }
                }
                uint4 *B4 = (uint4 *)(bits + blk * W + 8 * c);
                B4[0] = make_uint4(w[0], w[1], w[2], w[3]);
                B4[1] = make_uint4(w[4], w[5], w[6], w[7]);
            } else {
                const int16_t *Lc = L + (int64_t)yb * W + c;
                for (int j = 0; j < nrow; j++) w[0] |= ((int)Lc[(int64_t)j * W] >= thr ? 1u : 0u) << j;
                bits[blk * W + c] = w[0];
            }
            // the block's rows that are the band's own: [lo, hi) of 0 .. 32
            const int lo = max(0, y0 - yb), hi = min(32, y1 - yb);
            const uint32_t own = hi > lo ? (hi >= 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
#pragma unroll
            for (int k = 0; k < GW; k++) {
                n_all += __popc(w[k]);
                n_band += __popc(w[k] & own);
            }
        }
        n_all = dist_wave_sum(n_all);
        n_band = dist_wave_sum(n_band);
        if (lane == 0) {
            if (n_band) atomicAdd(&cnt[0], n_band);
            if (n_all) atomicAdd(&cnt[1], n_all);
        }
    }
    __syncthreads();
    if (tid == 0 && cnt[0]) {  // (n_src is zeroed and flags preset to LSLAM_DIST_EMPTY by the launcher)
        atomicAdd(&a.b.n_src[r], cnt[0]);
        a.b.flags[r] = 0;
    }
    const bool empty = cnt[1] == 0;  // no source within reach of the band: every row is saturated

    // ---- 2. the band's rows, one per wave ----
    const int cap = d_max * d_max;
    const int niter = (y1 - y0 + DIST_NW - 1) / DIST_NW;
    for (int it = 0; it < niter; it++) {
        const int y = y0 + it * DIST_NW + wv;
        const bool active = y < y1;
        bool sat = true;
        if (active && !empty) {
            uint64_t any = 0;
            for (int x0 = 0; x0 < W; x0 += 64) {  // (uniform: the ballot below is taken by the whole wave)
                const int x = x0 + lane;
                int g = d_max;
                if (x < W) {
                    g = dist_column_g(bits + x, W, nblk, y - base, d_max);
                    gb[x] = (uint8_t)g;
                }
                const uint64_t m = ballot(g < d_max);
                if (lane == 0) mk[x0 >> 6] = m;
                any |= m;
            }
            sat = any == 0;
        }
        __syncthreads();  // the wave's row of g is complete
        if (active) {
            uint16_t *Dr = D + (int64_t)y * W;
            for (int x = lane; x < W; x += 64) {
                int v = cap;
                if (!sat) {
                    const int r0 = dist_nearest_col(mk, (W + 63) >> 6, x, d_max);
                    if (r0 < d_max) v = dist_row_d2(gb, W, x, d_max, r0);
                }
                if (a.not_free) v = min(v, dist_border2(x, y, W));
                if constexpr (CELLS == 8) ob[x] = (uint16_t)v;
                else Dr[x] = (uint16_t)v;
            }
        }
        __syncthreads();  // the wave's row of d2 is complete, and its row of g has been read
        if constexpr (CELLS == 8) {
            if (active) {
                uint4 *D4 = (uint4 *)(D + (int64_t)y * W);
                const uint4 *O4 = (const uint4 *)ob;
                for (int gi = lane; gi < (W >> 3); gi += 64) D4[gi] = O4[gi];
            }
        }
    }
}

struct FieldScoreArgs {
    lslam_fieldscore_batch b;
    double inv, max_r2;
    int grid_w, trunc2, near2, off2;
    int n_slices;  // workgroups per robot
};

__device__ __forceinline__ unsigned long long fieldscore_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor_u64(v, o);
    return v;
}

__global__ __launch_bounds__(FIELDSCORE_TPB) void fieldscore_kernel(const FieldScoreArgs a) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int ns = a.n_slices;
    const int r = (int)blockIdx.x / ns, slice = (int)blockIdx.x - r * ns;
    const bool first = slice == 0;  // the robot's workgroup that writes rot, clear2 and flags

    // ---- 0. pose, rotation, robot cell ----
    const double px = a.b.pose[3 * r], py = a.b.pose[3 * r + 1], th = a.b.pose[3 * r + 2];
    const double ox = a.b.origin[2 * r], oy = a.b.origin[2 * r + 1];
    const double inv = a.inv;
    const double c = cos(th), s = sin(th);
    if (first && tid == 0) {
        a.b.rot[2 * r] = c;
        a.b.rot[2 * r + 1] = s;
    }
    double X0d, Y0d;
    if (!mapmatch_robot_cell(px, py, th, ox, oy, inv, X0d, Y0d)) {
        if (first && tid == 0) {  // (stats[r] is zeroed by the launcher)
            a.b.flags[r] = LSLAM_FIELD_BAD_POSE;
            a.b.clear2[r] = 0;
        }
        return;
    }
    const int W = a.grid_w;
    const uint16_t *D = a.b.d2 + (int64_t)r * W * W;
    if (first && tid == 0) {
        const int X0 = (int)X0d, Y0 = (int)Y0d;
        const bool on = (unsigned)X0 < (unsigned)W && (unsigned)Y0 < (unsigned)W;
        a.b.flags[r] = 0;
        a.b.clear2[r] = on ? (int)D[(int64_t)Y0 * W + X0] : a.off2;
    }
    // the slice's points [s0, s1): a multiple of 64 of them but for the robot's last
    const int p0 = a.b.pt_off[r], p1 = a.b.pt_off[r + 1];
    const int per = (int)((((int64_t)(p1 - p0) + ns - 1) / ns + 63) & ~(int64_t)63);
    const int64_t s0l = (int64_t)p0 + (int64_t)slice * per;
    const int s0 = (int)(s0l < p1 ? s0l : p1), s1 = (int)(s0l + per < p1 ? s0l + per : p1);
    if (s0 >= s1) return;

    // ---- 1. points -> hit cells -> the field ----
    const double2 *xy = (const double2 *)a.b.xy;
    unsigned long long sum = 0, n = 0, near = 0, off = 0;
    for (int p = s0 + tid; p < s1; p += FIELDSCORE_TPB) {
        const double2 q = xy[p];
        if (!grid_valid(q) || q.x * q.x + q.y * q.y > a.max_r2) continue;
        const double wx = px + (c * q.x - s * q.y);
        const double wy = py + (s * q.x + c * q.y);
        // within max_range / cell + 1 <= 4097 cells of the robot cell: the conversions cannot overflow
        const int X1 = (int)floor((wx - ox) * inv), Y1 = (int)floor((wy - oy) * inv);
        const bool on = (unsigned)X1 < (unsigned)W && (unsigned)Y1 < (unsigned)W;
        const int v = on ? (int)D[(int64_t)Y1 * W + X1] : a.off2;
        sum += (unsigned long long)min(v, a.trunc2);
        n++;
        near += v <= a.near2 ? 1u : 0u;
        off += on ? 0u : 1u;
    }
    const unsigned long long t[4] = {fieldscore_wave_sum(sum), fieldscore_wave_sum(n), fieldscore_wave_sum(near),
                                     fieldscore_wave_sum(off)};
    if (lane == 0) {
        unsigned long long *st = (unsigned long long *)(a.b.stats + 4 * (int64_t)r);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (t[k]) atomicAdd(&st[k], t[k]);
    }
}

}  // namespace lslam
