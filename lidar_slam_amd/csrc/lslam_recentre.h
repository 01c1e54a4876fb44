// lslam_recentre.h — rolling occupancy grids: each robot's grid and origin are shifted by whole
// cells, in place, when the filter's pose nears the edge of the map.  The definition (robot cell,
// shift rule, the two roundings of the new origin, the moved 16-bit patterns) is the comment on
// lslam_grid_recentre in include/lidarslam.h; tests/recentre_ref.py is its NumPy form; the shift rule
// and the in-place plan (bands, their order, copy and zero intervals) are lslam_recentre_plan.h.
//
// recentre_kernel<CELLS>: one 256-thread workgroup per robot, and only one: two workgroups on one
// robot would race, the second reading rows that the first has already stored.
//   0. every thread reads the pose and the origin (40 bytes) and computes the decision with the same
//      instructions, so all hold what thread 0 writes to shift and flags.  A robot that does not
//      move ends here.
//   1. the bands of the plan, in its order.  A band is loaded completely, the loads are waited for
//      (vmcnt(0)) in front of a workgroup barrier, and only then is it stored: no wave stores a row
//      that another wave has yet to read.  The next band's loads need no second barrier: by the
//      plan's order no band reads a row that an earlier one stored.
//      With rows and the column shift on 16-byte groups (grid_w and sx multiples of 8) a thread
//      holds 8 groups in registers: 256 x 8 x 16 B = 32 KiB in flight per workgroup.  Zero rows and
//      zero groups are registers set to zero, from the plan's intervals.
//      Otherwise (CELLS = 1 only) a lane per cell, 2-byte accesses, the band parked in 32 KiB of LDS;
//      a thread reads back only what it wrote there, so LDS needs no barrier of its own.
//   2. after the last barrier's side of the reads, thread 0 writes the new origin: every thread has
//      read the old one before the first barrier.
// The robot of a workgroup is a permutation of its block index (recentre_robot_of_block).
// CELLS = 0 is launched when grid_w and quantum are multiples of 8 (the defaults): every shift is
// then on 16-byte groups, and the instantiation carries no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_recentre_plan.h"

namespace lslam {

constexpr int RECENTRE_TPB = 256;  // threads per workgroup
constexpr int RECENTRE_VPT = RECENTRE_BAND_CELLS / 8 / RECENTRE_TPB;  // 16-byte groups per thread and band: 8

struct RecentreArgs {
    lslam_recentre_batch b;
    double cell, inv;
    int grid_w, margin, quantum;
    int band_rows;  // recentre_band_rows(grid_w)
    int vec;        // rows of logodds lie on 16-byte boundaries
};

// Workgroups are dealt to the 8 XCDs by blockIdx % 8.  With robot = block, a fleet in which every 8th
// or 16th robot moves would do all its moving on one XCD or two.  The low three bits of the block index
// are therefore XORed with two higher groups of three: within every aligned group of 8 blocks a
// permutation (its own inverse), under which strides of 8, 16 and 64 robots spread over all XCDs as
// neighbours do.  Measured, 4096 robots with one in sixteen moving: 0.2125 ms before.
__host__ __device__ static inline int recentre_robot_of_block(int b) { return b ^ (((b >> 3) ^ (b >> 6)) & 7); }
static inline int recentre_blocks(int n_robots) { return (n_robots + 7) & ~7; }

// Steps 0 to 3 of the definition for robot r: the one text of the decision, for this kernel and for
// the paged one (lslam_page.h).  Every thread computes it with the same instructions.
struct RecentreDecision {
    int sx, sy, flag;
    double nox, noy;  // the new origin (the old one where nothing moves)
};

__device__ __forceinline__ RecentreDecision recentre_decide(const RecentreArgs &a, int r) {
    const int W = a.grid_w;
    const double px = a.b.pose[3 * r], py = a.b.pose[3 * r + 1], th = a.b.pose[3 * r + 2];
    const double ox = a.b.origin[2 * r], oy = a.b.origin[2 * r + 1];
    const double X0d = floor((px - ox) * a.inv), Y0d = floor((py - oy) * a.inv);
    const bool finite5 = __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(th) &&
                         __builtin_isfinite(ox) && __builtin_isfinite(oy);
    int sx = 0, sy = 0, flag = 0;
    double nox = ox, noy = oy;
    if (!(finite5 && fabs(X0d) < 1048576.0 && fabs(Y0d) < 1048576.0)) {
        flag = LSLAM_RECENTRE_BAD_POSE;
    } else {
        recentre_shift((int)X0d, (int)Y0d, W, a.margin, a.quantum, sx, sy);
        if (sx | sy) {
            {
#pragma clang fp contract(off)
                const double mx = (double)sx * a.cell, my = (double)sy * a.cell;
                nox = ox + mx;
                noy = oy + my;
            }
            if (__builtin_isfinite(nox) && __builtin_isfinite(noy)) {
                flag = LSLAM_RECENTRE_MOVED | ((abs(sx) >= W || abs(sy) >= W) ? LSLAM_RECENTRE_CLEARED : 0);
            } else {
                flag = LSLAM_RECENTRE_BAD_POSE;
                sx = sy = 0;
            }
        }
    }
    return {sx, sy, flag, nox, noy};
}

// Step 4 for one robot's grid L, by the whole workgroup: the bands of the plan, in its order.  Every
// band's stores stand behind a workgroup barrier that follows the band's loads.
template <int CELLS>
__device__ __forceinline__ void recentre_move(const RecentreArgs &a, int16_t *L, int sx, int sy, int tid) {
    const int W = a.grid_w;
    const RecentrePlan p = recentre_plan(W, sx, sy, a.band_rows);
    bool groups = true;
    if constexpr (CELLS != 0) groups = a.vec && (sx & 7) == 0;
    if (groups) {
        uint4 *L4 = (uint4 *)L;
        const int W8 = W >> 3, gx0 = p.dx0 >> 3, gx1 = p.dx1 >> 3, gs = sx >> 3;  // (sx is a multiple of 8: the shift is exact)
        for (int k = 0; k < p.nbands; k++) {
            const RecentreBand b = recentre_band(p, k);
            const int n = (b.y1 - b.y0) * W8;  // <= RECENTRE_TPB * RECENTRE_VPT groups
            uint4 v[RECENTRE_VPT];
#pragma unroll
            for (int j = 0; j < RECENTRE_VPT; j++) {
                const int g = tid + j * RECENTRE_TPB;
                const int row = g / W8, c = g - row * W8, y = b.y0 + row;
                const bool copy = g < n && y >= b.cy0 && y < b.cy1 && c >= gx0 && c < gx1;
                // (a group that is not copied loads the robot's first group instead of branching
                // around the load: eight loads are issued back to back)
                const uint4 t = L4[copy ? (y + sy) * W8 + c + gs : 0];
                v[j] = copy ? t : make_uint4(0u, 0u, 0u, 0u);
            }
            // the band's reads have returned, in every wave, before any wave stores: vmcnt(0), with
            // expcnt and lgkmcnt left alone (0x0f70)
            __builtin_amdgcn_s_waitcnt(0x0f70);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < RECENTRE_VPT; j++) {
                const int g = tid + j * RECENTRE_TPB;
                if (g < n) L4[b.y0 * W8 + g] = v[j];
            }
        }
    } else if constexpr (CELLS != 0) {
        __shared__ uint16_t buf[RECENTRE_BAND_CELLS];
        uint16_t *L1 = (uint16_t *)L;
        for (int k = 0; k < p.nbands; k++) {
            const RecentreBand b = recentre_band(p, k);
            const int n = (b.y1 - b.y0) * W;  // <= RECENTRE_BAND_CELLS
            for (int i = tid; i < n; i += RECENTRE_TPB) {
                const int row = i / W, x = i - row * W;
                int src;
                buf[i] = recentre_source(p, b, b.y0 + row, x, src) ? L1[src] : (uint16_t)0;
            }
            __syncthreads();  // (a value parked in LDS has returned from HBM)
            for (int i = tid; i < n; i += RECENTRE_TPB) L1[b.y0 * W + i] = buf[i];
        }
    }
}

template <int CELLS>
__global__ __launch_bounds__(RECENTRE_TPB) void recentre_kernel(const RecentreArgs a) {
    const int tid = (int)threadIdx.x, r = recentre_robot_of_block((int)blockIdx.x);
    if (r >= a.b.n_robots) return;  // (the grid is padded to whole groups of 8 blocks)

    // ---- 0. the decision: steps 0 to 3 ----
    const RecentreDecision d = recentre_decide(a, r);
    if (tid == 0) {
        a.b.shift[2 * r] = d.sx;
        a.b.shift[2 * r + 1] = d.sy;
        a.b.flags[r] = d.flag;
    }
    if (!(d.sx | d.sy)) return;  // (uniform: every thread holds the same decision)

    // ---- 1. the grid, band after band ----
    recentre_move<CELLS>(a, a.b.logodds + (int64_t)r * a.grid_w * a.grid_w, d.sx, d.sy, tid);

    // ---- 2. the origin: every thread read it before the barriers above ----
    if (tid == 0) {
        a.b.origin[2 * r] = d.nox;
        a.b.origin[2 * r + 1] = d.noy;
    }
}

}  // namespace lslam
