// lslam_raycast.h — batched ray casting through the occupancy grid: one revolution per robot, the
// robot's pose and its log-odds grid -> per beam where the map stops it and how that compares with
// where it returned.  The definition is the comment on lslam_grid_raycast in include/lidarslam.h;
// tests/raycast_ref.py is its NumPy form; one beam's far cell, walk and class are
// lslam_raycast_walk.h (plain C++, also compiled on the CPU).
//
// raycast_kernel<FORM>: one 512-thread workgroup per (robot, slice of the robot's points), a lane
// per ray.  A slice is a multiple of 64 points, so a wave's rays are neighbours in the revolution
// and of similar length.  The walk carries the ray's remainders and the squared radius along
// (grid_walk_next): no division and no multiplication of offsets per step.
//   FORM 1 (HBM), which ships: the code is taken from the int16 cell in HBM as the walk reaches it,
//     bounds tested.  It reads only the cells that rays touch, a few sectors per ray in a room.
//   FORM 0 (LDS), LSLAM_RAYCAST_FORM=lds: a walk reads only cells with ox^2 + oy^2 <= Rc^2, the window
//     of 2 Rc + 1 cells a side around the robot cell.  The workgroup loads that window, clipped to the
//     map, as 2-bit codes (0 unknown, 1 free, 2 occupied), 16 cells to a dword, with an apron of one
//     unknown cell on every side: a ray moves one cell a step, so it meets the apron before it can
//     leave the loaded rectangle, and the walk needs no bounds test.  Rows have an odd number of
//     dwords, so that the lanes of a wave walking along a column fall on different banks.  With rows
//     of the map on 16-byte boundaries a lane loads 8 cells (a wave takes rows of the window, four
//     of them in flight: 64 lanes x 8 cells is a 512-cell row), thresholds them to 16 bits and ORs
//     them into the one or two dwords they straddle; otherwise a lane per cell.  A step is then one
//     ds_read_b32, a shift and the cap test.  At the defaults (Rc = 400, a 512-cell map) the codes
//     are 514 rows of 33 dwords: 67,856 B + 32 B of counters, two workgroups to a CU's 160 KiB, 16
//     waves per CU.  It fits while min(2 Rc + 1, grid_w) <= 558 (RAYCAST_LDS_BUDGET); beyond, the HBM
//     form runs whatever is asked for.  Measured 4 % slower than the HBM form at 4096 robots in the
//     bench room, where a ray walks 75 steps and the window is 512 KiB: DESIGN.md §4.4, §5.
// A robot cell off the map stops every ray at step 0 (unknown); nothing is loaded then.
// counts: per round a ballot per counter, the wave's first lane adds the popcounts to LDS, and at the
// end the workgroup adds its seven sums to the zeroed counts[r] (global atomicAdd: integers, any order).
// rot and flags are written by the robot's slice 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_grid.h"
#include "lslam_mapmatch.h"
#include "lslam_raycast_walk.h"
#include "lslam_wave.h"

namespace lslam {

constexpr int RAYCAST_TPB = 512;
constexpr int RAYCAST_LDS_BUDGET = 80 * 1024;  // two workgroups to a CU
constexpr int RAYCAST_MAX_SLICES = 16;

struct RaycastArgs {
    lslam_raycast_batch b;
    double inv, max_r2, far;
    int grid_w, Rc, occ_min, free_max, tol;
    int n_slices;  // workgroups per robot
    int vec;       // rows of logodds lie on 16-byte boundaries
    int Sd;        // dwords per row of the codes in LDS
};

// cells a side of the largest window a robot can have
static inline int raycast_window(int Rc, int grid_w) { return 2 * Rc + 1 < grid_w ? 2 * Rc + 1 : grid_w; }
// dwords per row of a window of win cells with its apron: odd
static inline int raycast_row_dwords(int win) { return ((win + 2 + 15) >> 4) | 1; }
// LDS bytes: eight counters, then the codes
static inline int raycast_lds_bytes(int win) { return 32 + (((win + 2) * raycast_row_dwords(win) * 4 + 15) & ~15); }

// bits 2j, 2j + 1 of the result: the code of cell j of a 16-byte group of eight int16 cells
__device__ __forceinline__ uint32_t raycast_code8(uint4 v, int occ_min, int free_max) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int l0 = (int)(int16_t)(d[i] & 0xffffu), l1 = (int)d[i] >> 16;  // (the low half is the lower address)
        m |= (uint32_t)raycast_code(l0, occ_min, free_max) << (4 * i);
        m |= (uint32_t)raycast_code(l1, occ_min, free_max) << (4 * i + 2);
    }
    return m;
}

// the codes in LDS; (bx, by): the robot cell's column and row there
struct RaycastLdsMap {
    const uint32_t *G;
    int bx, by, Sd;
    bool on;  // the robot cell lies on the map
    __device__ __forceinline__ int operator()(int ox, int oy) const {
        if (!on) return RAYCAST_UNKNOWN;
        const int col = bx + ox, row = by + oy;
        return (int)((G[row * Sd + (col >> 4)] >> ((col & 15) * 2)) & 3u);
    }
};

// the robot's grid in HBM
struct RaycastHbmMap {
    const int16_t *L;
    int X0, Y0, W, occ_min, free_max;
    __device__ __forceinline__ int operator()(int ox, int oy) const {
        const int X = X0 + ox, Y = Y0 + oy;
        if ((unsigned)X >= (unsigned)W || (unsigned)Y >= (unsigned)W) return RAYCAST_UNKNOWN;
        return raycast_code((int)L[(int64_t)Y * W + X], occ_min, free_max);
    }
};

template <class Map>
__device__ __forceinline__ void raycast_points(const RaycastArgs &a, const RaycastPose &rp, const Map &map, int s0, int s1,
                                               int *cnt) {
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const double2 *xy = (const double2 *)a.b.xy;
    for (int t0 = s0; t0 < s1; t0 += RAYCAST_TPB) {
        const int p = t0 + tid;
        int cl = -1, ox = 0, oy = 0, ih = 0;
        bool beyond = false;
        if (p < s1) {
            const double2 q = xy[p];
            cl = 0;
            if (grid_valid(q)) cl = raycast_point(rp, q.x, q.y, a.max_r2, a.far, a.Rc, a.tol, map, ox, oy, ih, beyond);
            a.b.cls[p] = (uint8_t)cl;
            if (a.b.stop) {
                int32_t *st = a.b.stop + 3 * (int64_t)p;
                st[0] = ox;
                st[1] = oy;
                st[2] = ih;
            }
        }
        const int c = cl & 15;  // (15 for a lane without a point)
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const bool mine = k < 5 ? c == k : (k == 5 ? beyond : (cl > 0 && (cl >> 4) == RAYCAST_K_NONE));
            const uint64_t bk = ballot(mine);
            if (lane == 0 && bk) atomicAdd(&cnt[k], popc64(bk));
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(RAYCAST_TPB) void raycast_kernel(const RaycastArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *cnt = (int *)smem;  // [8]: classes 0..4, beyond, kind NONE, unused
    uint32_t *G = (uint32_t *)(smem + 32);
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ns = a.n_slices;
    const int r = (int)blockIdx.x / ns, slice = (int)blockIdx.x - r * ns;
    const bool first = slice == 0;  // the robot's workgroup that writes rot and flags

    // ---- 0. pose and rotation ----
    RaycastPose rp;
    rp.px = a.b.pose[3 * r];
    rp.py = a.b.pose[3 * r + 1];
    const double th = a.b.pose[3 * r + 2];
    rp.ox = a.b.origin[2 * r];
    rp.oy = a.b.origin[2 * r + 1];
    rp.inv = a.inv;
    rp.c = cos(th);
    rp.s = sin(th);
    if (first && tid == 0) {
        a.b.rot[2 * r] = rp.c;
        a.b.rot[2 * r + 1] = rp.s;
    }
    // the slice's points [s0, s1): a multiple of 64 of them but for the robot's last
    const int p0 = a.b.pt_off[r], p1 = a.b.pt_off[r + 1];
    const int per = (int)((((int64_t)(p1 - p0) + ns - 1) / ns + 63) & ~(int64_t)63);
    const int64_t s0l = (int64_t)p0 + (int64_t)slice * per;
    const int s0 = (int)(s0l < p1 ? s0l : p1), s1 = (int)(s0l + per < p1 ? s0l + per : p1);
    if (!mapmatch_robot_cell(rp.px, rp.py, th, rp.ox, rp.oy, rp.inv, rp.X0d, rp.Y0d)) {
        if (first && tid == 0) a.b.flags[r] = LSLAM_RAYCAST_BAD_POSE;
        for (int p = s0 + tid; p < s1; p += RAYCAST_TPB) {
            a.b.cls[p] = 0;
            if (a.b.stop) {
                int32_t *st = a.b.stop + 3 * (int64_t)p;
                st[0] = st[1] = st[2] = 0;
            }
        }
        return;
    }
    if (first && tid == 0) a.b.flags[r] = 0;
    if (s0 >= s1) return;  // (counts[r] is zeroed by the launcher)
    const int X0 = (int)rp.X0d, Y0 = (int)rp.Y0d;
    const int W = a.grid_w;
    const int16_t *L = a.b.logodds + (int64_t)r * W * W;
    if (tid < 8) cnt[tid] = 0;

    if (FORM == 0) {
        const int Rc = a.Rc, Sd = a.Sd;
        RaycastLdsMap map;
        map.G = G;
        map.Sd = Sd;
        map.on = (unsigned)X0 < (unsigned)W && (unsigned)Y0 < (unsigned)W;
        map.bx = map.by = 0;
        if (map.on) {
            // the window's cells on the map: at most raycast_window() a side
            const int mx0 = max(0, X0 - Rc), mx1 = min(W, X0 + Rc + 1);
            const int my0 = max(0, Y0 - Rc), my1 = min(W, Y0 + Rc + 1);
            const int nrows = my1 - my0;
            map.bx = X0 - mx0 + 1;
            map.by = Y0 - my0 + 1;
            uint4 *G4 = (uint4 *)G;
            for (int i = tid; i < ((nrows + 2) * Sd + 3) / 4; i += RAYCAST_TPB) G4[i] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            const int occ_min = a.occ_min, free_max = a.free_max;
            if (a.vec) {
                const int g0 = mx0 >> 3, ng = ((mx1 + 7) >> 3) - g0;  // map-aligned groups of 8 cells
                constexpr int NW = RAYCAST_TPB / 64, UN = 4;  // a wave keeps UN rows' loads in flight
                for (int gi = lane; gi < ng; gi += 64) {
                    const int cx = 8 * (g0 + gi);
                    const int cut_lo = max(0, mx0 - cx), cut_hi = min(8, mx1 - cx);  // the group's cells in the window
                    const uint32_t keep = ~((1u << (2 * cut_lo)) - 1u) & ((1u << (2 * cut_hi)) - 1u);
                    const int lc0 = cx - mx0 + 1;  // column in LDS of the group's first cell
                    const int shr = lc0 < 0 ? 2 * (-lc0) : 0, lc = max(lc0, 0);  // (its cells left of the window are cleared)
                    for (int row0 = wv; row0 < nrows; row0 += NW * UN) {
                        uint4 v[UN];
#pragma unroll
                        for (int j = 0; j < UN; j++) {
                            const int row = min(row0 + NW * j, nrows - 1);
                            v[j] = *(const uint4 *)(L + (int64_t)(my0 + row) * W + cx);
                        }
#pragma unroll
                        for (int j = 0; j < UN; j++) {
                            const int row = row0 + NW * j;
                            const uint32_t m = (raycast_code8(v[j], occ_min, free_max) & keep) >> shr;
                            if (row >= nrows || !m) continue;
                            const uint64_t w = (uint64_t)m << ((lc & 15) * 2);
                            uint32_t *gd = G + (row + 1) * Sd + (lc >> 4);
                            if ((uint32_t)w) atomicOr(gd, (uint32_t)w);
                            if ((uint32_t)(w >> 32)) atomicOr(gd + 1, (uint32_t)(w >> 32));  // (a set bit there is a cell of this row)
                        }
                    }
                }
            } else {
                for (int row = wv; row < nrows; row += RAYCAST_TPB / 64) {
                    const int16_t *Lr = L + (int64_t)(my0 + row) * W;
                    uint32_t *Gr = G + (row + 1) * Sd;
                    for (int cx = mx0 + lane; cx < mx1; cx += 64) {
                        const int code = raycast_code((int)Lr[cx], occ_min, free_max);
                        const int lc = cx - mx0 + 1;
                        if (code) atomicOr(Gr + (lc >> 4), (uint32_t)code << ((lc & 15) * 2));
                    }
                }
            }
        }
        __syncthreads();
        raycast_points(a, rp, map, s0, s1, cnt);
    } else {
        __syncthreads();
        const RaycastHbmMap map = {L, X0, Y0, W, a.occ_min, a.free_max};
        raycast_points(a, rp, map, s0, s1, cnt);
    }
    __syncthreads();
    if (tid < 7 && cnt[tid]) atomicAdd(&a.b.counts[8 * r + tid], cnt[tid]);
}

}  // namespace lslam
