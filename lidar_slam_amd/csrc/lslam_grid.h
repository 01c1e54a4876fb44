// lslam_grid.h — batched occupancy-grid mapping: one revolution per robot and the robot's pose ->
// clamped log-odds of its grid.  The definition (pose, points, integer ray, per-revolution sum, one
// clamp per call) is the comment on lslam_grid_update in include/lidarslam.h; tests/occgrid_ref.py
// is its NumPy form; the integer ray and its clip to a tile are lslam_grid_ray.h.
//
// grid_update_kernel<T, WAVE_RAY>: one 256-thread workgroup per (robot, tile of T x T cells).
//   LDS: the tile's per-revolution sum D as int32 [T][T] (16 KiB at T = 64, which ships; 64 KiB at
//   T = 128, two workgroups to a CU's 160 KiB), one staged list of 256 clipped rays (int4: dx, dy,
//   first and last step inside the tile; 4 KiB) and four counters: 20,496 B.
//   1. every workgroup of a robot computes (cos, sin) of the heading with the same instructions, so
//      all of them hold the bits that the robot's first workgroup writes to rot;
//   2. the robot's points are walked in staged tiles of 256, one point per thread: validity, range,
//      the hit cell, then grid_ray_clip gives the steps of the ray inside this tile.  Rays with
//      some are compacted into the list (a ballot and one LDS atomicAdd per wave);
//   3. a lane takes a ray of the list and walks its steps inside the tile, each an LDS atomicAdd of
//      l_miss (l_hit at step n) into D; the offsets come from grid_walk_next, which carries the
//      closed form's remainder along instead of dividing per step (one division per ray and axis).
//      (WAVE_RAY, measured and dropped: a wave per ray, its lanes over the steps, 64 at a time.
//      Inside a tile a ray has at most T steps, usually far fewer, so most lanes idle, and the
//      per-ray set-up, an LDS read and the divisions by 2n, is paid by a whole wave: 8.6 ms against
//      3.6 ms for 4096 robots);
//   4. after a barrier the tile's cells with D != 0 get L' = clamp(L + D): with rows on 16-byte
//      boundaries (grid_w a multiple of 8) a thread owns 8 cells, reads their D first and touches
//      HBM (one 16-byte load and store) only if one of them is non-zero; otherwise a thread per cell.
//   D is zeroed when the first ray reaches the tile, so a tile that no ray reaches costs neither LDS
//   traffic nor HBM traffic: the workgroup ends after the point walk.
//   The robot's first workgroup also tallies n_used and the CLIPPED flag.
// Measured against T = 128 and against a wave per ray: DESIGN.md §4.4 (tools/gridbench.py; the
// LSLAM_GRID_FORM environment variable selects the other instantiations for that tool).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_grid_ray.h"
#include "lslam_wave.h"

namespace lslam {

constexpr int GRID_TPB = 256;    // threads per workgroup
constexpr int GRID_STAGE = 256;  // points staged per tile of the point walk: one per thread
constexpr int GRID_T = 64;       // tile side that ships
constexpr int GRID_WAVE_RAY = 0; // a lane per ray ships

struct GridArgs {
    lslam_grid_batch b;
    double inv, max_r2;
    int grid_w, l_hit, l_miss, l_min, l_max;
    int ntile;  // tiles a side
    int vec;    // rows of logodds lie on 16-byte boundaries
};

static inline int grid_lds_bytes(int T) { return T * T * 4 + GRID_STAGE * 16 + 16; }

__device__ __forceinline__ bool grid_valid(double2 q) {
    return __builtin_isfinite(q.x) && __builtin_isfinite(q.y) && !(q.x == 0.0 && q.y == 0.0);
}

// step 4 for one cell: clamp(L + D) = clamp(L + clamp(D, +-65535)), in int32
__device__ __forceinline__ int grid_apply(int l, int d, int lmin, int lmax) {
    if (d == 0) return l;
    d = min(max(d, -65535), 65535);
    return min(max(l + d, lmin), lmax);
}
// two cells packed in a dword (the low half is the lower address)
__device__ __forceinline__ uint32_t grid_apply2(uint32_t v, int d0, int d1, int lmin, int lmax) {
    const int l0 = (int)(int16_t)(v & 0xffffu), l1 = (int)(int16_t)(v >> 16);
    const uint32_t r0 = (uint32_t)grid_apply(l0, d0, lmin, lmax) & 0xffffu;
    const uint32_t r1 = (uint32_t)grid_apply(l1, d1, lmin, lmax) & 0xffffu;
    return r0 | (r1 << 16);
}

template <int T, int WAVE_RAY>
__global__ __launch_bounds__(GRID_TPB) void grid_update_kernel(const GridArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *D = (int *)smem;
    int4 *stage = (int4 *)(smem + T * T * 4);
    int *cnt = (int *)(stage + GRID_STAGE);  // [0] rays in the list; [1], [2] n_used; [3] a hit cell outside
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int W = a.grid_w, nt = a.ntile, nt2 = nt * nt;
    const int r = (int)blockIdx.x / nt2, tile = (int)blockIdx.x - r * nt2;
    const int tyi = tile / nt, txi = tile - tyi * nt;
    const bool first = tile == 0;  // the robot's workgroup that writes rot, n_used, flags

    // ---- 0. pose and rotation ----
    const double px = a.b.pose[3 * r], py = a.b.pose[3 * r + 1], th = a.b.pose[3 * r + 2];
    const double ox = a.b.origin[2 * r], oy = a.b.origin[2 * r + 1];
    const double inv = a.inv;
    const double c = cos(th), s = sin(th);
    if (first && tid == 0) {
        a.b.rot[2 * r] = c;
        a.b.rot[2 * r + 1] = s;
    }
    const double X0d = floor((px - ox) * inv), Y0d = floor((py - oy) * inv);
    const bool finite5 = __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(th) &&
                         __builtin_isfinite(ox) && __builtin_isfinite(oy);
    if (!(finite5 && fabs(X0d) < 1048576.0 && fabs(Y0d) < 1048576.0)) {
        if (first && tid == 0) {
            a.b.flags[r] = LSLAM_GRID_BAD_POSE;
            a.b.n_used[2 * r] = 0;
            a.b.n_used[2 * r + 1] = 0;
        }
        return;
    }
    const int X0 = (int)X0d, Y0 = (int)Y0d;
    const int tx0 = txi * T, ty0 = tyi * T, tx1 = min(W, tx0 + T), ty1 = min(W, ty0 + T);
    const int p0 = a.b.pt_off[r], p1 = a.b.pt_off[r + 1];
    const double2 *xy = (const double2 *)a.b.xy;
    const int l_hit = a.l_hit, l_miss = a.l_miss;
    if (tid < 4) cnt[tid] = 0;

    // ---- 1-3. points -> rays clipped to the tile -> D ----
    int used = 0, far = 0, out = 0;
    bool zeroed = false;
    for (int t0 = p0; t0 < p1; t0 += GRID_STAGE) {
        __syncthreads();  // the previous list's readers are done
        if (tid == 0) cnt[0] = 0;
        __syncthreads();
        const int p = t0 + tid;
        bool in = false;
        int dx = 0, dy = 0, ilo = 0, ihi = 0;
        if (p < p1) {
            const double2 q = xy[p];
            if (grid_valid(q)) {
                if (q.x * q.x + q.y * q.y > a.max_r2) {
                    far++;
                } else {
                    used++;
                    const double wx = px + (c * q.x - s * q.y);
                    const double wy = py + (s * q.x + c * q.y);
                    // within max_range / cell + 1 <= 4097 cells of the robot cell: the conversions cannot overflow
                    const int X1 = (int)floor((wx - ox) * inv), Y1 = (int)floor((wy - oy) * inv);
                    if ((unsigned)X1 >= (unsigned)W || (unsigned)Y1 >= (unsigned)W) out = 1;
                    dx = X1 - X0;
                    dy = Y1 - Y0;
                    in = grid_ray_clip(X0, Y0, dx, dy, tx0, ty0, tx1, ty1, ilo, ihi);
                }
            }
        }
        const uint64_t bin = ballot(in);
        int base = 0;
        if (lane == 0 && bin) base = atomicAdd(&cnt[0], popc64(bin));
        base = uni(base);
        if (in) stage[base + (int)mbcnt(bin)] = make_int4(dx, dy, ilo, ihi);
        __syncthreads();
        const int nl = cnt[0];
        if (nl == 0) continue;
        if (!zeroed) {  // the first ray to reach this tile
            int4 *D4 = (int4 *)D;
            for (int i = tid; i < T * T / 4; i += GRID_TPB) D4[i] = make_int4(0, 0, 0, 0);
            __syncthreads();
            zeroed = true;
        }
        if (WAVE_RAY) {
            for (int j = wv; j < nl; j += GRID_TPB / 64) {
                const int4 e = stage[j];
                const int ax = grid_iabs(e.x), ay = grid_iabs(e.y), sx = grid_sgn(e.x), sy = grid_sgn(e.y);
                const int n = max(ax, ay);
                const int bx = X0 - tx0, by = Y0 - ty0;
                for (int i = e.z + lane; i <= e.w; i += 64) {
                    const int cx = bx + sx * grid_ray_offset(i, ax, n), cy = by + sy * grid_ray_offset(i, ay, n);
                    atomicAdd(&D[cy * T + cx], i == n ? l_hit : l_miss);
                }
            }
        } else {
            for (int j = tid; j < nl; j += GRID_TPB) {
                const int4 e = stage[j];
                const int ax = grid_iabs(e.x), ay = grid_iabs(e.y), sx = grid_sgn(e.x), sy = grid_sgn(e.y);
                const int n = max(ax, ay);
                const int bx = X0 - tx0, by = Y0 - ty0;
                GridAxisWalk wx = grid_walk_begin(e.z, ax, n), wy = grid_walk_begin(e.z, ay, n);
                for (int i = e.z; i <= e.w; i++) {
                    const int cx = bx + sx * wx.off, cy = by + sy * wy.off;
                    atomicAdd(&D[cy * T + cx], i == n ? l_hit : l_miss);
                    grid_walk_next(wx);
                    grid_walk_next(wy);
                }
            }
        }
    }
    __syncthreads();  // D is complete (and cnt[1..3] are zero when the robot has no points)

    if (first) {
        if (used) atomicAdd(&cnt[1], used);
        if (far) atomicAdd(&cnt[2], far);
        if (out) atomicOr(&cnt[3], 1);
        __syncthreads();
        if (tid == 0) {
            const int nu = cnt[1];
            const bool robot_out = (unsigned)X0 >= (unsigned)W || (unsigned)Y0 >= (unsigned)W;
            a.b.n_used[2 * r] = nu;
            a.b.n_used[2 * r + 1] = cnt[2];
            a.b.flags[r] = (cnt[3] || (nu > 0 && robot_out)) ? LSLAM_GRID_CLIPPED : 0;
        }
    }
    if (!zeroed) return;  // no ray reaches this tile: its cells are neither read nor written

    // ---- 4. L' = clamp(L + D) where D != 0 ----
    const int h = ty1 - ty0, w = tx1 - tx0;
    const int lmin = a.l_min, lmax = a.l_max;
    int16_t *L = a.b.logodds + ((int64_t)r * W + ty0) * W + tx0;
    if (a.vec) {
        constexpr int C8 = T / 8;
        for (int idx = tid; idx < h * C8; idx += GRID_TPB) {
            const int row = idx / C8, c8 = idx - row * C8;
            if (c8 * 8 >= w) continue;  // (w is a multiple of 8 here)
            const int4 d0 = *(const int4 *)&D[row * T + c8 * 8], d1 = *(const int4 *)&D[row * T + c8 * 8 + 4];
            if (!(d0.x | d0.y | d0.z | d0.w | d1.x | d1.y | d1.z | d1.w)) continue;
            uint4 *g = (uint4 *)(L + (int64_t)row * W + c8 * 8);
            uint4 v = *g;
            v.x = grid_apply2(v.x, d0.x, d0.y, lmin, lmax);
            v.y = grid_apply2(v.y, d0.z, d0.w, lmin, lmax);
            v.z = grid_apply2(v.z, d1.x, d1.y, lmin, lmax);
            v.w = grid_apply2(v.w, d1.z, d1.w, lmin, lmax);
            *g = v;
        }
    } else {
        for (int idx = tid; idx < h * T; idx += GRID_TPB) {
            const int row = idx / T, col = idx - row * T;
            const int d = D[idx];
            if (col >= w || d == 0) continue;
            int16_t *g = L + (int64_t)row * W + col;
            *g = (int16_t)grid_apply((int)*g, d, lmin, lmax);
        }
    }
}

}  // namespace lslam
