// lslam_page.h — the paged rolling grid: behind each robot's W x W window a canvas of Cw x Cw log-odds.
// A recentre writes the strip that leaves the window to the canvas and reads the strip that enters
// from it; flush and load copy the whole window.  The definition is the comment on
// lslam_grid_recentre_paged in include/lidarslam.h; tests/page_ref.py is its NumPy form; the strips and
// their clipping to the canvas are lslam_page_plan.h.
//
// page_recentre_kernel<CELLS>: one 256-thread workgroup per robot, as recentre_kernel and for its
// reason; the decision and the in-place shift are that kernel's own device functions
// (recentre_decide, recentre_move), so there is one text of each.
//   0. the decision.  A robot that does not move writes its outputs and ends here: it has read the
//      40 bytes of pose and origin and nothing else.
//   1. store: the leaving strips, clipped to the canvas, window -> canvas.
//   2. recentre_move.  Its first barrier stands behind every load of pass 1 (a thread's canvas stores
//      waited for their data), so no band is stored over a cell that pass 1 has yet to read.
//   3. a barrier (with vmcnt(0) in front, as in recentre_move): the zeros that the bands stored into
//      the entering cells are written, in every wave, before pass 4 stores to those cells.
//   4. load: the entering strips, clipped to the canvas where the window now lies, canvas -> window.
//      What is off the canvas keeps the zero of pass 2.
//   5. thread 0 writes win, moved, the page flags and the origin; every thread read win before pass 2.
// The leaving cells lie in the old window and not in the new one, the entering cells the reverse: no
// canvas cell is both stored and loaded in one call.
//
// A strip is copied on one of two paths, chosen per robot.  16-byte groups where the window's rows,
// the canvas' rows, the strip's columns and the window's place on the canvas are all on groups of 8
// cells (grid_w, canvas_w, sx and wx multiples of 8, both pointers 16-byte aligned: the defaults).
// Otherwise a lane per cell.  Either way the strip's cells are numbered row after row and a thread
// takes every 256th, eight at a time: loads first, then stores.  The vertical strip is |sx| cells wide
// (4 groups at sx = 32), so a wave covers 16 of its rows at once, not a sixteenth of one; at the
// defaults either strip of a (32, 16) shift is one round of loads and one of stores.  Nothing is
// kept between the passes and nothing is shared: no LDS.
//
// page_window_kernel<STORE>: flush (STORE) and load, the whole window.  A robot's rows are cut into
// slices, a workgroup each, so that a small fleet still fills the chip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_page_plan.h"
#include "lslam_recentre.h"

namespace lslam {

constexpr int PAGE_TPB = RECENTRE_TPB;
constexpr int PAGE_UNROLL = 8;  // cells or groups a thread has in flight, as a band's (RECENTRE_VPT)

// The kernel's arguments, flat and without padding: 120 bytes, inside two 64-byte lines of the
// argument segment (the recentre's arguments with the page batch behind them would be 136).
struct PageArgs {
    const double *pose;  // the recentre batch
    double *origin;
    int16_t *logodds;
    int32_t *shift, *flags;
    int16_t *canvas;  // the page batch
    int32_t *win, *moved, *pflags;
    double cell, inv;
    int n_robots, grid_w, margin, quantum;
    int band_rows;  // recentre_band_rows(grid_w)
    int vec;        // rows of logodds lie on 16-byte boundaries
    int canvas_w;
    int pvec;       // vec, and the canvas' rows do too (canvas_w a multiple of 8, canvas aligned)
};

// what recentre_decide and recentre_move take (registers: nothing is copied)
__device__ __forceinline__ RecentreArgs page_recentre_args(const PageArgs &a) {
    RecentreArgs r;
    r.b.n_robots = a.n_robots;
    r.b.reserved = 0;
    r.b.pose = a.pose;
    r.b.origin = a.origin;
    r.b.logodds = a.logodds;
    r.b.shift = a.shift;
    r.b.flags = a.flags;
    r.cell = a.cell;
    r.inv = a.inv;
    r.grid_w = a.grid_w;
    r.margin = a.margin;
    r.quantum = a.quantum;
    r.band_rows = a.band_rows;
    r.vec = a.vec;
    return r;
}

// Rectangle q of window cells (all on the canvas: page_clip's) between the window L, rows of W cells,
// and the canvas Cv, rows of Cw cells, whose cell (ox, oy) is window cell (0, 0).  STORE: window ->
// canvas; else canvas -> window.  T = uint4: q's columns and ox are multiples of 8 and the unit is a
// group of 8 cells; T = uint16_t: a cell.  Thread tid of nthreads.
template <typename T, bool STORE>
__device__ __forceinline__ void page_copy_rect(int16_t *__restrict__ L, int16_t *__restrict__ Cv, int W, int Cw, const PageRect q,
                                               int64_t ox, int64_t oy, int tid, int nthreads) {
    constexpr int U = (int)(sizeof(T) / 2);  // cells per unit
    const int nu = (q.x1 - q.x0) / U, n = nu * (q.y1 - q.y0);
    if (n <= 0) return;
    // (on the canvas: 0 <= oy + y < Cw and 0 <= ox + x < Cw for every cell of q, so the offsets fit 32 bits)
    const int cx0 = (int)(ox + q.x0), cy0 = (int)(oy + q.y0);
    for (int i0 = tid; i0 < n; i0 += nthreads * PAGE_UNROLL) {
        T v[PAGE_UNROLL];
        int to[PAGE_UNROLL];  // (a window and a canvas hold at most 2^22 cells)
#pragma unroll
        for (int j = 0; j < PAGE_UNROLL; j++) {
            const int i = i0 + j * nthreads;
            const int row = (i < n ? i : 0) / nu, c = (i < n ? i : 0) - row * nu;
            const int w = (q.y0 + row) * W + q.x0 + c * U, cv = (cy0 + row) * Cw + cx0 + c * U;
            v[j] = *(const T *)((STORE ? L : Cv) + (STORE ? w : cv));
            to[j] = STORE ? cv : w;
        }
#pragma unroll
        for (int j = 0; j < PAGE_UNROLL; j++)
            if (i0 + j * nthreads < n) *(T *)((STORE ? Cv : L) + to[j]) = v[j];
    }
}

// both strips of s, clipped to the canvas; returns the cells copied (uniform over the workgroup)
template <bool STORE>
__device__ __forceinline__ int page_copy_strips(int16_t *L, int16_t *Cv, int W, int Cw, const PageStrips s, int64_t ox, int64_t oy,
                                                bool groups, int tid) {
    const PageRect h = page_clip(s.h, ox, oy, Cw), v = page_clip(s.v, ox, oy, Cw);
    if (groups) {
        page_copy_rect<uint4, STORE>(L, Cv, W, Cw, h, ox, oy, tid, PAGE_TPB);
        page_copy_rect<uint4, STORE>(L, Cv, W, Cw, v, ox, oy, tid, PAGE_TPB);
    } else {
        page_copy_rect<uint16_t, STORE>(L, Cv, W, Cw, h, ox, oy, tid, PAGE_TPB);
        page_copy_rect<uint16_t, STORE>(L, Cv, W, Cw, v, ox, oy, tid, PAGE_TPB);
    }
    return page_area(h) + page_area(v);
}

// passes 1 to 5 for a robot that moves
template <int CELLS>
__device__ __forceinline__ void page_move(const PageArgs a, const RecentreArgs ra, const RecentreDecision d, int r, int tid) {
    const int W = a.grid_w, Cw = a.canvas_w, sx = d.sx, sy = d.sy;
    const int64_t wx = a.win[2 * r], wy = a.win[2 * r + 1];
    int16_t *L = a.logodds + (int64_t)r * W * W;
    int16_t *Cv = a.canvas + (int64_t)r * Cw * Cw;
    const bool groups = a.pvec && ((sx | (int)wx) & 7) == 0;

    // ---- 1. store the strip that leaves ----
    const PageStrips out = page_leaving(W, sx, sy);
    const int stored = page_copy_strips<true>(L, Cv, W, Cw, out, wx, wy, groups, tid);
    const int left = page_area(out.h) + page_area(out.v);

    // ---- 2. the grid, band after band ----
    recentre_move<CELLS>(ra, L, sx, sy, tid);

    // ---- 3. the bands' zeros are in memory before the entering cells are stored again ----
    // (the barrier's own workgroup-scope fence orders them; the explicit vmcnt(0) is recentre_move's
    // idiom kept beside it, belt and braces)
    __builtin_amdgcn_s_waitcnt(0x0f70);
    __syncthreads();

    // ---- 4. load the strip that enters ----
    const int loaded = page_copy_strips<false>(L, Cv, W, Cw, page_entering(W, sx, sy), wx + sx, wy + sy, groups, tid);

    // ---- 5. the robot's outputs ----
    if (tid == 0) {
        a.win[2 * r] = (int32_t)(wx + sx);
        a.win[2 * r + 1] = (int32_t)(wy + sy);
        a.moved[2 * r] = stored;
        a.moved[2 * r + 1] = loaded;
        a.pflags[r] = stored < left ? LSLAM_PAGE_LOST : 0;
        a.origin[2 * r] = d.nox;
        a.origin[2 * r + 1] = d.noy;
    }
}

// At most 80 scalar registers.  Left alone the compiler takes 100, which it counts as eight waves a
// SIMD; measured, 4096 robots at rest then take 0.0076 ms against the plain call's 0.0068 ms, and a
// build that only lacks the moving path 0.0071 ms.  Held to 80 (24 scalars parked in lanes of one
// vector register, 63 in all): 0.0070 to 0.0073 ms beside 0.0068 to 0.0071 ms.
// tests/test_page_budget.py holds the counts.  The compiler follows the bound for CELLS = 0, the
// instantiation of the defaults; CELLS = 1 keeps its 101, behind the 32 KiB of LDS that hold it to
// five workgroups a CU in any case.
template <int CELLS>
__attribute__((amdgpu_num_sgpr(80))) __global__ __launch_bounds__(PAGE_TPB) void page_recentre_kernel(const PageArgs a) {
    const int tid = (int)threadIdx.x, r = recentre_robot_of_block((int)blockIdx.x);
    if (r >= a.n_robots) return;  // (the grid is padded to whole groups of 8 blocks)

    // ---- 0. the decision ----
    const RecentreArgs ra = page_recentre_args(a);
    const RecentreDecision d = recentre_decide(ra, r);
    if (tid == 0) {
        a.shift[2 * r] = d.sx;
        a.shift[2 * r + 1] = d.sy;
        a.flags[r] = d.flag;
    }
    if (!(d.sx | d.sy)) {  // (uniform)
        if (tid == 0) {
            a.moved[2 * r] = 0;
            a.moved[2 * r + 1] = 0;
            a.pflags[r] = 0;
        }
        return;
    }
    page_move<CELLS>(a, ra, d, r, tid);
}

struct PageWindowArgs {
    lslam_page_batch pg;
    int16_t *logodds;
    int grid_w, canvas_w;
    int vec;       // as PageArgs.pvec
    int n_slices;  // workgroups per robot
    int rows;      // window rows per slice
};

// Flush (STORE) and load.  Workgroup = (robot, slice): the slice's rows of the window.  A load writes
// every cell of them, zero where the cell is off the canvas; on the 16-byte path a group is on the
// canvas whole or not at all.
template <bool STORE>
__global__ __launch_bounds__(PAGE_TPB) void page_window_kernel(const PageWindowArgs a) {
    const int tid = (int)threadIdx.x;
    const int r = (int)(blockIdx.x / (unsigned)a.n_slices), sl = (int)(blockIdx.x % (unsigned)a.n_slices);
    const int W = a.grid_w, Cw = a.canvas_w;
    const int64_t wx = a.pg.win[2 * r], wy = a.pg.win[2 * r + 1];
    int16_t *L = a.logodds + (int64_t)r * W * W;
    int16_t *Cv = a.pg.canvas + (int64_t)r * Cw * Cw;
    const bool groups = a.vec && ((int)wx & 7) == 0;
    const PageRect all = page_clip(PageRect{0, W, 0, W}, wx, wy, Cw);
    if (sl == 0 && tid == 0) {
        a.pg.moved[2 * r] = STORE ? page_area(all) : 0;
        a.pg.moved[2 * r + 1] = STORE ? 0 : page_area(all);
    }
    const int y0 = sl * a.rows, y1 = y0 + a.rows < W ? y0 + a.rows : W;
    if (y0 >= y1) return;
    const PageRect mine = page_clip(PageRect{0, W, y0, y1}, wx, wy, Cw);
    if constexpr (!STORE) {
        // the slice's cells off the canvas: zero.  Its rows are contiguous in the window
        if (page_area(mine) < (y1 - y0) * W) {
            if (groups) {
                uint4 *L4 = (uint4 *)(L + (int64_t)y0 * W);
                const int W8 = W >> 3, n = (y1 - y0) * W8;
                for (int i = tid; i < n; i += PAGE_TPB) {
                    const int row = i / W8, x = (i - row * W8) << 3, y = y0 + row;
                    if (!(y >= mine.y0 && y < mine.y1 && x >= mine.x0 && x < mine.x1)) L4[i] = make_uint4(0u, 0u, 0u, 0u);
                }
            } else {
                const int n = (y1 - y0) * W;
                for (int i = tid; i < n; i += PAGE_TPB) {
                    const int row = i / W, x = i - row * W, y = y0 + row;
                    if (!(y >= mine.y0 && y < mine.y1 && x >= mine.x0 && x < mine.x1)) L[(int64_t)y0 * W + i] = 0;
                }
            }
        }
    }
    if (groups) page_copy_rect<uint4, STORE>(L, Cv, W, Cw, mine, wx, wy, tid, PAGE_TPB);
    else page_copy_rect<uint16_t, STORE>(L, Cv, W, Cw, mine, wx, wy, tid, PAGE_TPB);
}

}  // namespace lslam
