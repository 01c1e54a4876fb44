// lslam_grid_ray.h — the integer ray of the occupancy-grid update (lslam_grid_update, step 2 of its
// definition in include/lidarslam.h) and its clip to a tile.  Plain C++, no HIP: the kernels of
// lslam_grid.h and a CPU program (tests/test_grid_ray.py) compile this same text.
//
// A ray runs from the robot cell (X0, Y0) to the hit cell (X0 + dx, Y0 + dy) in n = max(|dx|, |dy|)
// steps.  Step i = 0 .. n-1 is a free cell, step n the hit cell: with a = |d| along an axis the
// offset at step i is (2 i a + n) div 2n, which is a at i = n, so one closed form covers both.
// Every step is independent of the others; along the major axis (a = n) the offset is i itself,
// along the minor one it is monotone in i.  |dx|, |dy| <= 4100 (max_range / cell <= 4096) keeps
// every product below 2^27.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSLAM_GRID_HD __host__ __device__
#else
#define LSLAM_GRID_HD
#endif

LSLAM_GRID_HD static inline int grid_iabs(int v) { return v < 0 ? -v : v; }
LSLAM_GRID_HD static inline int grid_sgn(int v) { return (v > 0) - (v < 0); }
LSLAM_GRID_HD static inline int grid_ray_steps(int dx, int dy) {
    const int ax = grid_iabs(dx), ay = grid_iabs(dy);
    return ax > ay ? ax : ay;
}

// offset along an axis at step i (0 <= i <= n) of a ray whose end lies a cells away on it (0 <= a <= n)
LSLAM_GRID_HD static inline int grid_ray_offset(int i, int a, int n) {
    if (a == n) return i;  // the major axis (and n == 0)
    return (int)((uint32_t)(2 * i * a + n) / (uint32_t)(2 * n));
}

// the cell at step i
LSLAM_GRID_HD static inline void grid_ray_cell(int X0, int Y0, int dx, int dy, int n, int i, int &x, int &y) {
    x = X0 + grid_sgn(dx) * grid_ray_offset(i, grid_iabs(dx), n);
    y = Y0 + grid_sgn(dy) * grid_ray_offset(i, grid_iabs(dy), n);
}

// The same offsets for consecutive steps without a division per step: 2 i a + n = off 2n + rem is
// carried along; a <= n, so a step carries at most once.
struct GridAxisWalk {
    int off, rem, a2, n2;
};
LSLAM_GRID_HD static inline GridAxisWalk grid_walk_begin(int i, int a, int n) {
    GridAxisWalk w;
    w.a2 = 2 * a;
    w.n2 = n > 0 ? 2 * n : 1;
    const uint32_t num = (uint32_t)(2 * i * a + n);
    w.off = (int)(num / (uint32_t)w.n2);
    w.rem = (int)(num - (uint32_t)w.off * (uint32_t)w.n2);
    return w;
}
LSLAM_GRID_HD static inline void grid_walk_next(GridAxisWalk &w) {
    w.rem += w.a2;
    if (w.rem >= w.n2) {
        w.rem -= w.n2;
        w.off++;
    }
}

// Narrows the step interval [ilo, ihi] (inside [0, n]) to the steps whose coordinate along one axis,
// P0 + sgn(d) offset(i), lies in [t0, t1).  |P0| < 2^21, t0 and t1 in [0, 4096].
LSLAM_GRID_HD static inline void grid_clip_axis(int P0, int d, int n, int t0, int t1, int &ilo, int &ihi) {
    const int a = grid_iabs(d);
    if (a == 0) {  // the ray stays on P0
        if (P0 < t0 || P0 >= t1) ihi = ilo - 1;
        return;
    }
    // the offsets wanted: lo <= offset(i) <= hi
    const int lo = d > 0 ? t0 - P0 : P0 - (t1 - 1);
    const int hi = d > 0 ? t1 - 1 - P0 : P0 - t0;
    if (hi < 0 || lo > a) {
        ihi = ilo - 1;
        return;
    }
    if (lo > 0) {  // (2 i a + n) div 2n >= lo  <=>  2 i a + n >= 2 n lo  <=>  i >= ceil(n (2 lo - 1) / 2a)
        const int q = (n * (2 * lo - 1) + 2 * a - 1) / (2 * a);
        if (q > ilo) ilo = q;
    }
    if (hi < a) {  // (2 i a + n) div 2n <= hi  <=>  2 i a + n <= 2 n (hi + 1) - 1  <=>  i <= floor((n (2 hi + 1) - 1) / 2a)
        const int q = (n * (2 * hi + 1) - 1) / (2 * a);
        if (q < ihi) ihi = q;
    }
}

// The steps of the ray inside the tile [tx0, tx1) x [ty0, ty1): they form one interval, since each
// axis is monotone in i.  Returns false if there are none (the ray's bounding box may still meet
// the tile).
LSLAM_GRID_HD static inline bool grid_ray_clip(int X0, int Y0, int dx, int dy, int tx0, int ty0, int tx1, int ty1,
                                               int &ilo, int &ihi) {
    const int n = grid_ray_steps(dx, dy);
    ilo = 0;
    ihi = n;
    grid_clip_axis(X0, dx, n, tx0, tx1, ilo, ihi);
    if (ilo > ihi) return false;
    grid_clip_axis(Y0, dy, n, ty0, ty1, ilo, ihi);
    return ilo <= ihi;
}
