// lslam_gridpoints_plan.h — the plain C++ of a map read as a revolution (lslam_grid_points in
// include/lidarslam.h): the bands of rows a grid is cut into, the units a wave walks in a band, the range
// test and the point of a cell (steps 2 and 4 of the definition), the stride and the slot of an ordinal
// (step 3).  No HIP: the kernels of lslam_gridpoints.h and a CPU program (tests/test_gridpoints_plan.py)
// compile this same text, so the arithmetic that decides an index is run under the sanitizers on the CPU.
//
// A W x W grid is cut into bands of `rows` whole rows, at most GP_BANDS of them; one wave owns a band.
// It walks the band's units in row-major order, GP_WAVE units an iteration, a lane a unit; a unit is
// CELLS consecutive cells of one row (8: one 16-byte load, W a multiple of 8; or 1).  Row-major order
// of the cells is therefore: iteration, then lane, then cell of the unit.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSLAM_GP_HD __host__ __device__
#else
#define LSLAM_GP_HD
#endif

#define GP_BANDS 256  // most bands of a grid (LSLAM_GRIDPOINTS_BANDS): a row of band_counts
#define GP_WAVE 64    // lanes of a wave: units of an iteration

// rows of a band when a grid of W rows is dealt to at most `want` waves, and the bands that gives
LSLAM_GP_HD static inline int gp_band_rows(int W, int want) {
    const int n = want < 1 ? 1 : (want > GP_BANDS ? GP_BANDS : want);
    return (W + n - 1) / n;
}
LSLAM_GP_HD static inline int gp_bands(int W, int rows) { return (W + rows - 1) / rows; }  // <= GP_BANDS for rows of gp_band_rows

// units of band b of a W x W grid in units of `cells` cells: (first row, units in the band)
struct GpBand {
    int y0, n;
};
LSLAM_GP_HD static inline GpBand gp_band(int W, int rows, int b, int cells) {
    GpBand q;
    q.y0 = b * rows;
    const int y1 = q.y0 + rows < W ? q.y0 + rows : W;
    q.n = (y1 - q.y0) * (W / cells);  // W <= 2048: at most 2^22
    return q;
}

// unit u of a band that starts at row y0: its row and its first column
LSLAM_GP_HD static inline void gp_unit(int W, int y0, int u, int cells, int &X0, int &Y) {
    const int upr = W / cells, row = u / upr;
    Y = y0 + row;
    X0 = (u - row * upr) * cells;
}

// what steps 1, 2 and 4 read of a robot
struct GpAnchor {
    double ox, oy;  // origin
    double ax, ay;  // the anchor's position
    double c, s;    // cos and sin of its heading
    double cell, r2;
};

LSLAM_GP_HD static inline bool gp_is_finite(double v) { return fabs(v) <= DBL_MAX; }  // (a NaN fails)

// step 1
LSLAM_GP_HD static inline bool gp_anchor_finite(const GpAnchor &a) {
    return gp_is_finite(a.ox) && gp_is_finite(a.oy) && gp_is_finite(a.ax) && gp_is_finite(a.ay) && gp_is_finite(a.c) && gp_is_finite(a.s);
}

// step 2: the offset from the anchor of the centre of column (or row) X, and the range test
LSLAM_GP_HD static inline double gp_offset(double origin, int X, double cell, double anchor) {
    const double w = origin + ((double)X + 0.5) * cell;
    return w - anchor;
}
LSLAM_GP_HD static inline bool gp_in_range(double dx, double dy, double r2) {
    const double d2 = dx * dx + dy * dy;
    return d2 > 0.0 && d2 <= r2;
}

// step 4: the point in the anchor's frame
LSLAM_GP_HD static inline void gp_point(const GpAnchor &a, double dx, double dy, double &px, double &py) {
    px = (a.c * dx) + (a.s * dy);
    py = (a.c * dy) - (a.s * dx);
}

// step 3 (n_in <= 2^22, 1 <= cap <= 65536: the sums fit 32 bits)
LSLAM_GP_HD static inline int gp_stride(int n_in, int cap) {
    const int s = (n_in + cap - 1) / cap;
    return s < 1 ? 1 : s;
}
LSLAM_GP_HD static inline int gp_n_out(int n_in, int stride) { return (n_in + stride - 1) / stride; }
// the slot of ordinal i, or -1 if it is not taken
LSLAM_GP_HD static inline int gp_slot(int i, int stride) {
    if (stride == 1) return i;
    const int j = i / stride;
    return i - j * stride == 0 ? j : -1;
}

// step 5
LSLAM_GP_HD static inline int gp_flags(int n_out, int stride) { return (n_out == 0 ? 2 : 0) | (stride > 1 ? 4 : 0); }

// set bits of a 64-lane ballot strictly below `lane`: what mbcnt gives a lane on the device
static inline int gp_below(uint64_t m, int lane) { return __builtin_popcountll(m & (((uint64_t)1 << lane) - 1)); }
