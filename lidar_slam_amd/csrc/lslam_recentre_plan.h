// lslam_recentre_plan.h — the plan of a grid recentre (lslam_grid_recentre, steps 1 and 4 of its
// definition in include/lidarslam.h): the shift rule, and how a W x W grid is shifted IN PLACE by
// whole cells, band of rows after band of rows.  Plain C++, no HIP: the kernel of lslam_recentre.h
// and a CPU program (tests/test_recentre_plan.py) compile this same text.
//
// The shift (sx, sy) gives L'[y][x] = L[y + sy][x + sx] where that source cell is on the map and 0
// elsewhere.  Destination row y is copied for y in [dy0, dy1) = [max(0, -sy), min(W, W - sy)) and
// destination column x for x in [dx0, dx1), likewise from sx; every other destination cell is zero.
//
// In place a destination row may be a source row that has not been read yet.  The rule:
//   - the destination rows are cut into bands of B rows, [jB, min(W, (j+1)B));
//   - a band is read completely (its source cells, into a buffer as large as the band) before any
//     of it is stored;
//   - bands go in ascending j for sy >= 0 and in descending j for sy < 0.
// For sy >= 0 band j reads rows [jB + sy, (j+1)B + sy), none below jB, and bands 0 .. j-1 stored
// rows below jB only: nothing a later band reads has been stored.  Rows a band both reads and
// stores (sy < B, and sy = 0 with sx != 0, where a row moves along itself) are safe because the
// band's reads end before its stores begin.  sy < 0 is the mirror image.  The zero-fill rows and
// columns are part of the bands, stored with them: for sy > 0 the rows [W - sy, W) are sources of
// the rows sy below them, and they come last.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSLAM_RECENTRE_HD __host__ __device__
#else
#define LSLAM_RECENTRE_HD
#endif

// cells of one band: 32 KiB of int16, what one workgroup keeps in flight
enum { RECENTRE_BAND_CELLS = 16384 };

// floor(a / b) for b > 0
LSLAM_RECENTRE_HD static inline int recentre_floordiv(int a, int b) {
    const int q = a / b;
    return (a - q * b < 0) ? q - 1 : q;
}

// step 1 for one axis once the margin has triggered: the robot cell c goes to within quantum / 2 of W / 2.
// |c| < 2^20, W <= 2048, quantum <= 64: nothing leaves int32
LSLAM_RECENTRE_HD static inline int recentre_axis_shift(int c, int W, int quantum) {
    return quantum * recentre_floordiv(c - W / 2 + quantum / 2, quantum);
}

// step 1: the shift of a robot whose cell is (X0, Y0)
LSLAM_RECENTRE_HD static inline void recentre_shift(int X0, int Y0, int W, int margin, int quantum, int &sx, int &sy) {
    const bool inside = margin <= X0 && X0 < W - margin && margin <= Y0 && Y0 < W - margin;
    sx = inside ? 0 : recentre_axis_shift(X0, W, quantum);
    sy = inside ? 0 : recentre_axis_shift(Y0, W, quantum);
}

// rows of a band: as many whole rows as RECENTRE_BAND_CELLS hold (grid_w <= 2048: at least 8)
LSLAM_RECENTRE_HD static inline int recentre_band_rows(int W) {
    const int b = RECENTRE_BAND_CELLS / W;
    return b < 1 ? 1 : (b > W ? W : b);
}

struct RecentrePlan {
    int W, sx, sy, B, nbands;
    int dx0, dx1;  // destination columns that are copied, from columns [dx0 + sx, dx1 + sx)
    int dy0, dy1;  // destination rows that are copied, from rows [dy0 + sy, dy1 + sy)
};

// a band in the order of execution
struct RecentreBand {
    int y0, y1;    // its destination rows: all of them are stored
    int cy0, cy1;  // those of them that are copied (cy0 == cy1: none); [y0, cy0) and [cy1, y1) are zero rows;
                   // in a copied row the columns [0, dx0) and [dx1, W) are zero
};

LSLAM_RECENTRE_HD static inline int recentre_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// |sx|, |sy| < 2^21.  A shift of W or more on either axis copies nothing
LSLAM_RECENTRE_HD static inline RecentrePlan recentre_plan(int W, int sx, int sy, int B) {
    RecentrePlan p;
    p.W = W;
    p.sx = sx;
    p.sy = sy;
    p.B = B;
    p.nbands = (W + B - 1) / B;
    p.dx0 = recentre_clampi(-sx, 0, W);
    p.dx1 = recentre_clampi(W - sx, 0, W);
    p.dy0 = recentre_clampi(-sy, 0, W);
    p.dy1 = recentre_clampi(W - sy, 0, W);
    if (p.dx0 >= p.dx1 || p.dy0 >= p.dy1) p.dx0 = p.dx1 = p.dy0 = p.dy1 = 0;
    return p;
}

// the k-th band to execute, k = 0 .. nbands - 1
LSLAM_RECENTRE_HD static inline RecentreBand recentre_band(const RecentrePlan &p, int k) {
    const int j = p.sy >= 0 ? k : p.nbands - 1 - k;
    RecentreBand b;
    b.y0 = j * p.B;
    b.y1 = b.y0 + p.B < p.W ? b.y0 + p.B : p.W;
    b.cy0 = recentre_clampi(p.dy0, b.y0, b.y1);
    b.cy1 = recentre_clampi(p.dy1, b.cy0, b.y1);
    return b;
}

// destination cell (y, x) of band b: true and its source cell's flat index when it is copied, false when it is zero
LSLAM_RECENTRE_HD static inline bool recentre_source(const RecentrePlan &p, const RecentreBand &b, int y, int x, int &src) {
    if (y < b.cy0 || y >= b.cy1 || x < p.dx0 || x >= p.dx1) return false;
    src = (y + p.sy) * p.W + x + p.sx;
    return true;
}
