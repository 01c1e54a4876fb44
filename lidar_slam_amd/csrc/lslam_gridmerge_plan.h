// lslam_gridmerge_plan.h — the plain C++ of a map merge (lslam_grid_merge in include/lidarslam.h): the
// tiles of a destination grid and their slices, the source cell of a destination cell (step 2 of the
// definition), the clipped 3 x 3 block of N, the class of a cell and its merged value.  No HIP: the
// kernels of lslam_gridmerge.h and a CPU program (tests/test_gridmerge_plan.py) compile this same text,
// so the arithmetic that decides an index is run under the sanitizers on the CPU.
//
// A W x W destination is cut into tiles of MERGE_TW columns and MERGE_TH rows, numbered row after row;
// the tiles at the right and bottom edges are clipped to the map.  A pair's tiles are dealt to its
// workgroups in slices of `per` consecutive tiles.  A tile, not a row, is the unit because of the
// rotated gather: the source cells of a tile lie in a rotated rectangle of about the tile's area, so a
// source line that one destination row of the tile touched is touched again by the next.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSLAM_MERGE_HD __host__ __device__
#else
#define LSLAM_MERGE_HD
#endif

#define MERGE_TW 64  // columns of a tile: a wave's lanes, or its 8 groups of 8 cells
#define MERGE_TH 32  // rows of a tile: with 8 cells a lane, one pass of a 256-thread workgroup

// destination cells [x0, x1) x [y0, y1), never empty for a tile of the map
struct MergeTile {
    int x0, x1, y0, y1;
};

LSLAM_MERGE_HD static inline int merge_tiles_x(int W) { return (W + MERGE_TW - 1) / MERGE_TW; }
LSLAM_MERGE_HD static inline int merge_tiles_y(int W) { return (W + MERGE_TH - 1) / MERGE_TH; }
LSLAM_MERGE_HD static inline int merge_tiles(int W) { return merge_tiles_x(W) * merge_tiles_y(W); }  // W <= 2048: at most 2048

// tile t of a W x W map, 0 <= t < merge_tiles(W)
LSLAM_MERGE_HD static inline MergeTile merge_tile(int W, int t) {
    const int ntx = merge_tiles_x(W), ty = t / ntx, tx = t - ty * ntx;
    MergeTile q;
    q.x0 = tx * MERGE_TW;
    q.y0 = ty * MERGE_TH;
    q.x1 = q.x0 + MERGE_TW < W ? q.x0 + MERGE_TW : W;
    q.y1 = q.y0 + MERGE_TH < W ? q.y0 + MERGE_TH : W;
    return q;
}

// tiles per slice when a pair's n tiles are dealt to at most `want` workgroups, and the slices that gives
LSLAM_MERGE_HD static inline int merge_slice_tiles(int n, int want) { return (n + (want < 1 ? 1 : want) - 1) / (want < 1 ? 1 : want); }
LSLAM_MERGE_HD static inline int merge_slices(int n, int per) { return (n + per - 1) / per; }

// what step 2 reads of a pair
struct MergeXform {
    double c, s, tx, ty;  // destination world -> source world
    double oxd, oyd;      // destination origin
    double oxs, oys;      // source origin
    double cell, inv;     // inv = 1.0 / cell
    int src_w;
};

LSLAM_MERGE_HD static inline bool merge_is_finite(double v) { return fabs(v) <= DBL_MAX; }  // (a NaN fails)

// step 1
LSLAM_MERGE_HD static inline bool merge_xform_finite(const MergeXform &t) {
    return merge_is_finite(t.c) && merge_is_finite(t.s) && merge_is_finite(t.tx) && merge_is_finite(t.ty) && merge_is_finite(t.oxd) &&
           merge_is_finite(t.oyd) && merge_is_finite(t.oxs) && merge_is_finite(t.oys);
}

// the world coordinate of the centre of destination column (or row) X
LSLAM_MERGE_HD static inline double merge_world(double origin, int X, double cell) { return origin + ((double)X + 0.5) * cell; }

// The source cell of the destination cell whose centre is (wx, wy): fy * Sw + fx, or -1 off the source
// map.  The comparisons are in doubles, before any conversion: inside them fx and fy are integers below
// 2048, so the index is at most 2^22.
LSLAM_MERGE_HD static inline int merge_src_cell(const MergeXform &t, double wx, double wy) {
    const double xs = (t.c * wx - t.s * wy) + t.tx;
    const double ys = (t.s * wx + t.c * wy) + t.ty;
    const double fx = floor((xs - t.oxs) * t.inv), fy = floor((ys - t.oys) * t.inv);
    const double sw = (double)t.src_w;
    if (!(fx >= 0.0 && fx < sw && fy >= 0.0 && fy < sw)) return -1;
    return (int)fy * t.src_w + (int)fx;
}

// N(X, Y): some cell of the 3 x 3 block around (X, Y), clipped to the W x W map L, has L >= occ_min
LSLAM_MERGE_HD static inline bool merge_near_occupied(const int16_t *L, int W, int X, int Y, int occ_min) {
    const int xa = X > 0 ? X - 1 : 0, xb = X + 1 < W ? X + 1 : W - 1;
    const int ya = Y > 0 ? Y - 1 : 0, yb = Y + 1 < W ? Y + 1 : W - 1;
    bool n = false;
    for (int y = ya; y <= yb; y++)
        for (int x = xa; x <= xb; x++) n |= (int)L[(int64_t)y * W + x] >= occ_min;
    return n;
}

// the counters of stats[m], in its order
enum { MERGE_ON = 0, MERGE_NZ = 1, MERGE_SUPP = 2, MERGE_CONTRA = 3, MERGE_NEW = 4, MERGE_SAME = 5, MERGE_OPP = 6, MERGE_CHANGED = 7 };

// step 4: the gates' flags (LSLAM_MERGE_WEAK = 2, LSLAM_MERGE_CONFLICT = 4)
LSLAM_MERGE_HD static inline int merge_gates(int supported, int contradicted, int min_support, int max_permille) {
    int f = 0;
    if (supported < min_support) f |= 2;
    if (1000 * (int64_t)contradicted > (int64_t)max_permille * ((int64_t)supported + (int64_t)contradicted)) f |= 4;
    return f;
}

// step 5: the merged value of a cell that holds L under the source value v (fill: LSLAM_MERGE_FILL)
LSLAM_MERGE_HD static inline int merge_value(int L, int v, int fill, int l_min, int l_max) {
    if (v == 0 || (fill && L != 0)) return L;
    const int t = fill ? v : L + v;
    return t < l_min ? l_min : (t > l_max ? l_max : t);
}
