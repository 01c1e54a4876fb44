// lslam_dist_core.h — the two 1-D passes of lslam_grid_distance (its definition is the comment in
// include/lidarslam.h): a column of source bits -> g, the distance to the column's nearest source
// saturated at d_max, and a row of g -> d2, the squared Euclidean distance saturated at d_max^2.
// Plain C++, no HIP: the kernel of lslam_dist.h and a CPU program (tests/test_dist_core.py) compile
// this same text.
//
// The transform is separable:
//   g[y][x]  = min(d_max, min over sources (x, y') of |y - y'|)
//   d2[y][x] = min(d_max^2, min over x' of (x - x')^2 + g[y][x']^2)
// A saturated g stands for a column distance >= d_max, whose square is >= the cap whatever x' is, and
// |x - x'| >= d_max gives a square >= the cap whatever g is: only |x - x'| < d_max and g < d_max can
// matter.  Every loop below is bounded by d_max or by the length of what it reads, not by the data.
#pragma once
#include <stdint.h>

#include "lslam_grid_ray.h"

enum { DIST_D_MAX = 255 };  // the largest d_max: g fits a byte and d_max^2 = 65025 a uint16

// A column of source bits, 32 rows to a word: bit j of col[k * stride] is row 32 k + j of the column,
// k = 0 .. nblk-1; rows outside those words hold no source.  Returns g of row ry
// (0 <= ry < 32 nblk): the distance to the nearest set bit, ry itself included, saturated at d_max.
// At most 2 (d_max / 32 + 2) words are read: a direction ends at a set bit or when the rows it has
// passed reach d_max.
LSLAM_GRID_HD static inline int dist_column_g(const uint32_t *col, int stride, int nblk, int ry, int d_max) {
    const int wi = ry >> 5, bi = ry & 31;
    const uint32_t w0 = col[wi * stride];
    int best = d_max;
    // towards larger rows, from ry itself
    uint32_t w = w0 >> bi;
    if (w) {
        best = __builtin_ctz(w);
    } else {
        int d = 32 - bi;  // rows passed without a source
        for (int k = wi + 1; k < nblk && d < d_max; k++, d += 32) {
            w = col[k * stride];
            if (w) {
                d += __builtin_ctz(w);
                if (d < best) best = d;
                break;
            }
        }
    }
    // towards smaller rows, from ry itself
    w = w0 << (31 - bi);
    if (w) {
        const int d = __builtin_clz(w);
        if (d < best) best = d;
    } else {
        int d = bi + 1;
        for (int k = wi - 1; k >= 0 && d < best; k--, d += 32) {
            w = col[k * stride];
            if (w) {
                d += __builtin_clz(w);
                if (d < best) best = d;
                break;
            }
        }
    }
    return best < d_max ? best : d_max;
}

// The columns of a row that can matter (g < d_max) as bits, 64 columns to a word, nwords words; columns
// outside them cannot.  Returns the distance from column x to the nearest set bit, x itself included,
// saturated at limit: at most 2 (limit / 64 + 2) words are read.
LSLAM_GRID_HD static inline int dist_nearest_col(const uint64_t *m, int nwords, int x, int limit) {
    const int wi = x >> 6, bi = x & 63;
    const uint64_t w0 = m[wi];
    int best = limit;
    uint64_t w = w0 >> bi;
    if (w) {
        best = __builtin_ctzll(w);
    } else {
        int d = 64 - bi;
        for (int k = wi + 1; k < nwords && d < limit; k++, d += 64) {
            w = m[k];
            if (w) {
                d += __builtin_ctzll(w);
                if (d < best) best = d;
                break;
            }
        }
    }
    w = w0 << (63 - bi);
    if (w) {
        const int d = __builtin_clzll(w);
        if (d < best) best = d;
    } else {
        int d = bi + 1;
        for (int k = wi - 1; k >= 0 && d < best; k--, d += 64) {
            w = m[k];
            if (w) {
                d += __builtin_clzll(w);
                if (d < best) best = d;
                break;
            }
        }
    }
    return best < limit ? best : limit;
}

// A row of g (W entries, each 0 .. d_max) -> d2 of cell x: the search runs outwards from x, r = r_first,
// r_first + 1, .. and ends when r^2 alone reaches the best sum so far, at r = d_max or at r = W,
// whichever is first.  r_first: every column nearer to x than that, x aside, is saturated (1 if nothing
// is known; dist_nearest_col of the row's unsaturated columns skips the saturated stretch around x).
template <class G>
LSLAM_GRID_HD static inline int dist_row_d2(const G *g, int W, int x, int d_max, int r_first = 1) {
    const int g0 = (int)g[x];
    int best = g0 < d_max ? g0 * g0 : d_max * d_max;
    const int rmax = d_max < W ? d_max : W;
    for (int r = r_first < 1 ? 1 : r_first; r < rmax; r++) {
        const int r2 = r * r;
        if (r2 >= best) break;
        int m = d_max;
        if (x - r >= 0) m = (int)g[x - r];
        if (x + r < W) {
            const int t = (int)g[x + r];
            if (t < m) m = t;
        }
        if (m < d_max) {
            const int c = r2 + m * m;
            if (c < best) best = c;
        }
    }
    return best;
}

// NOT_FREE mode: every cell off the map is a source, so cell (x, y) is b = min(x + 1, W - x, y + 1, W - y)
// cells from the nearest of them
LSLAM_GRID_HD static inline int dist_border2(int x, int y, int W) {
    int b = x + 1;
    if (W - x < b) b = W - x;
    if (y + 1 < b) b = y + 1;
    if (W - y < b) b = W - y;
    return b * b;
}
