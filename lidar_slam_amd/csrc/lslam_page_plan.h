// lslam_page_plan.h — the strips of a paged grid recentre (lslam_grid_recentre_paged, steps 2 and 3 of
// its definition in include/lidarslam.h): which cells of a W x W window leave it under a shift, which
// enter it, and what of either lies on the robot's canvas.  Plain C++, no HIP: the kernels of
// lslam_page.h and a CPU program (tests/test_page_plan.py) compile this same text.
//
// Under the shift (sx, sy) window cell (x, y) goes to (x - sx, y - sy).  It stays on the window for x in
// [max(0, sx), min(W, W + sx)) and y likewise; every other cell LEAVES.  The leaving set is an L: a
// horizontal strip h of |sy| full rows and a vertical strip v of |sx| columns over the remaining rows;
// with |sx| >= W or |sy| >= W it is the whole window, given as h alone.  Destination cell (x, y) ENTERS
// when its source (x + sx, y + sy) is off the window: the leaving set of the shift (-sx, -sy).
//
// A rectangle of window cells [x0, x1) x [y0, y1) is laid on the canvas with window cell (0, 0) at
// canvas cell (ox, oy), which may be negative or beyond the canvas: ox, oy are 64-bit (win is 32-bit
// and a shift is added to it).  page_clip gives the part of it whose cells are on the canvas.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSLAM_PAGE_HD __host__ __device__
#else
#define LSLAM_PAGE_HD
#endif

// window cells [x0, x1) x [y0, y1); empty when x0 >= x1 or y0 >= y1
struct PageRect {
    int x0, x1, y0, y1;
};

struct PageStrips {
    PageRect h, v;  // disjoint; either may be empty
};

LSLAM_PAGE_HD static inline int page_clampi(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

LSLAM_PAGE_HD static inline int page_area(const PageRect &q) {
    return (q.x0 < q.x1 && q.y0 < q.y1) ? (q.x1 - q.x0) * (q.y1 - q.y0) : 0;  // W <= 2048: at most 2^22
}

// the cells that leave a W x W window under the shift (sx, sy); |sx|, |sy| < 2^21
LSLAM_PAGE_HD static inline PageStrips page_leaving(int W, int sx, int sy) {
    PageStrips s;
    const int kx0 = page_clampi(sx, 0, W), kx1 = page_clampi((int64_t)W + sx, 0, W);  // the columns that stay
    const int ky0 = page_clampi(sy, 0, W), ky1 = page_clampi((int64_t)W + sy, 0, W);  // the rows that stay
    if (kx0 >= kx1 || ky0 >= ky1) {  // nothing stays
        s.h = PageRect{0, W, 0, W};
        s.v = PageRect{0, 0, 0, 0};
        return s;
    }
    // (a shift has one sign on an axis: of [0, k0) and [k1, W) at most one holds a cell)
    s.h = ky0 > 0 ? PageRect{0, W, 0, ky0} : PageRect{0, W, ky1, W};
    s.v = kx0 > 0 ? PageRect{0, kx0, ky0, ky1} : PageRect{kx1, W, ky0, ky1};
    return s;
}

// the destination cells that enter under the shift (sx, sy): their sources are off the window
LSLAM_PAGE_HD static inline PageStrips page_entering(int W, int sx, int sy) { return page_leaving(W, -sx, -sy); }

// the cells of q that are on a canvas of Cw x Cw cells whose cell (ox, oy) is window cell (0, 0)
LSLAM_PAGE_HD static inline PageRect page_clip(const PageRect &q, int64_t ox, int64_t oy, int Cw) {
    PageRect c;
    c.x0 = page_clampi(-ox, q.x0, q.x1 > q.x0 ? q.x1 : q.x0);
    c.x1 = page_clampi((int64_t)Cw - ox, c.x0, q.x1 > c.x0 ? q.x1 : c.x0);
    c.y0 = page_clampi(-oy, q.y0, q.y1 > q.y0 ? q.y1 : q.y0);
    c.y1 = page_clampi((int64_t)Cw - oy, c.y0, q.y1 > c.y0 ? q.y1 : c.y0);
    return c;
}

// window cell (x, y) is on the canvas: the definition's test, in 64 bits
LSLAM_PAGE_HD static inline bool page_on_canvas(int64_t ox, int64_t oy, int x, int y, int Cw) {
    return ox + x >= 0 && ox + x < Cw && oy + y >= 0 && oy + y < Cw;
}
