// lslam_fieldalign_core.h — the per-point arithmetic and the 3 x 3 solve of lslam_field_align (its
// definition is the comment in include/lidarslam.h): a point in the robot's frame and a pose -> the
// bilinear read of the distance field, its gradient and the point's ten fixed-point terms; ten integer
// sums -> one damped Gauss-Newton step by LDL^T.  Plain C++, no HIP: the kernel of lslam_fieldalign.h
// and a CPU program (tests/test_fieldalign_core.py) compile this same text.
//
// Every double operation is written as one statement's worth of one rounding: the library is built
// with -ffp-contract=off, so that nothing is fused, and the order below is the definition's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lslam_grid_ray.h"

enum { FIELDALIGN_S = 20 };          // a term t is summed as rint(t 2^S)
enum { FIELDALIGN_MAX_ITER = 32 };   // n_iter's upper end

// The overflow bound of the sums.  The field min(d, d_max) is 1-Lipschitz between neighbouring cells
// and dq floors it to a multiple of 1/256: a corner difference, and so |gx| and |gy|, which lie between
// two of them, is at most 1 + 1/256.  |rx| + |ry| <= sqrt(2) max_range, max_range / cell <= 4096:
// |jt| <= (1 + 1/256) sqrt(2) 4096 < 5817, jt^2 < 2^25.02; m <= trunc <= 255.  The largest term is jt^2:
// 2^25.02 2^20 = 2^45.02 per point, so 2^16 = 65536 points per robot stay below 2^61.1 < 2^63.  (The
// kernel adds as unsigned 64-bit integers: beyond that the sums wrap, they do not trap.)

// floor(256 sqrt(v)) for v < 2^16, as an integer: isqrt(65536 v).  The double square root of n < 2^32
// is within one of the integer root whatever the hardware rounds to; the two corrections make it exact.
LSLAM_GRID_HD static inline uint32_t fieldalign_isqrt16(uint32_t v) {
    const uint64_t n = (uint64_t)v << 16;
    uint64_t r = (uint64_t)sqrt((double)n);
    if (r * r > n) r--;
    if ((r + 1) * (r + 1) <= n) r++;
    return (uint32_t)r;
}
// a corner's distance in cells
LSLAM_GRID_HD static inline double fieldalign_dq(uint32_t v) { return (double)fieldalign_isqrt16(v) / 256.0; }

struct FieldAlignFrame {  // one evaluation's pose, the robot's origin and 1 / cell
    double px, py, c, s, ox, oy, inv;
};

// The field's cell corner below the point and the fractions in it: false if one of the four corners
// (ix .. ix + 1, iy .. iy + 1) lies off the map.  (rx, ry) is the rotated point, kept for jt.
LSLAM_GRID_HD static inline bool fieldalign_locate(const FieldAlignFrame &f, double x, double y, int W, double &rx,
                                                   double &ry, int &ix, int &iy, double &fu, double &fv) {
    rx = f.c * x - f.s * y;
    ry = f.s * x + f.c * y;
    const double wx = f.px + rx, wy = f.py + ry;
    const double u = (wx - f.ox) * f.inv - 0.5, v = (wy - f.oy) * f.inv - 0.5;
    const double iu = floor(u), iv = floor(v);
    const double top = (double)(W - 2);
    if (!(iu >= 0.0 && iu <= top && iv >= 0.0 && iv <= top)) return false;  // (a NaN is off the map)
    ix = (int)iu;
    iy = (int)iv;
    fu = u - iu;
    fv = v - iv;
    return true;
}

// Bilinear interpolation of the corner distances d00 = D[iy][ix], d10 = D[iy][ix + 1], d01 = D[iy + 1][ix],
// d11 = D[iy + 1][ix + 1]: the distance m and its partial derivatives along x and y, per cell.
LSLAM_GRID_HD static inline void fieldalign_bilinear(double d00, double d10, double d01, double d11, double fu, double fv,
                                                     double &m, double &gx, double &gy) {
    const double e0 = d10 - d00, e1 = d11 - d01;
    const double a0 = d00 + fu * e0, a1 = d01 + fu * e1;
    gy = a1 - a0;
    m = a0 + fv * gy;
    gx = e0 + fv * (e1 - e0);
}

LSLAM_GRID_HD static inline int64_t fieldalign_q(double t) { return (int64_t)rint(t * 1048576.0); }

// The point's ten terms: the six of J^T J (xx, xy, xt, yy, yt, tt), the three of J^T r and r^2
LSLAM_GRID_HD static inline void fieldalign_terms(double m, double gx, double gy, double rx, double ry, double inv,
                                                  int64_t t[10]) {
    const double jt = (gy * rx - gx * ry) * inv;
    t[0] = fieldalign_q(gx * gx);
    t[1] = fieldalign_q(gx * gy);
    t[2] = fieldalign_q(gx * jt);
    t[3] = fieldalign_q(gy * gy);
    t[4] = fieldalign_q(gy * jt);
    t[5] = fieldalign_q(jt * jt);
    t[6] = fieldalign_q(gx * m);
    t[7] = fieldalign_q(gy * m);
    t[8] = fieldalign_q(jt * m);
    t[9] = fieldalign_q(m * m);
}

LSLAM_GRID_HD static inline bool fieldalign_pivot_ok(double d) { return d > 0.0 && d < (double)INFINITY; }

// One damped Gauss-Newton step from the ten sums: (J^T J + diag(damp_t, damp_t, damp_r)) delta = -J^T r
// by LDL^T; delta = (dx, dy in cells, dtheta in rad).  false: a pivot is not finite and > 0.
LSLAM_GRID_HD static inline bool fieldalign_solve(const int64_t n[10], double damp_t, double damp_r, double delta[3]) {
    const double sc = 1.0 / 1048576.0;
    const double h00 = (double)n[0] * sc + damp_t, h01 = (double)n[1] * sc, h02 = (double)n[2] * sc;
    const double h11 = (double)n[3] * sc + damp_t, h12 = (double)n[4] * sc, h22 = (double)n[5] * sc + damp_r;
    const double g0 = (double)n[6] * sc, g1 = (double)n[7] * sc, g2 = (double)n[8] * sc;
    delta[0] = delta[1] = delta[2] = 0.0;
    const double d0 = h00;
    if (!fieldalign_pivot_ok(d0)) return false;
    const double l10 = h01 / d0, l20 = h02 / d0;
    const double d1 = h11 - l10 * h01;
    if (!fieldalign_pivot_ok(d1)) return false;
    const double t21 = h12 - l20 * h01;
    const double l21 = t21 / d1;
    const double d2 = (h22 - l20 * h02) - l21 * t21;
    if (!fieldalign_pivot_ok(d2)) return false;
    const double y0 = g0, y1 = g1 - l10 * y0, y2 = (g2 - l20 * y0) - l21 * y1;
    const double z0 = y0 / d0, z1 = y1 / d1, z2 = y2 / d2;
    const double x2 = z2, x1 = z1 - l21 * x2, x0 = (z0 - l10 * x1) - l20 * x2;
    delta[0] = -x0;
    delta[1] = -x1;
    delta[2] = -x2;
    return true;
}
