// lslam_raycast_walk.h — one beam of lslam_grid_raycast: steps 2-4 of its definition in
// include/lidarslam.h (the far cell, the walk through the map until it stops the beam, the class),
// on top of the integer ray of lslam_grid_ray.h.  Plain C++, no HIP: the kernels of lslam_raycast.h
// and a CPU program (tests/test_raycast_walk.py) compile this same text.  The map is a template
// argument: a callable code(ox, oy) that gives the 2-bit code of the cell at an offset from the
// robot cell, RAYCAST_UNKNOWN for a cell off the map.
#pragma once
#include <stdint.h>

#include "lslam_grid_ray.h"

enum { RAYCAST_UNKNOWN = 0, RAYCAST_FREE = 1, RAYCAST_OCC = 2 };                  // cell codes
enum { RAYCAST_K_NONE = 0, RAYCAST_K_UNKNOWN = 1, RAYCAST_K_OCC = 2 };            // stop kinds
enum { RAYCAST_C_INVALID = 0, RAYCAST_C_MATCH = 1, RAYCAST_C_NOVEL = 2, RAYCAST_C_THROUGH = 3, RAYCAST_C_UNMAPPED = 4 };
enum { RAYCAST_D_MAX = 8192 };      // |Dx|, |Dy| of a far cell: 2 i |D| + n and ox ox + oy oy stay inside int32
enum { RAYCAST_I_BEYOND = 1 << 30 };  // the measured step of a beyond point: larger than any i_h + tol

// the code of a log-odds value
LSLAM_GRID_HD static inline int raycast_code(int l, int occ_min, int free_max) {
    return l >= occ_min ? RAYCAST_OCC : (l <= free_max ? RAYCAST_FREE : RAYCAST_UNKNOWN);
}

struct RaycastPose {  // step 0's values of one robot
    double px, py, c, s, ox, oy, inv, X0d, Y0d;
};

// the cell of a robot-frame point (lslam_grid_update step 1) as its offset from the robot cell, in doubles
LSLAM_GRID_HD static inline void raycast_cell_offset(const RaycastPose &r, double x, double y, double &dxd, double &dyd) {
    const double wx = r.px + (r.c * x - r.s * y);
    const double wy = r.py + (r.s * x + r.c * y);
    dxd = __builtin_floor((wx - r.ox) * r.inv) - r.X0d;
    dyd = __builtin_floor((wy - r.oy) * r.inv) - r.Y0d;
}

// step 2: the far cell's offset (Dx, Dy); false for a point that turns INVALID
LSLAM_GRID_HD static inline bool raycast_far_cell(const RaycastPose &r, double x, double y, double far, int &Dx, int &Dy) {
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const double m = ax > ay ? ax : ay;
    const double q = far / m;
    double dxd, dyd;
    raycast_cell_offset(r, x * q, y * q, dxd, dyd);
    // (a NaN fails the comparison)
    if (!(__builtin_fabs(dxd) <= (double)RAYCAST_D_MAX && __builtin_fabs(dyd) <= (double)RAYCAST_D_MAX)) return false;
    Dx = (int)dxd;
    Dy = (int)dyd;
    return true;
}

// step 3: walks the ray to (Dx, Dy) until the map stops it; returns the kind, (ox, oy, ih) as stop
template <class Code>
LSLAM_GRID_HD static inline int raycast_walk(int Dx, int Dy, int Rc, const Code &code, int &ox, int &oy, int &ih) {
    const int ax = grid_iabs(Dx), ay = grid_iabs(Dy), sx = grid_sgn(Dx), sy = grid_sgn(Dy);
    const int n = ax > ay ? ax : ay, rc2 = Rc * Rc;  // Rc <= 4096
    GridAxisWalk wx = grid_walk_begin(0, ax, n), wy = grid_walk_begin(0, ay, n);
    int r2 = 0;  // ox ox + oy oy, carried along: (u + 1)^2 = u^2 + 2 u + 1
    ox = 0;
    oy = 0;
    for (ih = 0; ih <= n; ih++) {
        if (r2 > rc2) return RAYCAST_K_NONE;
        const int v = code(ox, oy);
        if (v == RAYCAST_OCC) return RAYCAST_K_OCC;
        if (v != RAYCAST_FREE) return RAYCAST_K_UNKNOWN;
        if (ih == n) break;  // (ox, oy) stays the offset of step n
        const int ux = wx.off, uy = wy.off;
        grid_walk_next(wx);
        grid_walk_next(wy);
        if (wx.off != ux) {
            r2 += 2 * ux + 1;
            ox += sx;
        }
        if (wy.off != uy) {
            r2 += 2 * uy + 1;
            oy += sy;
        }
    }
    ih = n + 1;
    return RAYCAST_K_NONE;
}

// step 4: the class of a beam of this kind that the map stops at step ih and that returned at step im
// (RAYCAST_I_BEYOND for a beyond point)
LSLAM_GRID_HD static inline int raycast_class(int kind, int ih, int im, int tol) {
    if (kind == RAYCAST_K_OCC) return im < ih - tol ? RAYCAST_C_NOVEL : (im > ih + tol ? RAYCAST_C_THROUGH : RAYCAST_C_MATCH);
    if (kind == RAYCAST_K_UNKNOWN) return im < ih - tol ? RAYCAST_C_NOVEL : RAYCAST_C_UNMAPPED;
    return im >= ih - tol ? RAYCAST_C_MATCH : RAYCAST_C_NOVEL;  // (a beyond point's im exceeds every ih)
}

// steps 1 (the measured step) to 4 of one valid point: the byte of cls, and stop; 0 and (0, 0, 0) for
// a point that step 2 turns INVALID
template <class Code>
LSLAM_GRID_HD static inline int raycast_point(const RaycastPose &r, double x, double y, double max_r2, double far, int Rc,
                                              int tol, const Code &code, int &ox, int &oy, int &ih, bool &beyond) {
    ox = oy = ih = 0;
    beyond = x * x + y * y > max_r2;
    int Dx, Dy;
    if (!raycast_far_cell(r, x, y, far, Dx, Dy)) {
        beyond = false;
        return 0;
    }
    int im = RAYCAST_I_BEYOND;
    if (!beyond) {  // within max_range / cell + 1 cells of the robot cell: the conversions cannot overflow
        double dxd, dyd;
        raycast_cell_offset(r, x, y, dxd, dyd);
        im = grid_ray_steps((int)dxd, (int)dyd);
    }
    const int kind = raycast_walk(Dx, Dy, Rc, code, ox, oy, ih);
    return raycast_class(kind, ih, im, tol) | (kind << 4);
}
