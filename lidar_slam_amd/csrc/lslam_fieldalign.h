// lslam_fieldalign.h — Gauss-Newton pose refinement of a revolution in the robot's distance field.
// The definition is the comment on lslam_field_align in include/lidarslam.h; tests/fieldalign_ref.py is
// its NumPy form; the per-point arithmetic and the 3 x 3 solve are lslam_fieldalign_core.h (plain C++,
// also compiled on the CPU).
//
// fieldalign_kernel: one wave per robot, four robots to a 256-thread workgroup, the whole iteration in
// one launch.  A lane takes every 64th point of its robot (12 at 720 points): steps 0 and 1 of
// lslam_grid_update, four 2-byte gathers from d2, the bilinear read and the ten fixed-point terms, added
// into ten 64-bit integers per lane.  After the robot's points the ten sums go through the wave's
// butterfly (fieldscore_wave_sum), which leaves the totals in every lane; the points used are counted by
// ballots.  Every lane then makes the same step from the same sums, so that the next evaluation's pose
// is already in every lane's registers: nothing is broadcast, nothing leaves the chip between two
// evaluations, and there is no barrier and no LDS.  Lane 0 writes trace, and at the end the outputs.
// The loops are bounded by n_iter + 1 evaluations and by the robot's point count; a robot that stops
// early leaves its loop, and its wave ends while the workgroup's other waves go on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_dist.h"
#include "lslam_fieldalign_core.h"

namespace lslam {

constexpr int FIELDALIGN_TPB = 256;
constexpr int FIELDALIGN_RPB = FIELDALIGN_TPB / 64;  // robots per workgroup: one per wave

struct FieldAlignArgs {
    lslam_fieldalign_batch b;
    lslam_fieldalign_params p;
    double inv, cell, max_r2;
    int grid_w;
};

__global__ __launch_bounds__(FIELDALIGN_TPB) void fieldalign_kernel(const FieldAlignArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * FIELDALIGN_RPB + ((int)threadIdx.x >> 6);
    if (r >= a.b.n_robots) return;  // (wave-uniform)
    // (trace, normal, n_used, iters and flags are zeroed by the launcher)

    // ---- 0. pose ----
    const long long bx = ((const long long *)a.b.pose)[3 * r], by = ((const long long *)a.b.pose)[3 * r + 1],
                    bt = ((const long long *)a.b.pose)[3 * r + 2];
    const double px0 = __longlong_as_double(bx), py0 = __longlong_as_double(by), th0 = __longlong_as_double(bt);
    FieldAlignFrame f;
    f.ox = a.b.origin[2 * r];
    f.oy = a.b.origin[2 * r + 1];
    f.inv = a.inv;
    long long *out = (long long *)a.b.pose_out + 3 * (int64_t)r;
    double X0d, Y0d;
    if (!mapmatch_robot_cell(px0, py0, th0, f.ox, f.oy, f.inv, X0d, Y0d)) {
        if (lane == 0) {
            a.b.flags[r] = LSLAM_FIELDALIGN_BAD_POSE;
            out[0] = bx;
            out[1] = by;
            out[2] = bt;
        }
        return;
    }
    // The kernel's arguments fill the scalar registers; the four doubles that only the step's end and the
    // gates read are held in vector registers, of which there are enough, so that nothing spills.
    double eps_t = a.p.eps_t, eps_r = a.p.eps_r, max_shift = a.p.max_shift, max_turn = a.p.max_turn;
    asm volatile("" : "+v"(eps_t), "+v"(eps_r), "+v"(max_shift), "+v"(max_turn));
    const int W = a.grid_w, n_iter = a.p.n_iter;
    const uint16_t *D = a.b.d2 + (int64_t)r * W * W;
    const double2 *xy = (const double2 *)a.b.xy;
    const int p0 = a.b.pt_off[r], p1 = a.b.pt_off[r + 1];
    double *trace = a.b.trace + (int64_t)r * (n_iter + 1) * 5;

    double px = px0, py = py0, th = th0;
    int flags = 0, iters = 0, n_first = 0, n_last = 0, n_valid = 0;
    unsigned long long sum[10];
    int64_t n[10];  // the last evaluation's sums, in every lane
    for (int k = 0; k <= n_iter; k++) {
        // ---- evaluation k ----
        f.px = px;
        f.py = py;
        f.c = cos(th);
        f.s = sin(th);
        if (lane == 0) {
            trace[5 * k] = px;
            trace[5 * k + 1] = py;
            trace[5 * k + 2] = th;
            trace[5 * k + 3] = f.c;
            trace[5 * k + 4] = f.s;
        }
#pragma unroll
        for (int i = 0; i < 10; i++) sum[i] = 0;
        int used = 0, valid = 0;
        for (int pb = p0; pb < p1; pb += 64) {  // (uniform: the ballots below are taken by the whole wave)
            const int p = pb + lane;
            bool ok = false, use = false;
            if (p < p1) {
                const double2 q = xy[p];
                ok = grid_valid(q) && !(q.x * q.x + q.y * q.y > a.max_r2);
                double rx, ry, fu, fv;
                int ix, iy;
                if (ok && fieldalign_locate(f, q.x, q.y, W, rx, ry, ix, iy, fu, fv)) {
                    const uint16_t *Dc = D + (int64_t)iy * W + ix;  // 0 <= ix, iy <= W - 2: all four on the map
                    const uint32_t v00 = Dc[0], v10 = Dc[1], v01 = Dc[W], v11 = Dc[W + 1];
                    double m, gx, gy;
                    fieldalign_bilinear(fieldalign_dq(v00), fieldalign_dq(v10), fieldalign_dq(v01), fieldalign_dq(v11), fu,
                                        fv, m, gx, gy);
                    if (!(m > a.p.trunc)) {
                        int64_t t[10];
                        fieldalign_terms(m, gx, gy, rx, ry, f.inv, t);
#pragma unroll
                        for (int i = 0; i < 10; i++) sum[i] += (unsigned long long)t[i];
                        use = true;
                    }
                }
            }
            valid += popc64(ballot(ok));
            used += popc64(ballot(use));
        }
#pragma unroll
        for (int i = 0; i < 10; i++) n[i] = (int64_t)fieldscore_wave_sum(sum[i]);
        if (k == 0) {
            n_first = used;
            n_valid = valid;
        }
        n_last = used;
        if (used < a.p.min_points) {
            flags |= LSLAM_FIELDALIGN_FEW;
            break;
        }
        if (k == n_iter || (flags & LSLAM_FIELDALIGN_CONVERGED)) break;  // the evaluation after the last step
        // ---- step k ----
        double d[3];
        bool ok = fieldalign_solve(n, a.p.damp_t, a.p.damp_r, d);
        const double nx = px + d[0] * a.cell, ny = py + d[1] * a.cell, nt = th + d[2];
        ok = ok && __builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nt);
        if (!ok) {
            flags |= LSLAM_FIELDALIGN_SINGULAR;
            break;
        }
        px = nx;
        py = ny;
        th = nt;
        iters = k + 1;
        if (fmax(fabs(d[0]), fabs(d[1])) < eps_t && fabs(d[2]) < eps_r) flags |= LSLAM_FIELDALIGN_CONVERGED;
    }
    // ---- gates and outputs ----
    if (fabs(px - px0) > max_shift || fabs(py - py0) > max_shift || fabs(th - th0) > max_turn)
        flags |= LSLAM_FIELDALIGN_DIVERGED;
    if ((int64_t)1000 * n_last < (int64_t)a.p.min_permille * n_valid) flags |= LSLAM_FIELDALIGN_WEAK;
    if (lane == 0) {
        const int keep = LSLAM_FIELDALIGN_SINGULAR | LSLAM_FIELDALIGN_FEW | LSLAM_FIELDALIGN_DIVERGED | LSLAM_FIELDALIGN_WEAK;
        const bool moved = !(flags & keep);
        out[0] = moved ? __double_as_longlong(px) : bx;
        out[1] = moved ? __double_as_longlong(py) : by;
        out[2] = moved ? __double_as_longlong(th) : bt;
        int64_t *nm = a.b.normal + 10 * (int64_t)r;
#pragma unroll
        for (int i = 0; i < 10; i++) nm[i] = n[i];
        a.b.n_used[3 * r] = n_first;
        a.b.n_used[3 * r + 1] = n_last;
        a.b.n_used[3 * r + 2] = n_valid;
        a.b.iters[r] = iters;
        a.b.flags[r] = flags;
    }
}

}  // namespace lslam
