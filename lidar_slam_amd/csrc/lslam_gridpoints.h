// lslam_gridpoints.h — a map read as a revolution: the occupied cells of a grid within a radius of an
// anchor pose, compacted in row-major order into a fixed slice of points in the anchor's frame.  The
// definition is the comment on lslam_grid_points in include/lidarslam.h; tests/gridpoints_ref.py is its
// NumPy form; the bands, the units, the range test, the point and the stride are
// lslam_gridpoints_plan.h, plain C++ that a CPU program runs under the sanitizers.
//
// gridpoints_kernel<CELLS, WRITE>: ONE wave a workgroup, a workgroup is (robot, band of whole rows), by
// gp_band_rows, so a large fleet is a few waves a robot and a robot alone still fills the chip.  The
// wave walks its band's units in order, 64 an iteration.  CELLS = 8: a lane takes 8 consecutive cells
// of a row in one 16-byte load (grid_w a multiple of 8, logodds 16-byte aligned); CELLS = 1: a lane a
// cell.  The occupancy test is on integers; most 16-byte groups of a map hold no occupied cell, and an
// iteration whose ballot of them is empty ends there.  The FP64 range test runs only in a lane that
// holds an occupied cell, once per such cell.
//   WRITE = false, the count pass: (occupied, occupied in range) stay in two registers over the band,
//     are summed over the wave, and lane 0 stores them to band_counts[r][band].  No atomics, nothing to
//     clear: every band of every robot stores its pair (zeros for a BAD_ANCHOR robot).
//   WRITE = true, the write pass, behind it on the stream: every wave sums the finished pairs of its
//     robot (at most 256, four a lane): n_occ, n_in, and the n_in of the bands before its own, which is
//     its first ordinal.  Band 0 stores counts, flags and pt_off.  A band without a cell in range ends
//     there: of an empty map the write pass reads the counts only.  Otherwise the wave walks as the count
//     pass did; the ordinal of a cell is the running ordinal, plus the in-range cells of the lanes below
//     (one ballot and mbcnt per cell of the unit), plus those below it in its own unit; the running
//     ordinal then grows by the iteration's total (the ballots' population).  A taken cell stores its
//     point, 16 bytes, to its slot.  Order decides the slot, so no atomic does.
// The slots behind the last point are zeroed by the launcher's memset of xy, ahead of both passes.
// No LDS (a wave is a workgroup: there is no cross-wave prefix), no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_gridpoints_plan.h"
#include "lslam_wave.h"

namespace lslam {

static_assert(GP_BANDS == LSLAM_GRIDPOINTS_BANDS && GP_WAVE == LSLAM_WAVE, "the plan's constants are the ABI's and the wave's");

// 112 bytes
struct GridPointsArgs {
    lslam_gridpoints_batch b;
    double cell, r2;
    int grid_w, occ_min, cap;
    int n_robots;
    int rows;     // rows of a band
    int n_bands;  // workgroups per robot
};

__device__ __forceinline__ int gp_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int CELLS, bool WRITE>
__global__ __launch_bounds__(GP_WAVE) void gridpoints_kernel(const GridPointsArgs a) {
    const int lane = lane_id();
    const int r = (int)(blockIdx.x / (unsigned)a.n_bands), band = (int)(blockIdx.x % (unsigned)a.n_bands);
    int32_t *bc = a.b.band_counts + 2 * GP_BANDS * (int64_t)r;

    GpAnchor A;
    {
        const double *o = a.b.origin + 2 * (int64_t)r, *p = a.b.anchor + 4 * (int64_t)r;
        A.ox = o[0], A.oy = o[1];
        A.ax = p[0], A.ay = p[1], A.c = p[2], A.s = p[3];
        A.cell = a.cell, A.r2 = a.r2;
    }
    const bool ok = gp_anchor_finite(A);  // (uniform)

    int ord = 0, stride = 1;
    if constexpr (WRITE) {
        int n_occ = 0, n_in = 0;
        for (int k = lane; k < a.n_bands; k += GP_WAVE) {
            const int v_occ = bc[2 * k], v_in = bc[2 * k + 1];
            n_occ += v_occ;
            n_in += v_in;
            ord += k < band ? v_in : 0;
        }
        n_occ = gp_wave_sum(n_occ), n_in = gp_wave_sum(n_in), ord = gp_wave_sum(ord);
        stride = gp_stride(n_in, a.cap);
        if (band == 0 && lane == 0) {
            const int n_out = gp_n_out(n_in, stride);
            int32_t *cn = a.b.counts + 4 * (int64_t)r;
            cn[0] = n_occ, cn[1] = n_in, cn[2] = ok ? stride : 0, cn[3] = n_out;  // (a BAD_ANCHOR robot's pairs are zeros)
            a.b.flags[r] = ok ? gp_flags(n_out, stride) : LSLAM_GRIDPOINTS_BAD_ANCHOR;
            a.b.pt_off[r] = r * a.cap;
            if (r == a.n_robots - 1) a.b.pt_off[a.n_robots] = a.n_robots * a.cap;
        }
        if (!ok || bc[2 * band + 1] == 0) return;  // (uniform)
    } else {
        if (!ok) {
            if (lane == 0) bc[2 * band] = 0, bc[2 * band + 1] = 0;
            return;  // (uniform)
        }
    }

    const int W = a.grid_w;
    const int16_t *L = a.b.logodds + (int64_t)r * W * W;
    double *out = a.b.xy + 2 * (int64_t)r * a.cap;
    const GpBand q = gp_band(W, a.rows, band, CELLS);
    int c_occ = 0, c_in = 0;

    for (int u0 = 0; u0 < q.n; u0 += GP_WAVE) {
        const int u = u0 + lane;
        int X0 = 0, Y = 0;
        uint32_t occ = 0;  // bit j: cell j of the unit is occupied
        if (u < q.n) {
            gp_unit(W, q.y0, u, CELLS, X0, Y);
            const int16_t *Lp = L + (int64_t)Y * W + X0;
            if constexpr (CELLS == 8) {
                const uint4 g = *(const uint4 *)Lp;
                const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int j = 0; j < 8; j++) occ |= ((int)(int16_t)(w[j >> 1] >> ((j & 1) * 16)) >= a.occ_min ? 1u : 0u) << j;
            } else {
                occ = (int)Lp[0] >= a.occ_min ? 1u : 0u;
            }
        }
        if (!ballot(occ != 0)) continue;  // (uniform) no occupied cell in these 64 units
        // the occupied ones, a cell in a hundred of a map: one loop, not 8 branches
        uint32_t in = 0;  // bit j: cell j is occupied and in range
        const double dy = gp_offset(A.oy, Y, A.cell, A.ay);
        for (uint32_t m = occ; m;) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            in |= (gp_in_range(gp_offset(A.ox, X0 + j, A.cell, A.ax), dy, A.r2) ? 1u : 0u) << j;
        }
        if constexpr (!WRITE) {
            c_occ += __popc(occ);
            c_in += __popc(in);
        } else {
            int below = 0, total = 0;  // in-range cells of the lanes below, of the iteration
#pragma unroll
            for (int j = 0; j < CELLS; j++) {
                const uint64_t bj = ballot((in >> j) & 1u);
                below += (int)mbcnt(bj);
                total += popc64(bj);
            }
            int i = ord + below;
            for (uint32_t m = in; m; i++) {
                const int j = __ffs(m) - 1;
                m &= m - 1;
                const int slot = gp_slot(i, stride);
                if (slot >= 0 && slot < a.cap) {  // (slot < n_out <= cap by the counts; the bound is kept in sight)
                    double px, py;
                    gp_point(A, gp_offset(A.ox, X0 + j, A.cell, A.ax), dy, px, py);
                    out[2 * (int64_t)slot] = px, out[2 * (int64_t)slot + 1] = py;  // (xy is held to 8-byte alignment only)
                }
            }
            ord += total;
        }
    }

    if constexpr (!WRITE) {
        c_occ = gp_wave_sum(c_occ), c_in = gp_wave_sum(c_in);
        if (lane == 0) bc[2 * band] = c_occ, bc[2 * band + 1] = c_in;
    }
}

}  // namespace lslam
