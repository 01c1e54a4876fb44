// lslam_mapmatch.h — batched scan-to-map matching: one revolution per robot, a pose guess and the
// robot's log-odds grid -> the pose that best lays the revolution onto the occupied cells.  The
// definition (robot cell, look-up window, score volume, winner, gate, output pose) is the comment on
// lslam_map_match in include/lidarslam.h; tests/mapmatch_ref.py is its NumPy form.
//
// It is the correlative search of lslam_match.h with the map in the place of the previous
// revolution, on the same core, lslam_corr.h: the LDS layout, the smear passes, match_tile_task, the
// winner's key and the refinement are that header's.  This header holds the occupancy of G from the
// map, the loop over rotations and tiles with its own point transform (match_search_kernel's loop
// but for those lines), and the gate and pose_out; lslam_mapfuse.h and the fine stage of
// lslam_reloc.h launch mapmatch_search_kernel and use mapmatch_flags.
//
// Kernels:
//   mapmatch_search_kernel  one 512-thread workgroup per (robot, slice of rotations): builds the
//                           look-up grid G of the window in LDS from the map in HBM and writes its
//                           rotations' scores
//   mapmatch_pick_kernel    one workgroup per robot: winner, parabola refinement, gate, flags and
//                           pose_out
//
// LDS of mapmatch_search_kernel: lslam_corr.h's layout, and of its own the robot's six doubles of
// the point transform between the staged tile and the counters (pose, origin and robot cell: read
// back per point, which keeps them out of the scalar registers that the search loop has none left
// of): 78,356 B at the defaults, at most 81,836, two workgroups per CU.
//
// Two parts differ from match_search_kernel:
//   occupancy  the window's cells come from the robot's int16 grid.  The window's first column
//              X0 - half has any alignment against the 16-cell dwords of G (which the apron shifts
//              as well) and against the 16-byte groups of a map row.  With rows on 16-byte
//              boundaries (grid_w a multiple of 8) a lane reads one map-aligned group of 8 cells
//              (consecutive lanes: consecutive groups of a row), thresholds them to 8 bits on the
//              even positions of a 16-bit word, clears the cells outside the window, and ORs the
//              word, shifted to its column, into the one or two dwords of G it straddles (LDS
//              atomicOr).  Otherwise a lane per cell.  Only the rows and columns of the window that
//              lie on the map are read: 512 KiB per workgroup at most.  The occupied cells are
//              counted on the way (popcount), and slice 0 writes the sum.
//   points     a point is rotated by the guess's heading composed with the rotation candidate,
//              moved to the world frame and quantised in the map's grid; its offset from the robot
//              cell is what match_search_kernel's robot-frame cell is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_corr.h"
#include "lslam_wave.h"

namespace lslam {

// LDS bytes: match_search_kernel's, and six doubles between the staged tile and the counters
static inline int mapmatch_lds_bytes(int W, int Sd, int Nt) { return match_lds_bytes(W, Sd, Nt) + 48; }

struct MapMatchArgs {
    lslam_mapmatch_batch b;
    CorrGeom g;     // win_w: the window's
    int map_w;      // cells per side of the map
    int occ_min, min_permille;
    int vec;        // rows of logodds lie on 16-byte boundaries
};

// lslam_grid_update step 0: the robot cell as doubles, and whether the pose is usable
__device__ __forceinline__ bool mapmatch_robot_cell(double px, double py, double th, double ox, double oy, double inv,
                                                    double &X0d, double &Y0d) {
    X0d = floor((px - ox) * inv);
    Y0d = floor((py - oy) * inv);
    const bool finite5 = __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(th) &&
                         __builtin_isfinite(ox) && __builtin_isfinite(oy);
    return finite5 && fabs(X0d) < 1048576.0 && fabs(Y0d) < 1048576.0;
}

// bit 2j of the result: cell j of a 16-byte group of eight int16 cells holds L >= occ_min
__device__ __forceinline__ uint32_t mapmatch_threshold8(uint4 v, int occ_min) {
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int l0 = (int)(int16_t)(d[i] & 0xffffu), l1 = (int)d[i] >> 16;  // (the low half is the lower address)
        m |= (l0 >= occ_min ? 1u : 0u) << (4 * i);
        m |= (l1 >= occ_min ? 1u : 0u) << (4 * i + 2);
    }
    return m;
}

__global__ __launch_bounds__(MATCH_TPB) void mapmatch_search_kernel(const MapMatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const CorrGeom &g = a.g;
    const int W = g.W, Sd = g.Sd, kt = g.kt, half = g.half, ww = g.win_w, mw = a.map_w;
    const int S = Sd * 16;  // cells per row
    uint32_t *G = (uint32_t *)smem;
    uint32_t *stage = (uint32_t *)(smem + match_grid_bytes(W, Sd));
    double *wp = (double *)(stage + MATCH_TILE);  // px, py, ox, oy, X0, Y0
    int *cnt = (int *)(wp + 6);  // [0], [1]: the tile's lists; [2], [3]: occupied cells / valid points
    const int tid = (int)threadIdx.x;
    const int r = (int)blockIdx.x / g.n_slices, slice = (int)blockIdx.x - r * g.n_slices;
    const int Nt = g.Nt, Nt2 = Nt * Nt;
    const int kbeg = slice * g.per_slice, kend = min(g.Nth, kbeg + g.per_slice);

    // ---- 0. pose, rotation, robot cell ----
    const double px = a.b.pose[3 * r], py = a.b.pose[3 * r + 1], th = a.b.pose[3 * r + 2];
    const double ox = a.b.origin[2 * r], oy = a.b.origin[2 * r + 1];
    const double inv = g.inv;
    const double c = cos(th), s = sin(th);  // (the same instructions in every workgroup: the same bits)
    if (slice == 0 && tid == 0) {
        a.b.rot0[2 * r] = c;
        a.b.rot0[2 * r + 1] = s;
    }
    double X0d, Y0d;
    if (!mapmatch_robot_cell(px, py, th, ox, oy, inv, X0d, Y0d)) {
        int32_t *out = g.scores + ((int64_t)r * g.Nth + kbeg) * Nt2;
        for (int i = tid; i < (kend - kbeg) * Nt2; i += MATCH_TPB) out[i] = 0;
        if (slice == 0 && tid < 2) a.b.n_valid[2 * r + tid] = 0;
        return;
    }
    const int X0 = (int)X0d, Y0 = (int)Y0d;
    const int p0 = a.b.pt_off[r], p1 = a.b.pt_off[r + 1];
    const double2 *xy = (const double2 *)a.b.xy;

    for (int i = tid; i < W * Sd; i += MATCH_TPB) G[i] = 0u;
    if (tid < 4) cnt[tid] = 0;
    if (tid == 0) {
        wp[0] = px;
        wp[1] = py;
        wp[2] = ox;
        wp[3] = oy;
        wp[4] = X0d;
        wp[5] = Y0d;
    }
    __syncthreads();

    // ---- 1. occupancy: the window's cells that lie on the map ----
    {
        const int wx0 = X0 - half, wy0 = Y0 - half;  // the map cell of window cell (0, 0); |X0| < 2^20
        const int mx0 = max(0, wx0), mx1 = min(mw, wx0 + ww);
        const int my0 = max(0, wy0), my1 = min(mw, wy0 + ww);
        const int16_t *L = a.b.logodds + (int64_t)r * mw * mw;
        const int occ_min = a.occ_min;
        int nocc = 0;
        if (mx0 < mx1 && my0 < my1) {
            const int nrows = my1 - my0;
            if (a.vec) {
                const int g0 = mx0 >> 3, ng = ((mx1 + 7) >> 3) - g0;  // map-aligned groups of 8 cells
                for (int idx = tid; idx < nrows * ng; idx += MATCH_TPB) {
                    const int row = idx / ng, cx = 8 * (g0 + idx - row * ng), my = my0 + row;
                    uint32_t m = mapmatch_threshold8(*(const uint4 *)(L + (int64_t)my * mw + cx), occ_min);
                    const int cut_lo = max(0, mx0 - cx), cut_hi = min(8, mx1 - cx);  // the group's cells in the window
                    m &= ~((1u << (2 * cut_lo)) - 1u) & ((1u << (2 * cut_hi)) - 1u);
                    if (!m) continue;
                    nocc += __popc(m);
                    int lc = cx - wx0 + kt;  // column in G of the group's first cell
                    if (lc < 0) {            // (its cells left of the window are cleared)
                        m >>= 2 * (-lc);
                        lc = 0;
                    }
                    const uint64_t w = (uint64_t)m << ((lc & 15) * 2);
                    uint32_t *gd = G + (my - wy0 + kt) * Sd + (lc >> 4);
                    if ((uint32_t)w) atomicOr(gd, (uint32_t)w);
                    if ((uint32_t)(w >> 32)) atomicOr(gd + 1, (uint32_t)(w >> 32));  // (a set bit there is a cell of this row)
                }
            } else {
                const int ncols = mx1 - mx0;
                for (int idx = tid; idx < nrows * ncols; idx += MATCH_TPB) {
                    const int row = idx / ncols, cx = mx0 + idx - row * ncols, my = my0 + row;
                    if ((int)L[(int64_t)my * mw + cx] < occ_min) continue;
                    nocc++;
                    const int lc = cx - wx0 + kt;
                    atomicOr(&G[(my - wy0 + kt) * Sd + (lc >> 4)], 1u << ((lc & 15) * 2));
                }
            }
        }
        if (slice == 0) {  // n_valid: one workgroup per robot writes it
            int nc = 0;
            for (int p = p0 + tid; p < p1; p += MATCH_TPB) nc += match_valid(xy[p]) ? 1 : 0;
            if (nocc) atomicAdd(&cnt[2], nocc);
            if (nc) atomicAdd(&cnt[3], nc);
        }
    }
    __syncthreads();
    if (slice == 0 && tid < 2) a.b.n_valid[2 * r + tid] = cnt[2 + tid];

    // ---- 2, 3. rows, columns ----
    corr_smear_rows(g, G, tid);
    __syncthreads();
    corr_smear_cols(g, G, tid);
    __syncthreads();

    // ---- search ----
    int *sc = cnt + 4;  // [Nt][Nt] this rotation's scores
    const int ngrp = (Nt + 15) >> 4, ntask = Nt * ngrp, npg = MATCH_TPB / ntask;  // ntask <= 62
    const int task = tid % ntask, pg = tid / ntask;
    const int jy = task % Nt, jxb = 16 * (task / Nt);
    const int lofs = (jy - kt) * S + (jxb - kt);
    const int lane = tid & 63;
    const double dk = (double)(half + kt);
    for (int k = kbeg; k < kend; k++) {
        const double ck = a.b.rot[2 * k], sk = a.b.rot[2 * k + 1];
        const double cc = c * ck - s * sk, ss = s * ck + c * sk;
        __syncthreads();  // the previous rotation's scores are written out
        for (int i = tid; i < Nt2; i += MATCH_TPB) sc[i] = 0;
        for (int t0 = p0; t0 < p1; t0 += MATCH_TILE) {
            __syncthreads();  // the previous tile's readers are done
            if (tid < 2) cnt[tid] = 0;
            __syncthreads();
            const int p = t0 + tid;
            bool fast = false, slow = false;
            int axb = 0, ayb = 0;
            if (p < p1) {
                const double2 q = xy[p];
                if (match_valid(q)) {
                    const double wx = wp[0] + (cc * q.x - ss * q.y);
                    const double wy = wp[1] + (ss * q.x + cc * q.y);
                    const double ax = floor((wx - wp[2]) * inv) - wp[4], ay = floor((wy - wp[3]) * inv) - wp[5];
                    if (ax >= -dk && ax < dk && ay >= -dk && ay < dk) {  // can reach the window (in doubles)
                        axb = (int)ax + half + kt;
                        ayb = (int)ay + half + kt;
                        fast = axb >= kt && axb < kt + ww && ayb >= kt && ayb < kt + ww;
                        slow = !fast;
                    }
                }
            }
            const uint64_t bf = ballot(fast), bs = ballot(slow);
            int basef = 0, bases = 0;
            if (lane == 0) {
                if (bf) basef = atomicAdd(&cnt[0], popc64(bf));
                if (bs) bases = atomicAdd(&cnt[1], popc64(bs));
            }
            basef = uni(basef);
            bases = uni(bases);
            if (fast) stage[basef + (int)mbcnt(bf)] = (uint32_t)(ayb * S + axb);
            if (slow) stage[MATCH_TILE - 1 - (bases + (int)mbcnt(bs))] = ((uint32_t)ayb << 16) | (uint32_t)axb;
            __syncthreads();
            if (pg < npg) match_tile_task(G, stage, cnt[0], cnt[1], pg, npg, lofs, jy, jxb, kt, Nt, S, W, sc);
        }
        __syncthreads();
        int32_t *out = g.scores + ((int64_t)r * g.Nth + k) * Nt2;
        for (int i = tid; i < Nt2; i += MATCH_TPB) out[i] = sc[i];
    }
}

__device__ __forceinline__ double mapmatch_bits(unsigned long long v) { return __longlong_as_double((long long)v); }

// Steps 3 and 4's flags of robot r's winner at pose (px, py, th): a score of 0 (no valid point on an
// occupied cell; a bad pose's scores are zeros) is BAD_POSE or EMPTY, alone; otherwise EDGE, and
// WEAK by the gate, in int64.  (Read after the search kernel: n_valid is final.)
__device__ __forceinline__ int mapmatch_flags(const MapMatchArgs &a, int r, const MatchWinner &w, double px, double py,
                                              double th) {
    if (w.s0 == 0) {
        double X0d, Y0d;
        const bool ok = mapmatch_robot_cell(px, py, th, a.b.origin[2 * r], a.b.origin[2 * r + 1], a.g.inv, X0d, Y0d);
        return ok ? LSLAM_MAPMATCH_EMPTY : LSLAM_MAPMATCH_BAD_POSE;
    }
    int flags = w.edge ? LSLAM_MAPMATCH_EDGE : 0;
    const long long nv = (long long)a.b.n_valid[2 * r + 1];
    if (1000ll * (long long)w.s0 < (long long)a.min_permille * (long long)(a.g.smear + 1) * nv) flags |= LSLAM_MAPMATCH_WEAK;
    return flags;
}

__global__ __launch_bounds__(MATCH_PICK_TPB) void mapmatch_pick_kernel(const MapMatchArgs a) {
    __shared__ unsigned long long wk[MATCH_PICK_TPB / 64];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const CorrGeom &g = a.g;
    const int32_t *S = g.scores + (int64_t)r * (g.Nth * g.Nt * g.Nt);
    MatchWinner w = match_decode(g, match_best(g, S, wk, tid));
    if (tid != 0) return;
    // this thread alone reads pose[r] and, below, writes pose_out[r]: they may be one buffer
    const unsigned long long *pin = (const unsigned long long *)a.b.pose + 3 * r;
    const unsigned long long bx = pin[0], by = pin[1], bt = pin[2];
    const double px = mapmatch_bits(bx), py = mapmatch_bits(by), th = mapmatch_bits(bt);
    match_winner(g, S, w);
    const int flags = mapmatch_flags(a, r, w, px, py, th);
    match_store(w, a.b.delta, a.b.best, r);
    a.b.flags[r] = flags;
    if (flags & (LSLAM_MAPMATCH_EMPTY | LSLAM_MAPMATCH_BAD_POSE | LSLAM_MAPMATCH_WEAK)) {
        unsigned long long *pout = (unsigned long long *)a.b.pose_out + 3 * r;
        pout[0] = bx;
        pout[1] = by;
        pout[2] = bt;
    } else {
        a.b.pose_out[3 * r] = px + w.d[0];
        a.b.pose_out[3 * r + 1] = py + w.d[1];
        a.b.pose_out[3 * r + 2] = th + w.d[2];
    }
}

}  // namespace lslam
