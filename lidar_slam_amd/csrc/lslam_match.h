// lslam_match.h — batched correlative scan matching (LiDAR-only odometry): two consecutive
// revolutions of a robot -> the motion between them.  The definition (grid, score volume,
// winner, refinement, flags, wheel speeds) is the comment on lslam_scan_match in
// include/lidarslam.h; tests/scanmatch_ref.py is its NumPy form.
//
// The LDS layout, a thread's task against a tile (match_tile_task), the winner's key, its
// refinement and the geometry are lslam_corr.h's, which the scan-to-map matcher uses too.  This
// header holds the occupancy of G from the previous revolution, the smear passes and the loop over
// rotations and tiles written into match_search_kernel (lslam_corr.h says why they are not calls),
// and the flags and wheel speeds.
//
// Kernels:
//   match_search_kernel  one 512-thread workgroup per (robot, slice of rotations): builds the
//                        look-up grid G in LDS and writes its rotations' scores
//   match_pick_kernel    one workgroup per robot: winner (one 64-bit key maximum), parabola
//                        refinement, flags, wheel speeds
//
// LDS of match_search_kernel: lslam_corr.h's layout with nothing of its own, 78,308 B at the
// defaults, at most 81,788.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_corr.h"
#include "lslam_wave.h"

namespace lslam {

struct MatchArgs {
    lslam_match_batch b;
    CorrGeom g;         // win_w: grid_w
    double dt, wr, wb;  // wheel speeds (write_u)
    int write_u;
};

__global__ __launch_bounds__(MATCH_TPB) void match_search_kernel(const MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const CorrGeom &g = a.g;
    const int W = g.W, Sd = g.Sd, kt = g.kt, half = g.half, gw = g.win_w, sm = g.smear;
    const int S = Sd * 16;  // cells per row
    uint32_t *G = (uint32_t *)smem;
    uint32_t *stage = (uint32_t *)(smem + match_grid_bytes(W, Sd));
    int *cnt = (int *)(stage + MATCH_TILE);  // [0], [1]: the tile's lists; [2], [3]: valid ref / cur points
    const int tid = (int)threadIdx.x;
    const int r = (int)blockIdx.x / g.n_slices, slice = (int)blockIdx.x - r * g.n_slices;
    const int r0 = a.b.ref_off[r], r1 = a.b.ref_off[r + 1];
    const int c0 = a.b.cur_off[r], c1 = a.b.cur_off[r + 1];
    const double2 *ref = (const double2 *)a.b.ref_xy, *cur = (const double2 *)a.b.cur_xy;
    const double inv = g.inv, dh = (double)half, dk = (double)(half + kt);

    for (int i = tid; i < W * Sd; i += MATCH_TPB) G[i] = 0u;
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();

    // ---- 1. occupancy ----
    int nv = 0;
    for (int p = r0 + tid; p < r1; p += MATCH_TPB) {
        const double2 q = ref[p];
        if (!match_valid(q)) continue;
        nv++;
        const double fx = floor(q.x * inv), fy = floor(q.y * inv);
        if (fx >= -dh && fx < dh && fy >= -dh && fy < dh) {  // in doubles: the conversions below cannot overflow
            const int gx = (int)fx + half + kt, gy = (int)fy + half + kt;
            atomicOr(&G[gy * Sd + (gx >> 4)], 1u << ((gx & 15) * 2));
        }
    }
    if (slice == 0) {  // n_valid: one workgroup per robot writes it
        int nc = 0;
        for (int p = c0 + tid; p < c1; p += MATCH_TPB) nc += match_valid(cur[p]) ? 1 : 0;
        if (nv) atomicAdd(&cnt[2], nv);
        if (nc) atomicAdd(&cnt[3], nc);
    }
    __syncthreads();
    if (slice == 0 && tid < 2) a.b.n_valid[2 * r + tid] = cnt[2 + tid];

    // ---- 2. rows (only the grid's rows hold anything) ----
    for (int row = kt + tid; row < kt + gw; row += MATCH_TPB) {
        uint32_t *g = G + row * Sd;
        uint32_t P = 0u, c = g[0];
        for (int d = 0; d < Sd; d++) {
            const uint32_t N = d + 1 < Sd ? g[d + 1] : 0u;
            const uint32_t h1 = c | (c << 2) | (P >> 30) | (c >> 2) | (N << 30);
            const uint32_t h2 = h1 | (c << 4) | (P >> 28) | (c >> 4) | (N << 28);
            const uint32_t q1 = sm == 0 ? c : (sm == 1 ? h1 : h2);
            const uint32_t q2 = sm == 0 ? 0u : (sm == 1 ? c : h1);
            const uint32_t q3 = sm == 2 ? c : 0u;
            g[d] = match_code(q1, q2, q3);
            P = c;
            c = N;
        }
    }
    __syncthreads();

    // ---- 3. columns ----
    {
        const int nseg = MATCH_TPB / Sd;  // Sd <= 35: at least 14 segments
        const int seg_rows = (W + nseg - 1) / nseg;
        const int col = tid % Sd, seg = tid / Sd;
        const int y0 = seg * seg_rows, y1 = min(W, y0 + seg_rows);
        const bool on = seg < nseg && y0 < y1;
        uint32_t m2 = 0u, m1 = 0u, hp0 = 0u, hp1 = 0u;
        if (on) {
            if (y0 >= 2) m2 = G[(y0 - 2) * Sd + col];
            if (y0 >= 1) m1 = G[(y0 - 1) * Sd + col];
            if (y1 < W) hp0 = G[y1 * Sd + col];
            if (y1 + 1 < W) hp1 = G[(y1 + 1) * Sd + col];
        }
        __syncthreads();
        if (on) {
            // cells of this dword column inside the grid
            const int lo = min(max(kt - col * 16, 0), 16), hi = min(max(kt + gw - col * 16, 0), 16);
            const uint32_t mlo = lo >= 16 ? ~0u : ((1u << (2 * lo)) - 1u), mhi = hi >= 16 ? ~0u : ((1u << (2 * hi)) - 1u);
            const uint32_t cmask = mhi & ~mlo;
            uint32_t c = G[y0 * Sd + col];
            uint32_t p1 = y0 + 1 < y1 ? G[(y0 + 1) * Sd + col] : hp0;
            for (int y = y0; y < y1; y++) {
                const int yn = y + 2;
                const uint32_t p2 = yn < y1 ? G[yn * Sd + col] : (yn == y1 ? hp0 : hp1);
                uint32_t a1, a2, a3, b1, b2, b3, c1_, c2_, c3_, d1, d2, d3, e1, e2, e3;
                match_planes(m2, a1, a2, a3);
                match_planes(m1, b1, b2, b3);
                match_planes(c, c1_, c2_, c3_);
                match_planes(p1, d1, d2, d3);
                match_planes(p2, e1, e2, e3);
                uint32_t q1 = c1_, q2 = c2_;
                if (sm >= 1) q1 |= b1 | d1;
                if (sm >= 2) {
                    q1 |= a1 | e1;
                    q2 |= b2 | d2;
                }
                const bool inrow = y >= kt && y < kt + gw;
                G[y * Sd + col] = inrow ? (match_code(q1, q2, c3_) & cmask) : 0u;
                m2 = m1;
                m1 = c;
                c = p1;
                p1 = p2;
            }
        }
    }
    __syncthreads();

    // ---- search ----
    const int Nt = g.Nt, Nt2 = Nt * Nt;
    int *sc = cnt + 4;  // [Nt][Nt] this rotation's scores
    // tasks (row jy, 16 jx from jxb) x point shares: 42 tasks x 12 shares at the default window
    const int ngrp = (Nt + 15) >> 4, ntask = Nt * ngrp, npg = MATCH_TPB / ntask;  // ntask <= 62
    const int task = tid % ntask, pg = tid / ntask;
    const int jy = task % Nt, jxb = 16 * (task / Nt);
    const int lofs = (jy - kt) * S + (jxb - kt);
    const int lane = tid & 63;
    const int kbeg = slice * g.per_slice, kend = min(g.Nth, kbeg + g.per_slice);
    for (int k = kbeg; k < kend; k++) {
        const double rc = a.b.rot[2 * k], rs = a.b.rot[2 * k + 1];
        __syncthreads();  // the previous rotation's scores are written out
        for (int i = tid; i < Nt2; i += MATCH_TPB) sc[i] = 0;
        for (int t0 = c0; t0 < c1; t0 += MATCH_TILE) {
            __syncthreads();  // the previous tile's readers are done
            if (tid < 2) cnt[tid] = 0;
            __syncthreads();
            const int p = t0 + tid;
            bool fast = false, slow = false;
            int axb = 0, ayb = 0;
            if (p < c1) {
                const double2 q = cur[p];
                if (match_valid(q)) {
                    const double xr = rc * q.x - rs * q.y;
                    const double yr = rs * q.x + rc * q.y;
                    const double ax = floor(xr * inv), ay = floor(yr * inv);
                    if (ax >= -dk && ax < dk && ay >= -dk && ay < dk) {  // can reach the grid (in doubles)
                        axb = (int)ax + half + kt;
                        ayb = (int)ay + half + kt;
                        fast = axb >= kt && axb < kt + gw && ayb >= kt && ayb < kt + gw;
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

__global__ __launch_bounds__(MATCH_PICK_TPB) void match_pick_kernel(const MatchArgs a) {
    __shared__ unsigned long long wk[MATCH_PICK_TPB / 64];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const CorrGeom &g = a.g;
    const int32_t *S = g.scores + (int64_t)r * (g.Nth * g.Nt * g.Nt);
    MatchWinner w = match_decode(g, match_best(g, S, wk, tid));
    if (tid != 0) return;
    match_winner(g, S, w);
    // a score of 0: nothing matched (no valid point on one side, or no current point on an occupied cell)
    const int flags = w.s0 == 0 ? LSLAM_MATCH_EMPTY : (w.edge ? LSLAM_MATCH_EDGE : 0);
    match_store(w, a.b.delta, a.b.best, r);
    a.b.flags[r] = flags;
    if (a.write_u) {  // the inverse of fx (lslam_ukf.h): x += dt B(theta) u
        double u0 = 0.0, u1 = 0.0;
        if (!(flags & LSLAM_MATCH_EMPTY)) {
            const double fa = w.d[0] / (a.wr * a.dt);
            const double fb = w.d[2] * a.wb / (2.0 * a.wr * a.dt);
            u0 = fa - fb;
            u1 = fa + fb;
        }
        a.b.ukf_u[2 * r] = u0;
        a.b.ukf_u[2 * r + 1] = u1;
    }
}

}  // namespace lslam
