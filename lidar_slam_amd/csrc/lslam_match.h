// lslam_match.h — batched correlative scan matching (LiDAR-only odometry): two consecutive
// revolutions of a robot -> the motion between them.  The definition (grid, score volume,
// winner, refinement, flags, wheel speeds) is the comment on lslam_scan_match in
// include/lidarslam.h; tests/scanmatch_ref.py is its NumPy form.
//
// Kernels:
//   match_search_kernel  one 512-thread workgroup per (robot, slice of rotations): builds the
//                        look-up grid G in LDS and writes its rotations' scores
//   match_pick_kernel    one workgroup per robot: winner (one 64-bit key maximum), parabola
//                        refinement, flags, wheel speeds
//
// LDS of match_search_kernel: G at 2 bits per cell, W = grid_w + 2 k_trans cells a side (a zero
// apron of k_trans cells, so a point whose own cell is inside the grid needs no bounds test under
// any translation), rows of Sd dwords (16 cells each; Sd odd, so the rows that a wave's tasks read
// fall on different banks) -- 74,480 B at the defaults -- then one tile of 512 staged points
// (2 KiB), four counters and the rotation's Nt x Nt scores: 78,308 B, at most 81,788.  Two
// workgroups share a CU's 160 KiB.
//
// G is built in place, no second bitmap:
//   1. occupancy: LDS atomicOr of bit 0 of the cell;
//   2. rows: each thread sweeps whole rows left to right (the previous dword's old value kept
//      in a register) and leaves the ROW value vh = max(0, smear + 1 - |dx| to the nearest
//      occupied cell of the row), from the bit planes o, o dilated by 1, o dilated by 2:
//      the planes are nested, so their sum is the 2-bit code;
//   3. columns: G = max over |dy| <= smear of min(vh(y + dy), smear + 1 - |dy|), again on the
//      planes (vh >= j) of the 2-bit codes: a thread owns a dword column over a segment of rows,
//      reads the two rows above and below its segment before the barrier (its neighbours
//      overwrite them), then sweeps downwards through a five-row register window.  The write
//      masks the apron back to zero (the smear is clipped to the grid).
//
// Search, per rotation: each thread rotates and quantises one point of the tile; a wave compacts
// its points with a ballot (one LDS atomicAdd per wave and list) into the tile's two lists:
// from the front the points whose own cell is inside the grid, as one cell offset; from the back
// those up to k_trans cells outside it (they enter the grid under some translations), as packed
// coordinates with a bounds test per look-up.  Translations are then integer shifts.  A thread's
// task is one row jy of the translation window and 16 consecutive jx: for a point these are 16
// consecutive cells of one row of G, i.e. 32 bits of a 64-bit window (two dwords, v_alignbit), so
// one LDS read serves 16 candidates; their 2-bit values are summed in packed 4-bit fields, then
// bytes, then LDS atomicAdd into the rotation's scores.  The default window has 21 x 2 = 42 tasks;
// the 512 threads are 12 shares of the tile's points for each (lanes of one share read the same
// staged point: a broadcast).  First form, measured: one candidate per lane and a ds_read_b32 per
// cell, 10.8 ms for 4096 robots against 3.47 ms.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_wave.h"

namespace lslam {

constexpr int MATCH_TPB = 512;   // threads per search workgroup
constexpr int MATCH_TILE = 512;  // current points staged per tile: one per thread
constexpr int MATCH_PICK_TPB = 256;

struct MatchArgs {
    lslam_match_batch b;
    double inv, cell, theta_step;
    double dt, wr, wb;  // wheel speeds (write_u)
    int write_u;
    int grid_w, half, smear, kt, kth, Nt, Nth;
    int W;          // grid_w + 2 kt: cells a side with the apron
    int Sd;         // dwords per row of G
    int n_slices;   // workgroups per robot
    int per_slice;  // rotations per workgroup
    int32_t *scores;  // [n_scans][Nth][Nt][Nt]: the caller's, or the context's scratch
};

// LDS bytes of G (16-byte aligned: the staged tile follows)
__host__ __device__ static inline int match_grid_bytes(int W, int Sd) { return (W * Sd * 4 + 15) & ~15; }
static inline int match_row_dwords(int W) {
    const int d = (W + 15) / 16;
    return d | 1;
}
static inline int match_lds_bytes(int W, int Sd, int Nt) {
    return match_grid_bytes(W, Sd) + MATCH_TILE * 4 + 16 + Nt * Nt * 4;
}

__device__ __forceinline__ bool match_valid(double2 q) {
    return __builtin_isfinite(q.x) && __builtin_isfinite(q.y) && !(q.x == 0.0 && q.y == 0.0);
}

// the planes (v >= 1), (v >= 2), (v >= 3) of sixteen 2-bit codes, on the even bits
__device__ __forceinline__ void match_planes(uint32_t v, uint32_t &p1, uint32_t &p2, uint32_t &p3) {
    const uint32_t lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
    p1 = hi | lo;
    p2 = hi;
    p3 = hi & lo;
}
// nested planes (r3 within r2 within r1) -> 2-bit codes r1 + r2 + r3
__device__ __forceinline__ uint32_t match_code(uint32_t r1, uint32_t r2, uint32_t r3) {
    return (r2 << 1) | ((r1 ^ r2) | r3);
}

__device__ __forceinline__ int match_cell(const uint32_t *G, int c) { return (int)((G[c >> 4] >> ((c & 15) * 2)) & 3u); }

// A task = one row jy of the translation window and 16 consecutive jx of it (jxb ..): for a point
// they are 16 consecutive cells of one row of G, 32 bits of a 64-bit window.  The 2-bit values are
// summed in packed fields: 4-bit fields over at most 5 points (5 * 3 = 15), bytes over at most 17
// such groups (255), then LDS atomicAdd into the rotation's score array.
struct MatchBytes {
    uint32_t b0 = 0u, b1 = 0u, b2 = 0u, b3 = 0u;  // byte m: cells 4m, 4m + 2, 4m + 1, 4m + 3
    int groups = 0;
    __device__ __forceinline__ void add(uint32_t e, uint32_t o) {  // nibble n of e: cell 2n, of o: cell 2n + 1
        b0 += e & 0x0f0f0f0fu;
        b1 += (e >> 4) & 0x0f0f0f0fu;
        b2 += o & 0x0f0f0f0fu;
        b3 += (o >> 4) & 0x0f0f0f0fu;
        groups++;
    }
    __device__ __forceinline__ void flush(int *row, int jxb, int Nt) {
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const uint32_t bb = (c & 3) == 0 ? b0 : ((c & 3) == 1 ? b2 : ((c & 3) == 2 ? b1 : b3));
            const int v = (int)((bb >> (8 * (c >> 2))) & 0xffu);
            if (jxb + c < Nt && v) atomicAdd(&row[jxb + c], v);
        }
        b0 = b1 = b2 = b3 = 0u;
        groups = 0;
    }
};

// one task against its share (every npg-th entry from pg) of the tile's two lists
__device__ __forceinline__ void match_tile_task(const uint32_t *G, const uint32_t *stage, int nf, int ns, int pg, int npg,
                                                int lofs, int jy, int jxb, int kt, int Nt, int S, int W, int *sc) {
    int *row = sc + jy * Nt;
    MatchBytes acc;
    for (int i = pg; i < nf;) {
        uint32_t e = 0u, o = 0u;
        for (int q = 0; q < 5 && i < nf; q++, i += npg) {
            const int c = (int)stage[i] + lofs;
            const uint32_t lo = G[c >> 4], hi = G[(c >> 4) + 1];  // (one dword past G at most: the staged tile)
            const uint32_t w = __builtin_amdgcn_alignbit(hi, lo, (uint32_t)((c & 15) * 2));
            e += w & 0x33333333u;
            o += (w >> 2) & 0x33333333u;
        }
        acc.add(e, o);
        if (acc.groups == 17) acc.flush(row, jxb, Nt);
    }
    if (acc.groups) acc.flush(row, jxb, Nt);
    for (int j = pg; j < ns; j += npg) {
        const uint32_t e = stage[MATCH_TILE - 1 - j];
        const int gy = (int)(e >> 16) + jy - kt;
        if ((unsigned)gy >= (unsigned)W) continue;
        for (int c = 0; c < 16 && jxb + c < Nt; c++) {
            const int gx = (int)(e & 0xffffu) + jxb + c - kt;
            if ((unsigned)gx < (unsigned)W) {
                const int v = match_cell(G, gy * S + gx);
                if (v) atomicAdd(&row[jxb + c], v);
            }
        }
    }
}

__global__ __launch_bounds__(MATCH_TPB) void match_search_kernel(const MatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int W = a.W, Sd = a.Sd, kt = a.kt, half = a.half, gw = a.grid_w, sm = a.smear;
    const int S = Sd * 16;  // cells per row
    uint32_t *G = (uint32_t *)smem;
    uint32_t *stage = (uint32_t *)(smem + match_grid_bytes(W, Sd));
    int *cnt = (int *)(stage + MATCH_TILE);  // [0], [1]: the tile's lists; [2], [3]: valid ref / cur points
    const int tid = (int)threadIdx.x;
    const int r = (int)blockIdx.x / a.n_slices, slice = (int)blockIdx.x - r * a.n_slices;
    const int r0 = a.b.ref_off[r], r1 = a.b.ref_off[r + 1];
    const int c0 = a.b.cur_off[r], c1 = a.b.cur_off[r + 1];
    const double2 *ref = (const double2 *)a.b.ref_xy, *cur = (const double2 *)a.b.cur_xy;
    const double inv = a.inv, dh = (double)half, dk = (double)(half + kt);

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
    const int Nt = a.Nt, Nt2 = Nt * Nt;
    int *sc = cnt + 4;  // [Nt][Nt] this rotation's scores
    // tasks (row jy, 16 jx from jxb) x point shares: 42 tasks x 12 shares at the default window
    const int ngrp = (Nt + 15) >> 4, ntask = Nt * ngrp, npg = MATCH_TPB / ntask;  // ntask <= 62
    const int task = tid % ntask, pg = tid / ntask;
    const int jy = task % Nt, jxb = 16 * (task / Nt);
    const int lofs = (jy - kt) * S + (jxb - kt);
    const int lane = tid & 63;
    const int kbeg = slice * a.per_slice, kend = min(a.Nth, kbeg + a.per_slice);
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
        int32_t *out = a.scores + ((int64_t)r * a.Nth + k) * Nt2;
        for (int i = tid; i < Nt2; i += MATCH_TPB) out[i] = sc[i];
    }
}

// winner's key, most significant field first: score, 2047 - d^2 (d^2 <= 31^2 + 2 * 15^2 = 1411),
// 65535 - flat index (flat < 63 * 31^2 = 60543): the maximum is the highest score, then the
// smallest d^2, then the smallest flat index
__device__ __forceinline__ unsigned long long match_key(int score, int d2, int flat) {
    return ((unsigned long long)(uint32_t)score << 27) | ((unsigned long long)(2047 - d2) << 16) |
           (unsigned long long)(65535 - flat);
}

__device__ __forceinline__ unsigned long long match_shfl_xor(unsigned long long v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}

// parabola through (s-, s0, s+) along one axis of n candidates, the winner at index i
__device__ __forceinline__ double match_refine(const int32_t *S, int i, int n, int64_t at, int64_t stride, int s0,
                                               bool &edge) {
    if (i == 0 || i == n - 1) {
        edge = true;
        return 0.0;
    }
    const double sm = (double)S[at - stride], sp = (double)S[at + stride];
    const double den = sm - 2.0 * (double)s0 + sp;
    return den < 0.0 ? 0.5 * (sm - sp) / den : 0.0;
}

__global__ __launch_bounds__(MATCH_PICK_TPB) void match_pick_kernel(const MatchArgs a) {
    __shared__ unsigned long long wk[MATCH_PICK_TPB / 64];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int Nt = a.Nt, Nt2 = Nt * Nt, n = a.Nth * Nt2, kt = a.kt, kth = a.kth;
    const int32_t *S = a.scores + (int64_t)r * n;
    unsigned long long best = 0ull;
    for (int i = tid; i < n; i += MATCH_PICK_TPB) {
        const int k = i / Nt2, rem = i - k * Nt2, jy = rem / Nt, jx = rem - jy * Nt;
        const int d2 = (k - kth) * (k - kth) + (jy - kt) * (jy - kt) + (jx - kt) * (jx - kt);
        const unsigned long long key = match_key(S[i], d2, i);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = match_shfl_xor(best, o);
        best = v > best ? v : best;
    }
    if ((tid & 63) == 0) wk[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < MATCH_PICK_TPB / 64; w++) best = wk[w] > best ? wk[w] : best;
    const int flat = 65535 - (int)(best & 0xffffull), s0 = (int)(best >> 27);
    int k = flat / Nt2, jy = (flat - k * Nt2) / Nt, jx = flat - k * Nt2 - jy * Nt;
    double dx = 0.0, dy = 0.0, dth = 0.0;
    int flags = 0;
    if (s0 == 0) {  // nothing matched: no valid point on one side, or no current point on an occupied cell
        flags = LSLAM_MATCH_EMPTY;
        k = kth;
        jy = kt;
        jx = kt;
    } else {
        bool edge = false;
        const double ex = match_refine(S, jx, Nt, flat, 1, s0, edge);
        const double ey = match_refine(S, jy, Nt, flat, Nt, s0, edge);
        const double et = match_refine(S, k, a.Nth, flat, Nt2, s0, edge);
        dx = ((double)(jx - kt) + ex) * a.cell;
        dy = ((double)(jy - kt) + ey) * a.cell;
        dth = ((double)(k - kth) + et) * a.theta_step;
        if (edge) flags |= LSLAM_MATCH_EDGE;
    }
    a.b.delta[3 * r] = dx;
    a.b.delta[3 * r + 1] = dy;
    a.b.delta[3 * r + 2] = dth;
    a.b.best[4 * r] = k;
    a.b.best[4 * r + 1] = jy;
    a.b.best[4 * r + 2] = jx;
    a.b.best[4 * r + 3] = s0;
    a.b.flags[r] = flags;
    if (a.write_u) {  // the inverse of fx (lslam_ukf.h): x += dt B(theta) u
        double u0 = 0.0, u1 = 0.0;
        if (!(flags & LSLAM_MATCH_EMPTY)) {
            const double fa = dx / (a.wr * a.dt);
            const double fb = dth * a.wb / (2.0 * a.wr * a.dt);
            u0 = fa - fb;
            u1 = fa + fb;
        }
        a.b.ukf_u[2 * r] = u0;
        a.b.ukf_u[2 * r + 1] = u1;
    }
}

}  // namespace lslam
