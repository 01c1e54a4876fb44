// lslam_corr.h — the correlative-search core of the scan matcher (lslam_match.h) and the scan-to-map
// matcher (lslam_mapmatch.h, and through it lslam_mapfuse.h and the fine stage of lslam_reloc.h): a
// look-up grid G in LDS, a score per whole-cell shift and rotation of a revolution laid onto it, and
// the winner of the score volume.  The definitions are the comments on lslam_scan_match and
// lslam_map_match in include/lidarslam.h.  Here, once:
//   CorrGeom                        the geometry of a search, filled by corr_geometry (lslam_launch_map.h)
//   match_grid_bytes ...            the LDS layout
//   corr_smear_rows, _cols          occupancy -> G
//   match_tile_task                 a thread's 16 candidates against its share of a tile's points
//   match_best, corr_block_max      the winner's key, a block-wide 64-bit maximum
//   match_decode, match_winner      key -> k, jy, jx and score; their refinement to delta and EDGE
//   match_store                     delta and best to HBM
// A search kernel keeps the occupancy of G from its own source (the previous revolution, or the
// window of a map) and its own loop over the rotations and the tiles of the points, whose body is
// the same in both but for the three lines that turn a point into a cell of G.  The loop was one
// function here (and match_search_kernel called the smear passes below); both search kernels then
// ran 0.25-0.8 % slower at 4096 robots than with the loop in the kernel, and match_search_kernel
// 0.4 % slower with the shared smear passes alone: DESIGN §5.  So the loop stands in each kernel,
// and match_search_kernel keeps its smear passes inline: its instructions are those it had before
// there was a core.  A change to the loop or to a smear pass goes into both places.
//
// LDS of a search kernel: G at 2 bits per cell, W = win_w + 2 k_trans cells a side (a zero apron of
// k_trans cells, so a point whose own cell is inside the grid needs no bounds test under any
// translation), rows of Sd dwords (16 cells each; Sd odd, so the rows that a wave's tasks read fall
// on different banks) -- 74,480 B at the defaults -- then one tile of 512 staged points (2 KiB),
// whatever the kernel keeps of its own (the map matcher: 48 B), four counters and the rotation's
// Nt x Nt scores: 78,308 B without that, at most 81,788.  Two workgroups share a CU's 160 KiB.
//
// G is built in place, no second bitmap:
//   1. occupancy: LDS atomicOr of bit 0 of the cell (the kernel's own part);
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
// Search, per rotation: each thread transforms and quantises one point of the tile; a wave compacts
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

#include "lslam_wave.h"

namespace lslam {

constexpr int MATCH_TPB = 512;   // threads per search workgroup
constexpr int MATCH_TILE = 512;  // points staged per tile: one per thread
constexpr int MATCH_PICK_TPB = 256;

struct CorrGeom {
    double inv, cell, theta_step;
    int n;          // robots: score volumes, and n * n_slices search workgroups
    int win_w;      // cells a side of the look-up grid: the scan matcher's grid_w, the map matcher's win_w
    int half, smear, kt, kth, Nt, Nth;
    int W;          // win_w + 2 kt: cells a side with the apron
    int Sd;         // dwords per row of G
    int n_slices;   // workgroups per robot
    int per_slice;  // rotations per workgroup
    int32_t *scores;  // [n_robots][Nth][Nt][Nt]: the caller's, or the context's scratch
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

// Step 2, the row pass (only the grid's rows hold anything): each thread sweeps whole rows and
// leaves the ROW value max(0, smear + 1 - |dx| to the nearest occupied cell of the row).
__device__ __forceinline__ void corr_smear_rows(const CorrGeom &g, uint32_t *G, int tid) {
    const int kt = g.kt, gw = g.win_w, Sd = g.Sd, sm = g.smear;
    for (int row = kt + tid; row < kt + gw; row += MATCH_TPB) {
        uint32_t *p = G + row * Sd;
        uint32_t P = 0u, c = p[0];
        for (int d = 0; d < Sd; d++) {
            const uint32_t N = d + 1 < Sd ? p[d + 1] : 0u;
            const uint32_t h1 = c | (c << 2) | (P >> 30) | (c >> 2) | (N << 30);
            const uint32_t h2 = h1 | (c << 4) | (P >> 28) | (c >> 4) | (N << 28);
            const uint32_t q1 = sm == 0 ? c : (sm == 1 ? h1 : h2);
            const uint32_t q2 = sm == 0 ? 0u : (sm == 1 ? c : h1);
            const uint32_t q3 = sm == 2 ? c : 0u;
            p[d] = match_code(q1, q2, q3);
            P = c;
            c = N;
        }
    }
}

// Step 3, the column pass (it holds a barrier: every thread of the workgroup calls it):
// G = max over |dy| <= smear of min(row value(y + dy), smear + 1 - |dy|), the apron masked back to
// zero.
__device__ __forceinline__ void corr_smear_cols(const CorrGeom &g, uint32_t *G, int tid) {
    const int kt = g.kt, gw = g.win_w, W = g.W, Sd = g.Sd, sm = g.smear;
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
            uint32_t a1, a2, a3, b1, b2, b3, c1, c2, c3, d1, d2, d3, e1, e2, e3;
            match_planes(m2, a1, a2, a3);
            match_planes(m1, b1, b2, b3);
            match_planes(c, c1, c2, c3);
            match_planes(p1, d1, d2, d3);
            match_planes(p2, e1, e2, e3);
            uint32_t q1 = c1, q2 = c2;
            if (sm >= 1) q1 |= b1 | d1;
            if (sm >= 2) {
                q1 |= a1 | e1;
                q2 |= b2 | d2;
            }
            const bool inrow = y >= kt && y < kt + gw;
            G[y * Sd + col] = inrow ? (match_code(q1, q2, c3) & cmask) : 0u;
            m2 = m1;
            m1 = c;
            c = p1;
            p1 = p2;
        }
    }
}

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

// winner's key, most significant field first: score, 2047 - d^2 (d^2 <= 31^2 + 2 * 15^2 = 1411),
// 65535 - flat index (flat < 63 * 31^2 = 60543): the maximum is the highest score, then the
// smallest d^2, then the smallest flat index
__device__ __forceinline__ unsigned long long match_key(int score, int d2, int flat) {
    return ((unsigned long long)(uint32_t)score << 27) | ((unsigned long long)(2047 - d2) << 16) |
           (unsigned long long)(65535 - flat);
}

// flat index of the score volume -> rotation k, row jy, column jx
__device__ __forceinline__ void match_unflat(const CorrGeom &g, int flat, int &k, int &jy, int &jx) {
    const int Nt = g.Nt, Nt2 = Nt * Nt;
    k = flat / Nt2;
    const int rem = flat - k * Nt2;
    jy = rem / Nt;
    jx = rem - jy * Nt;
}

// The largest value of the workgroup's NW waves, in every thread (every thread calls it).  wk: one
// slot per wave, not in use: a caller in a loop puts a barrier between its rounds.
template <int NW>
__device__ __forceinline__ unsigned long long corr_block_max(unsigned long long v, unsigned long long *wk, int tid) {
    v = wave_max_u64(v);
    if ((tid & 63) == 0) wk[tid >> 6] = v;
    __syncthreads();
    v = wk[0];
#pragma unroll
    for (int w = 1; w < NW; w++) v = wk[w] > v ? wk[w] : v;
    return v;
}

// the winner's key of robot volume S, in every thread of a MATCH_PICK_TPB workgroup
__device__ __forceinline__ unsigned long long match_best(const CorrGeom &g, const int32_t *S, unsigned long long *wk,
                                                         int tid) {
    const int n = g.Nth * g.Nt * g.Nt, kt = g.kt, kth = g.kth;
    unsigned long long best = 0ull;
    for (int i = tid; i < n; i += MATCH_PICK_TPB) {
        int k, jy, jx;
        match_unflat(g, i, k, jy, jx);
        const int d2 = (k - kth) * (k - kth) + (jy - kt) * (jy - kt) + (jx - kt) * (jx - kt);
        const unsigned long long key = match_key(S[i], d2, i);
        best = key > best ? key : best;
    }
    return corr_block_max<MATCH_PICK_TPB / 64>(best, wk, tid);
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

// The winner: its candidate and score (match_decode, of the key, in any thread), then its refined
// delta (dx, dy, dtheta) and whether it lies on the window's border along some axis (match_winner,
// in the one thread that writes the robot's outputs).  A score of 0 (nothing matched) gives the
// centre and delta = 0.
struct MatchWinner {
    int flat, k, jy, jx, s0;
    bool edge;
    double d[3];
};
__device__ __forceinline__ MatchWinner match_decode(const CorrGeom &g, unsigned long long best) {
    MatchWinner w;
    w.flat = 65535 - (int)(best & 0xffffull);
    w.s0 = (int)(best >> 27);
    match_unflat(g, w.flat, w.k, w.jy, w.jx);
    w.edge = false;
    w.d[0] = w.d[1] = w.d[2] = 0.0;
    return w;
}
__device__ __forceinline__ void match_winner(const CorrGeom &g, const int32_t *S, MatchWinner &w) {
    const int Nt = g.Nt, kt = g.kt, kth = g.kth;
    if (w.s0 == 0) {
        w.k = kth;
        w.jy = kt;
        w.jx = kt;
        return;
    }
    const double ex = match_refine(S, w.jx, Nt, w.flat, 1, w.s0, w.edge);
    const double ey = match_refine(S, w.jy, Nt, w.flat, Nt, w.s0, w.edge);
    const double et = match_refine(S, w.k, g.Nth, w.flat, Nt * Nt, w.s0, w.edge);
    w.d[0] = ((double)(w.jx - kt) + ex) * g.cell;
    w.d[1] = ((double)(w.jy - kt) + ey) * g.cell;
    w.d[2] = ((double)(w.k - kth) + et) * g.theta_step;
}

// robot r's delta and best
__device__ __forceinline__ void match_store(const MatchWinner &w, double *delta, int32_t *best, int r) {
    delta[3 * r] = w.d[0];
    delta[3 * r + 1] = w.d[1];
    delta[3 * r + 2] = w.d[2];
    best[4 * r] = w.k;
    best[4 * r + 1] = w.jy;
    best[4 * r + 2] = w.jx;
    best[4 * r + 3] = w.s0;
}

}  // namespace lslam
