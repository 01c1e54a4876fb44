// lslam_reloc.h — global relocalisation in the occupancy grid: one revolution per robot and the
// robot's log-odds grid, no pose guess -> the K best separated peaks of a coarse correlative search
// over every coarse cell and every heading, for lslam_map_match to refine, and the selection among
// the refined poses.  The definition is the comment on lslam_map_relocalize in include/lidarslam.h;
// tests/reloc_ref.py is its NumPy form.
//
// Kernels:
//   reloc_search_kernel  one 512-thread workgroup per (robot, slice of headings): builds the coarse
//                        occupancy bitmap in LDS from the int16 map and writes its headings' scores
//   reloc_peak_kernel    one 256-thread workgroup per (robot, heading, 2048 cells of the heading's plane):
//                        the peaks among its cells and the K best of them as 64-bit keys
//   reloc_topk_kernel    one workgroup per robot: the K best keys of all its blocks, cand, cand_pose
//   reloc_select_kernel  one thread per robot: the winner among the refined ranks, the ambiguity
//                        test, pose_out and P_out
// The fine stage between the last two is the scan-to-map matcher's two kernels (launch_mapmatch_kernels),
// once per rank.  The coarse search is another algorithm than lslam_corr.h's (bit-sliced counters over
// a one-bit map, no smear); of that header it uses the block-wide key maximum, corr_block_max.
//
// reloc_search_kernel.  The bitmap holds one bit per coarse cell, Wc zero bits left of each row and
// at least Wc right of it, in rows of RW dwords (RW odd: consecutive rows start on different banks),
// and Wc zero rows above and below the map's.  With column c at bit c + Wc and row y at row y + Wc,
// the 32 cells tx0 .. tx0 + 31 of row ty seen through a point's offset (ay, ax), |ay|, |ax| < Wc,
// are the 32 bits from bit tx0 + ax + Wc of row ty + ay + Wc: two dwords and a funnel shift, no test
// per cell or per row.  tx0 is a multiple of 32, so the dword (ay + Wc) RW + ((ax + Wc) >> 5) and the
// shift (ax + Wc) & 31 are the point's alone: a heading's points are rotated and quantised once by
// the workgroup and staged as dword << 5 | shift, and a thread adds its own (ty RW + tx0 / 32).  A
// thread owns (ty, a span of 32 tx) and adds the windows of all staged points into bit-sliced
// counters: eight windows go through seven carry-save adders into the planes 1, 2, 4 and a carry of weight 8 that ripples into five more planes (Harley-Seal),
// about 5 logic operations per point and span instead of 32 additions.  After at most 248 points
// (8 planes) the planes are unpacked into 32 int32 sums, which are added to the volume in HBM at the
// end of the tile: a thread is the only writer of its cells.  RELOC form 1 (LSLAM_RELOC_FORM=add,
// tools/relocbench.py) is the plain form, one extraction and one addition per cell and point.
// LDS: 3 Wc * RW * 4 bytes of bitmap (76,800 at Wc = 256; 19,968 at 128), 8 KiB of staged points, 16 B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_mapmatch.h"
#include "lslam_wave.h"

namespace lslam {

constexpr int RELOC_TPB = 512;     // threads per search workgroup
constexpr int RELOC_TILE = 2048;   // points staged per tile
constexpr int RELOC_BATCH = 248;   // points per fill of the 8 planes (a multiple of 8, <= 255)
constexpr int RELOC_PEAK_TPB = 256;
constexpr int RELOC_PEAK_CELLS = 8;  // cells per thread of reloc_peak_kernel
constexpr int RELOC_PEAK_BLOCK = RELOC_PEAK_TPB * RELOC_PEAK_CELLS;
constexpr int RELOC_KMAX = 16;

struct RelocArgs {
    lslam_reloc_batch b;
    double invc, cellc, head_step, max_r2;
    double dup_mm, dup_rad, pxy, pth;  // pxy, pth: the diagonal of P_out
    int map_w, f, Wc, n_head, K, occ_min, ambig;
    int nspan;      // spans of 32 cells per coarse row
    int RW;         // dwords per row of the bitmap
    int n_slices;   // workgroups per robot
    int per_slice;  // headings per workgroup
    int vec;        // rows of logodds lie on 16-byte boundaries
    int form;       // 0: bit-sliced counters, 1: one addition per cell
    int r0;         // the chunk's first robot
    int nbh;        // blocks of reloc_peak_kernel per heading
    int nblk;       // and per robot: n_head * nbh
    int32_t *vol;              // [chunk][n_head][Wc][Wc]: the chunk's part of coarse_scores, or scratch
    unsigned long long *keys;  // [chunk][nblk][K] the blocks' best peaks
};

static inline int reloc_row_dwords(int Wc, int nspan) { return ((32 * nspan + 2 * Wc + 31) / 32 + 1) | 1; }
static inline int reloc_lds_bytes(int Wc, int RW) { return ((3 * Wc * RW + 3) & ~3) * 4 + RELOC_TILE * 4 + 16; }

// step 1: a point the coarse search uses
__device__ __forceinline__ bool reloc_used(double2 q, double max_r2) {
    return match_valid(q) && q.x * q.x + q.y * q.y <= max_r2;
}

// the thread's 32 cells (pb: its row ty and span in the bitmap) seen through the staged offset pk
__device__ __forceinline__ uint32_t reloc_window(const uint32_t *pb, uint32_t pk) {
    const uint32_t *p = pb + (pk >> 5);
    return (uint32_t)((((uint64_t)p[1] << 32) | (uint64_t)p[0]) >> (pk & 31u));
}

// carry-save adder: a + b + c = 2 h + l, bit by bit
__device__ __forceinline__ void reloc_csa(uint32_t &h, uint32_t &l, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t u = a ^ b;
    h = (a & b) | (u & c);
    l = u ^ c;
}

// acc[i] += the number of staged points [0, n8) whose window holds bit i; n8 is a multiple of 8
template <int FORM>
__device__ __forceinline__ void reloc_count(const uint32_t *pb, const uint32_t *stage, int n8, int (&acc)[32]) {
    if (FORM == 1) {
        for (int i = 0; i < n8; i++) {
            const uint32_t w = reloc_window(pb, stage[i]);
#pragma unroll
            for (int j = 0; j < 32; j++) acc[j] += (int)((w >> j) & 1u);
        }
        return;
    }
    for (int base = 0; base < n8; base += RELOC_BATCH) {
        const int end = min(n8, base + RELOC_BATCH);
        uint32_t p[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (int i = base; i < end; i += 8) {
            const uint4 q0 = *(const uint4 *)(stage + i), q1 = *(const uint4 *)(stage + i + 4);
            const uint32_t w0 = reloc_window(pb, q0.x), w1 = reloc_window(pb, q0.y);
            const uint32_t w2 = reloc_window(pb, q0.z), w3 = reloc_window(pb, q0.w);
            const uint32_t w4 = reloc_window(pb, q1.x), w5 = reloc_window(pb, q1.y);
            const uint32_t w6 = reloc_window(pb, q1.z), w7 = reloc_window(pb, q1.w);
            uint32_t tA, tB, fA, fB, e;
            reloc_csa(tA, p[0], p[0], w0, w1);
            reloc_csa(tB, p[0], p[0], w2, w3);
            reloc_csa(fA, p[1], p[1], tA, tB);
            reloc_csa(tA, p[0], p[0], w4, w5);
            reloc_csa(tB, p[0], p[0], w6, w7);
            reloc_csa(fB, p[1], p[1], tA, tB);
            reloc_csa(e, p[2], p[2], fA, fB);
#pragma unroll
            for (int j = 3; j < 8; j++) {  // (at most 248 points: no carry out of plane 7)
                const uint32_t t = p[j] & e;
                p[j] ^= e;
                e = t;
            }
        }
#pragma unroll
        for (int j = 0; j < 32; j++) {
            int v = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) v |= (int)((p[q] >> j) & 1u) << q;
            acc[j] += v;
        }
    }
}

// (relocprior_search_kernel, lslam_relocprior.h, holds a copy of the bitmap build, the n_occ / n_used block and
// the staging loop below: a fix here is a fix there.  This kernel's code is pinned, so nothing is shared yet.)
template <int FORM>
__global__ __launch_bounds__(RELOC_TPB) void reloc_search_kernel(const RelocArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Wc = a.Wc, RW = a.RW, mw = a.map_w, f = a.f;
    uint32_t *B = (uint32_t *)smem;
    const int nB = 3 * Wc * RW;  // dwords of the bitmap: Wc zero rows, the map's, Wc zero rows
    uint32_t *stage = B + ((nB + 3) & ~3);
    int *cnt = (int *)(stage + RELOC_TILE);  // [0]: staged points; [1], [2]: occupied coarse cells / used points
    const int tid = (int)threadIdx.x;
    const int rl = (int)blockIdx.x / a.n_slices, slice = (int)blockIdx.x - rl * a.n_slices;
    const int r = a.r0 + rl;
    const int kbeg = slice * a.per_slice, kend = min(a.n_head, kbeg + a.per_slice);
    const int p0 = a.b.pt_off[r], p1 = a.b.pt_off[r + 1];
    const double2 *xy = (const double2 *)a.b.xy;
    const double invc = a.invc, max_r2 = a.max_r2;

    for (int i = tid; i < nB; i += RELOC_TPB) B[i] = 0u;
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();

    // ---- 0. the coarse map: a set fine cell sets its coarse cell's bit ----
    {
        const int16_t *L = a.b.logodds + (int64_t)r * mw * mw;
        const int occ_min = a.occ_min;
        if (a.vec) {
            const int ng = mw >> 3, per = 8 / f;  // 16-byte groups per row; coarse cells per group (f = 2, 4, 8)
            const uint32_t sub = (1u << (2 * f)) - 1u;
            for (int idx = tid; idx < mw * ng; idx += RELOC_TPB) {
                const int y = idx / ng, g = idx - y * ng;
                const uint32_t m = mapmatch_threshold8(*(const uint4 *)(L + (int64_t)y * mw + 8 * g), occ_min);
                if (!m) continue;
                const int cy = y / f + Wc;
                for (int j = 0; j < per; j++)
                    if ((m >> (2 * f * j)) & sub) {
                        const int bit = g * per + j + Wc;
                        atomicOr(&B[cy * RW + (bit >> 5)], 1u << (bit & 31));
                    }
            }
        } else {
            for (int idx = tid; idx < mw * mw; idx += RELOC_TPB) {
                if ((int)L[idx] < occ_min) continue;
                const int y = idx / mw, x = idx - y * mw;
                const int bit = x / f + Wc;
                atomicOr(&B[(y / f + Wc) * RW + (bit >> 5)], 1u << (bit & 31));
            }
        }
    }
    __syncthreads();
    if (slice == 0) {  // n_occ and n_used: one workgroup per robot writes them
        int nocc = 0, nu = 0;
        for (int i = tid; i < nB; i += RELOC_TPB) nocc += __popc(B[i]);
        for (int p = p0 + tid; p < p1; p += RELOC_TPB) nu += reloc_used(xy[p], max_r2) ? 1 : 0;
        if (nocc) atomicAdd(&cnt[1], nocc);
        if (nu) atomicAdd(&cnt[2], nu);
        __syncthreads();
        if (tid == 0) {
            a.b.n_occ[r] = cnt[1];
            a.b.n_used[r] = cnt[2];
        }
    }

    // ---- 2. scores ----
    const int nspan = a.nspan, ntask = Wc * nspan;
    const int lane = tid & 63;
    const double dW = (double)Wc;
    const uint32_t null_pk = 0u;  // row ty of the bitmap: one of the zero rows above the map's
    for (int k = kbeg; k < kend; k++) {
        const double c = a.b.head_rot[2 * k], s = a.b.head_rot[2 * k + 1];
        int32_t *out = a.vol + ((int64_t)rl * a.n_head + k) * Wc * Wc;
        bool first = true;
        for (int t0 = p0; t0 < p1 || first; t0 += RELOC_TILE) {
            __syncthreads();  // the previous tile's readers are done
            if (tid == 0) cnt[0] = 0;
            __syncthreads();
            for (int p = t0 + tid; p < min(p1, t0 + RELOC_TILE); p += RELOC_TPB) {  // (uniform trip count per wave
                const double2 q = xy[p];                                            //  up to the last, partial one)
                bool on = false;
                uint32_t pk = 0u;
                if (reloc_used(q, max_r2)) {
                    const double xr = c * q.x - s * q.y, yr = s * q.x + c * q.y;
                    const double ax = floor(xr * invc + 0.5), ay = floor(yr * invc + 0.5);
                    if (ax > -dW && ax < dW && ay > -dW && ay < dW) {
                        on = true;
                        const int axp = (int)ax + Wc;
                        pk = ((uint32_t)(((int)ay + Wc) * RW + (axp >> 5)) << 5) | (uint32_t)(axp & 31);
                    }
                }
                if (on) stage[atomicAdd(&cnt[0], 1)] = pk;
            }
            __syncthreads();
            const int n = cnt[0], n8 = (n + 7) & ~7;
            if (tid < n8 - n) stage[n + tid] = null_pk;
            __syncthreads();
            for (int task = tid; task < ntask; task += RELOC_TPB) {
                const int ty = task / nspan, tx0 = 32 * (task - ty * nspan);
                int acc[32];
#pragma unroll
                for (int j = 0; j < 32; j++) acc[j] = 0;
                reloc_count<FORM>(B + ty * RW + (tx0 >> 5), stage, n8, acc);
                int32_t *o = out + ty * Wc + tx0;
                const int nx = min(32, Wc - tx0);
#pragma unroll
                for (int j = 0; j < 32; j++)
                    if (j < nx) o[j] = first ? acc[j] : o[j] + acc[j];
            }
            first = false;
        }
    }
}

// candidates in the definition's order: the larger key comes first
__device__ __forceinline__ unsigned long long reloc_key(int score, int flat) {
    return ((unsigned long long)(uint32_t)score << 32) | (unsigned long long)(0xffffffffu - (uint32_t)flat);
}

// the largest key of the workgroup in a loop of rounds (every thread calls it; wk: one slot per wave)
__device__ __forceinline__ unsigned long long reloc_block_max(unsigned long long v, unsigned long long *wk, int tid) {
    __syncthreads();  // the previous round's readers are done
    return corr_block_max<RELOC_PEAK_TPB / 64>(v, wk, tid);
}

__global__ __launch_bounds__(RELOC_PEAK_TPB) void reloc_peak_kernel(const RelocArgs a) {
    __shared__ unsigned long long wk[RELOC_PEAK_TPB / 64];
    const int tid = (int)threadIdx.x;
    const int rl = (int)blockIdx.x / a.nblk, blk = (int)blockIdx.x - rl * a.nblk;
    const int Wc = a.Wc, nh = a.n_head, W2 = Wc * Wc, n = nh * W2;
    const int32_t *S = a.vol + (int64_t)rl * n;
    const int k = blk / a.nbh, c0 = (blk - k * a.nbh) * RELOC_PEAK_BLOCK + tid;  // the heading; the thread's first cell
    // the thread's cells are RELOC_PEAK_TPB apart in the plane: one division, then steps of (sy, sx)
    const int sy = RELOC_PEAK_TPB / Wc, sx = RELOC_PEAK_TPB - sy * Wc;
    int ty = c0 / Wc, tx = c0 - ty * Wc;
    unsigned long long key[RELOC_PEAK_CELLS];
#pragma unroll
    for (int e = 0; e < RELOC_PEAK_CELLS; e++, ty += sy + (tx + sx >= Wc ? 1 : 0), tx += sx - (tx + sx >= Wc ? Wc : 0)) {
        const int c = c0 + e * RELOC_PEAK_TPB, i = k * W2 + c;
        key[e] = 0ull;
        if (c >= W2) continue;
        const int s0 = S[i];
        if (s0 <= 0) continue;
        bool peak = true;
        for (int d = 0; d < 3 && peak; d++) {  // the cell's own plane first: most candidates fall there
            const int dk = d == 0 ? 0 : (d == 1 ? -1 : 1);
            const int kk = k + dk < 0 ? nh - 1 : (k + dk >= nh ? 0 : k + dk);
            for (int dy = -1; dy <= 1 && peak; dy++) {
                const int yy = ty + dy;
                if (yy < 0 || yy >= Wc) continue;
                for (int dx = -1; dx <= 1; dx++) {
                    const int xx = tx + dx;
                    if (xx < 0 || xx >= Wc || (dk == 0 && dy == 0 && dx == 0)) continue;
                    const int j = (kk * Wc + yy) * Wc + xx;
                    const int sj = S[j];
                    if (sj > s0 || (sj == s0 && j < i)) peak = false;
                }
            }
        }
        if (peak) key[e] = reloc_key(s0, i);
    }
    unsigned long long *out = a.keys + ((int64_t)rl * a.nblk + blk) * a.K;
    unsigned long long last = ~0ull;
    for (int j = 0; j < a.K; j++) {
        unsigned long long m = 0ull;
        if (last) {  // (uniform: a round without a key ends the search)
#pragma unroll
            for (int e = 0; e < RELOC_PEAK_CELLS; e++) m = (key[e] < last && key[e] > m) ? key[e] : m;
            m = reloc_block_max(m, wk, tid);
        }
        if (tid == 0) out[j] = m;
        last = m;
    }
}

__global__ __launch_bounds__(RELOC_PEAK_TPB) void reloc_topk_kernel(const RelocArgs a) {
    __shared__ unsigned long long wk[RELOC_PEAK_TPB / 64];
    const int tid = (int)threadIdx.x, rl = (int)blockIdx.x, r = a.r0 + rl;
    const int Wc = a.Wc, W2 = Wc * Wc, K = a.K, R = a.b.n_robots;
    const int nkeys = a.nblk * K;
    const unsigned long long *keys = a.keys + (int64_t)rl * nkeys;
    const double ox = a.b.origin[2 * r], oy = a.b.origin[2 * r + 1];
    unsigned long long last = ~0ull;
    for (int j = 0; j < K; j++) {
        unsigned long long m = 0ull;
        if (last) {
            for (int i = tid; i < nkeys; i += RELOC_PEAK_TPB) {
                const unsigned long long v = keys[i];
                m = (v < last && v > m) ? v : m;
            }
            m = reloc_block_max(m, wk, tid);
        }
        last = m;
        if (tid != 0) continue;
        int32_t *cd = a.b.cand + ((int64_t)j * R + r) * 4;
        double *cp = a.b.cand_pose + ((int64_t)j * R + r) * 3;
        if (m) {
            const int score = (int)(m >> 32), flat = (int)(0xffffffffu - (uint32_t)m);
            const int k = flat / W2, rem = flat - k * W2, ty = rem / Wc, tx = rem - ty * Wc;
            cd[0] = k;
            cd[1] = ty;
            cd[2] = tx;
            cd[3] = score;
            cp[0] = ox + ((double)tx + 0.5) * a.cellc;
            cp[1] = oy + ((double)ty + 0.5) * a.cellc;
            cp[2] = (double)k * a.head_step;
        } else {
            cd[0] = cd[1] = cd[2] = -1;
            cd[3] = 0;
            const double qnan = __longlong_as_double(0x7ff8000000000000ll);
            cp[0] = cp[1] = cp[2] = qnan;
        }
    }
}

// (relocprior_select_kernel, lslam_relocprior.h, is a copy of this kernel behind its own eligibility test: a fix
// to the winner, the rivals or the ambiguity test is a fix there too.)
__global__ __launch_bounds__(64) void reloc_select_kernel(const RelocArgs a) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x), R = a.b.n_robots, K = a.K;
    if (r >= R) return;
    const int bad = LSLAM_MAPMATCH_EMPTY | LSLAM_MAPMATCH_BAD_POSE | LSLAM_MAPMATCH_WEAK;
    int win = -1, sw = 0;
    for (int j = 0; j < K; j++) {
        if (a.b.fine_flags[(int64_t)j * R + r] & bad) continue;
        const int s = a.b.fine_best[((int64_t)j * R + r) * 4 + 3];
        if (win < 0 || s > sw) {
            win = j;
            sw = s;
        }
    }
    int32_t *res = a.b.result + 8 * (int64_t)r;
    if (win < 0) {
        res[0] = res[1] = res[2] = res[3] = -1;
        res[4] = res[5] = 0;
        res[6] = -1;
        res[7] = 0;
        a.b.flags[r] = LSLAM_RELOC_LOST;
        return;
    }
    const double *pw = a.b.fine_pose + ((int64_t)win * R + r) * 3;
    const double wx = pw[0], wy = pw[1], wt = pw[2];
    int riv = -1, sr = 0;
    for (int j = 0; j < K; j++) {
        if (j == win || (a.b.fine_flags[(int64_t)j * R + r] & bad)) continue;
        const double *pj = a.b.fine_pose + ((int64_t)j * R + r) * 3;
        double dt = fabs(wt - pj[2]);
        if (dt > 3.141592653589793) dt = 6.283185307179586 - dt;
        if (fabs(wx - pj[0]) <= a.dup_mm && fabs(wy - pj[1]) <= a.dup_mm && dt <= a.dup_rad) continue;
        const int s = a.b.fine_best[((int64_t)j * R + r) * 4 + 3];
        if (riv < 0 || s > sr) {
            riv = j;
            sr = s;
        }
    }
    const bool ambiguous = riv >= 0 && 1000ll * (long long)sr >= (long long)a.ambig * (long long)sw;
    const int32_t *cd = a.b.cand + ((int64_t)win * R + r) * 4;
    res[0] = win;
    res[1] = cd[0];
    res[2] = cd[1];
    res[3] = cd[2];
    res[4] = cd[3];
    res[5] = sw;
    res[6] = riv;
    res[7] = riv >= 0 ? sr : 0;
    a.b.flags[r] = ambiguous ? LSLAM_RELOC_AMBIGUOUS : 0;
    if (ambiguous) return;
    const unsigned long long *pin = (const unsigned long long *)pw;
    unsigned long long *pout = (unsigned long long *)a.b.pose_out + 3 * (int64_t)r;
    pout[0] = pin[0];
    pout[1] = pin[1];
    pout[2] = pin[2];
    if (a.b.P_out) {
        double *P = a.b.P_out + 9 * (int64_t)r;
        for (int i = 0; i < 9; i++) P[i] = 0.0;
        P[0] = a.pxy;
        P[4] = a.pxy;
        P[8] = a.pth;
    }
}

}  // namespace lslam
