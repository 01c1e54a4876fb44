// lslam_relocprior.h — relocalisation over a set of admissible coarse candidates: the free-space prior
// from the clearance field and the search window around a stale pose.  The definition is the comment on
// lslam_map_relocalize_prior in include/lidarslam.h; tests/relocprior_ref.py is its NumPy form.  The
// peak, top-K and fine kernels are lslam_map_relocalize's own (lslam_reloc.h, lslam_mapmatch.h).
//
// Kernels (templates only for their place in the code object, as fieldfuse_kernel is: behind every other;
// the rule is at the include of lslam_launch_map.h in lslam_launch.h):
//   relocprior_admit_kernel   one 256-thread workgroup per robot, once per call: the admissible bits
//                             Af & Aw, one per coarse cell in the search's task order (row ty, span of 32
//                             tx: dword ty nspan + span), the ordered list of the admissible headings,
//                             n_admit.  8 KiB of static LDS (Wc <= 256: 2048 dwords) and a counter.
//   relocprior_search_kernel  reloc_search_kernel<0> over that set.  The workgroup of (robot, slice) takes
//                             the slice's share of the robot's ADMISSIBLE headings (a contiguous window
//                             leaves no slice empty while another holds the whole window), loads the
//                             robot's bits into LDS beside the bitmap and compacts the live tasks, those
//                             whose span holds a set bit, into an LDS list once; the list does not
//                             depend on the heading and keeps the tasks' order.  Its threads then walk
//                             the list in the place of all Wc nspan tasks, so the live spans fill the
//                             first waves and the others retire, and a live span's 32 sums are written
//                             under its bits.  Cells of dead spans and of skipped headings are not
//                             touched: the launcher clears the chunk's volume first (DESIGN 4.4 has the
//                             cost).  With neither prior the launcher runs reloc_search_kernel<0> itself.
//                             LDS: reloc_search_kernel's, plus 4 bytes (the bits) and 2 bytes (the
//                             list) per task: 12 KiB more at Wc = 256 (97,296 bytes), 3 KiB at 128.
//   relocprior_select_kernel  reloc_select_kernel with the gather of fine_clear2 and step 5's test.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_reloc.h"

namespace lslam {

constexpr int RELOCPRIOR_ADMIT_TPB = 256;
constexpr int RELOCPRIOR_MAX_TASKS = 256 * 8;  // Wc <= 256 rows of at most 8 spans

struct RelocPriorArgs {
    RelocArgs r;  // b = the embedded batch; n_slices: workgroups per robot, per_slice is not used
    const uint16_t *clear_d2;
    const double *win_pose;
    int32_t *n_admit, *fine_clear2;
    double half_xy, half_theta;
    double inv;      // 1.0 / cell: the fine cell of a refined pose
    int clear_min2;
    int vec_d;       // rows of clear_d2 lie on 16-byte boundaries
    uint32_t *bits;  // [n_robots][Wc * nspan] the admissible bits
    int32_t *heads;  // [n_robots][1 + n_head] the number of admissible headings, then the headings, ascending
};

static inline int relocprior_lds_bytes(int Wc, int RW, int nspan) {
    const int ntask = Wc * nspan;
    return reloc_lds_bytes(Wc, RW) + ntask * 4 + ((ntask * 2 + 3) & ~3);
}

template <int kForm>
__global__ __launch_bounds__(RELOCPRIOR_ADMIT_TPB) void relocprior_admit_kernel(const RelocPriorArgs pa) {
    __shared__ uint32_t M[RELOCPRIOR_MAX_TASKS];
    __shared__ int cnt;  // the admissible cells
    const RelocArgs &a = pa.r;
    const int tid = (int)threadIdx.x, r = (int)blockIdx.x;
    const int Wc = a.Wc, nspan = a.nspan, ntask = Wc * nspan, f = a.f, W = a.map_w;

    // ---- Af: a fine cell with enough clearance sets its coarse cell's bit ----
    if (pa.clear_d2) {
        for (int t = tid; t < ntask; t += RELOCPRIOR_ADMIT_TPB) M[t] = 0u;
        if (tid == 0) cnt = 0;
        __syncthreads();
        const uint16_t *D = pa.clear_d2 + (int64_t)r * W * W;
        const uint32_t cmin = (uint32_t)pa.clear_min2;
        if (pa.vec_d) {
            const int ng = W >> 3, per = 8 / f;  // 16-byte groups per row; coarse cells per group (f = 2, 4, 8)
            const uint32_t sub = (1u << f) - 1u;
            for (int idx = tid; idx < W * ng; idx += RELOCPRIOR_ADMIT_TPB) {
                const int y = idx / ng, g = idx - y * ng;
                const uint4 v = *(const uint4 *)(D + (int64_t)y * W + 8 * g);
                const uint32_t d[4] = {v.x, v.y, v.z, v.w};
                uint32_t m = 0u;  // bit j: cell j of the group
#pragma unroll
                for (int i = 0; i < 4; i++)
                    m |= ((d[i] & 0xffffu) >= cmin ? 1u : 0u) << (2 * i) | ((d[i] >> 16) >= cmin ? 2u : 0u) << (2 * i);
                if (!m) continue;
                const int row = (y / f) * nspan;
                for (int j = 0; j < per; j++)
                    if ((m >> (f * j)) & sub) {
                        const int tx = g * per + j;
                        atomicOr(&M[row + (tx >> 5)], 1u << (tx & 31));
                    }
            }
        } else {
            for (int idx = tid; idx < W * W; idx += RELOCPRIOR_ADMIT_TPB) {
                if ((uint32_t)D[idx] < cmin) continue;
                const int y = idx / W, tx = (idx - y * W) / f;
                atomicOr(&M[(y / f) * nspan + (tx >> 5)], 1u << (tx & 31));
            }
        }
    } else {
        for (int t = tid; t < ntask; t += RELOCPRIOR_ADMIT_TPB) {
            const int nx = min(32, Wc - 32 * (t % nspan));
            M[t] = nx == 32 ? 0xffffffffu : (1u << nx) - 1u;
        }
        if (tid == 0) cnt = 0;
    }
    __syncthreads();

    // ---- Aw, the bits and their count: a thread owns the dwords it reads ----
    {
        const double ox = a.b.origin[2 * r], oy = a.b.origin[2 * r + 1];
        const bool win = pa.win_pose != nullptr;
        const double wx = win ? pa.win_pose[3 * (int64_t)r] : 0.0, wy = win ? pa.win_pose[3 * (int64_t)r + 1] : 0.0;
        const double hxy = pa.half_xy;
        uint32_t *out = pa.bits + (int64_t)r * ntask;
        int n = 0;
        for (int t = tid; t < ntask; t += RELOCPRIOR_ADMIT_TPB) {
            uint32_t m = M[t];
            if (win && m) {
                const int ty = t / nspan, tx0 = 32 * (t - ty * nspan);
                const double cy = oy + ((double)ty + 0.5) * a.cellc;
                uint32_t w = 0u;
                if (fabs(cy - wy) <= hxy)
                    for (int j = 0; j < 32; j++) {
                        const double cx = ox + ((double)(tx0 + j) + 0.5) * a.cellc;
                        if (fabs(cx - wx) <= hxy) w |= 1u << j;
                    }
                m &= w;
            }
            out[t] = m;
            n += __popc(m);
        }
        if (n) atomicAdd(&cnt, n);
    }

    // ---- H: the first wave lists the admissible headings in order ----
    if (tid < 64) {
        const bool win = pa.win_pose != nullptr;
        const double wt = win ? pa.win_pose[3 * (int64_t)r + 2] : 0.0;
        int32_t *hl = pa.heads + (int64_t)r * (a.n_head + 1) + 1;
        int n = 0;
        for (int base = 0; base < a.n_head; base += 64) {  // (the same trips for every lane)
            const int k = base + tid;
            bool h = k < a.n_head;
            if (h && win) h = fabs(remainder((double)k * a.head_step - wt, 6.283185307179586)) <= pa.half_theta;
            const uint64_t bal = ballot(h);
            if (h) hl[n + (int)mbcnt(bal)] = k;
            n += __popcll(bal);
        }
        if (tid == 0) hl[-1] = pa.n_admit[2 * (int64_t)r + 1] = n;
    }
    __syncthreads();
    if (tid == 0) pa.n_admit[2 * (int64_t)r] = cnt;
}

template <int kForm>
__global__ __launch_bounds__(RELOC_TPB) void relocprior_search_kernel(const RelocPriorArgs pa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const RelocArgs &a = pa.r;
    const int Wc = a.Wc, RW = a.RW, mw = a.map_w, f = a.f;
    const int nspan = a.nspan, ntask = Wc * nspan;
    uint32_t *B = (uint32_t *)smem;
    const int nB = 3 * Wc * RW;  // dwords of the bitmap: Wc zero rows, the map's, Wc zero rows
    uint32_t *stage = B + ((nB + 3) & ~3);
    int *cnt = (int *)(stage + RELOC_TILE);  // [0]: staged points; [1], [2]: occupied coarse cells / used points
    uint32_t *M = (uint32_t *)(cnt + 4);     // the robot's admissible bits, a dword per task
    uint16_t *live = (uint16_t *)(M + ntask);  // the tasks with a set bit (a task is < 2048)
    const int tid = (int)threadIdx.x;
    const int rl = (int)blockIdx.x / a.n_slices, slice = (int)blockIdx.x - rl * a.n_slices;
    const int r = a.r0 + rl;
    // the slice's share of the admissible headings
    const int32_t *heads = pa.heads + (int64_t)r * (a.n_head + 1) + 1;
    const int nH = heads[-1];
    const int per = (nH + a.n_slices - 1) / a.n_slices;
    const int ibeg = slice * per, iend = min(nH, ibeg + per);
    if (slice != 0 && ibeg >= iend) return;  // (slice 0 writes n_occ and n_used whatever is admissible)
    const int p0 = a.b.pt_off[r], p1 = a.b.pt_off[r + 1];
    const double2 *xy = (const double2 *)a.b.xy;
    const double invc = a.invc, max_r2 = a.max_r2;

    for (int i = tid; i < nB; i += RELOC_TPB) B[i] = 0u;
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();

    // ---- the admissible bits and the live tasks, in task order: neighbouring lanes keep neighbouring
    //      spans, as in the plain search (a wave's stores fill whole lines of the volume between them) ----
    int nlive = 0;
    {
        const uint32_t *bits = pa.bits + (int64_t)r * ntask;
        int *wn = (int *)stage;  // a count per wave (the staged points are not in use yet)
        const int wave = tid >> 6;
        for (int t0 = 0; t0 < ntask; t0 += RELOC_TPB) {  // (the same trips for every thread)
            const int t = t0 + tid;
            const uint32_t m = t < ntask ? bits[t] : 0u;
            if (t < ntask) M[t] = m;
            const uint64_t bal = ballot(m != 0u);
            if ((tid & 63) == 0) wn[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < RELOC_TPB / 64; w++) {
                const int c = wn[w];
                before += w < wave ? c : 0;
                all += c;
            }
            if (m) live[nlive + before + (int)mbcnt(bal)] = (uint16_t)t;
            nlive += all;
            __syncthreads();  // wn is written again
        }
    }

    // ---- 0. the coarse map: a set fine cell sets its coarse cell's bit ----
    {
        const int16_t *L = a.b.logodds + (int64_t)r * mw * mw;
        const int occ_min = a.occ_min;
        if (a.vec) {
            const int ng = mw >> 3, per8 = 8 / f;  // 16-byte groups per row; coarse cells per group (f = 2, 4, 8)
            const uint32_t sub = (1u << (2 * f)) - 1u;
            for (int idx = tid; idx < mw * ng; idx += RELOC_TPB) {
                const int y = idx / ng, g = idx - y * ng;
                const uint32_t m = mapmatch_threshold8(*(const uint4 *)(L + (int64_t)y * mw + 8 * g), occ_min);
                if (!m) continue;
                const int cy = y / f + Wc;
                for (int j = 0; j < per8; j++)
                    if ((m >> (2 * f * j)) & sub) {
                        const int bit = g * per8 + j + Wc;
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
    if (nlive == 0) return;  // (every thread holds the same count)

    // ---- 2'. scores of the live spans at the admissible headings ----
    const double dW = (double)Wc;
    const uint32_t null_pk = 0u;  // row ty of the bitmap: one of the zero rows above the map's
    for (int ih = ibeg; ih < iend; ih++) {
        const int k = heads[ih];
        const double c = a.b.head_rot[2 * k], s = a.b.head_rot[2 * k + 1];
        int32_t *out = a.vol + ((int64_t)rl * a.n_head + k) * Wc * Wc;
        bool first = true;
        for (int t0 = p0; t0 < p1 || first; t0 += RELOC_TILE) {
            __syncthreads();  // the previous tile's readers are done
            if (tid == 0) cnt[0] = 0;
            __syncthreads();
            for (int p = t0 + tid; p < min(p1, t0 + RELOC_TILE); p += RELOC_TPB) {
                const double2 q = xy[p];
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
            for (int li = tid; li < nlive; li += RELOC_TPB) {
                const int task = (int)live[li];
                const int ty = task / nspan, tx0 = 32 * (task - ty * nspan);
                int acc[32];
#pragma unroll
                for (int j = 0; j < 32; j++) acc[j] = 0;
                reloc_count<0>(B + ty * RW + (tx0 >> 5), stage, n8, acc);
                int32_t *o = out + ty * Wc + tx0;
                const uint32_t m = M[task];  // (no bit at or beyond Wc - tx0)
#pragma unroll
                for (int j = 0; j < 32; j++)
                    if ((m >> j) & 1u) o[j] = first ? acc[j] : o[j] + acc[j];
            }
            first = false;
        }
    }
}

template <int kForm>
__global__ __launch_bounds__(64) void relocprior_select_kernel(const RelocPriorArgs pa) {
    const RelocArgs &a = pa.r;
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x), R = a.b.n_robots, K = a.K;
    if (r >= R) return;
    const int bad = LSLAM_MAPMATCH_EMPTY | LSLAM_MAPMATCH_BAD_POSE | LSLAM_MAPMATCH_WEAK;
    // ---- 5'. fine_clear2 and the eligible ranks (K <= 16: a bit each) ----
    uint32_t elig = 0u;
    {
        const bool have = pa.clear_d2 != nullptr;
        const int W = a.map_w;
        const uint16_t *D = pa.clear_d2 + (have ? (int64_t)r * W * W : 0);
        const double ox = a.b.origin[2 * r], oy = a.b.origin[2 * r + 1];
        for (int j = 0; j < K; j++) {
            int fc = 0;
            if (have) {
                fc = -1;
                const double *p = a.b.fine_pose + ((int64_t)j * R + r) * 3;
                double X0d, Y0d;
                if (mapmatch_robot_cell(p[0], p[1], p[2], ox, oy, pa.inv, X0d, Y0d)) {
                    const int X0 = (int)X0d, Y0 = (int)Y0d;
                    if ((unsigned)X0 < (unsigned)W && (unsigned)Y0 < (unsigned)W) fc = (int)D[(int64_t)Y0 * W + X0];
                }
            }
            pa.fine_clear2[(int64_t)j * R + r] = fc;
            if (!(a.b.fine_flags[(int64_t)j * R + r] & bad) && (!have || fc >= pa.clear_min2)) elig |= 1u << j;
        }
    }
    int win = -1, sw = 0;
    for (int j = 0; j < K; j++) {
        if (!((elig >> j) & 1u)) continue;
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
        if (j == win || !((elig >> j) & 1u)) continue;
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
