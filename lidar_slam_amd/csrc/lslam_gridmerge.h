// lslam_gridmerge.h — the map merge: one grid resampled into another's frame under a rigid transform,
// compared where the two overlap, and added.  The definition is the comment on lslam_grid_merge in
// include/lidarslam.h; tests/gridmerge_ref.py is its NumPy form; the tiles, the source cell of a
// destination cell, the classes and the merged value are lslam_gridmerge_plan.h, plain C++ that a CPU
// program runs under the sanitizers.
//
// gridmerge_kernel<CELLS, APPLY>: 256 threads; a workgroup is (pair, slice of the pair's tiles), by
// slices_for, so a large fleet is one workgroup a pair and a pair alone still fills the chip.  A pair
// that is SKIPPED or has a BAD_XFORM ends after the few scalar loads that say so: a fleet of them costs
// the two launches.
//   APPLY = false, the statistics: every destination cell gathers its source value and is counted; the
//     seven counters stay in registers over all the workgroup's tiles, are summed over the wave, and
//     lane 0 adds what is not zero to stats[m] (cleared by the launcher), one atomic a wave and counter.
//   APPLY = true, the merge, behind it on the stream: every workgroup takes the pair's decision from the
//     finished counters (and the pair's first writes flags[m]), ends if the pair is gated or the call a
//     dry run, else gathers again, stores the cells that change and counts them into stats[m][7].
// The work unit is a tile of 64 columns and 32 rows (lslam_gridmerge_plan.h).  CELLS = 8: a thread takes
// 8 consecutive cells of a row, one 16-byte load of the destination (and one store, if a cell of them
// changed): grid_w a multiple of 8 and dst 16-byte aligned.  CELLS = 1: a lane per cell.  Either way the
// source is read cell by cell, from memory, along the slanted line that the transform makes of a row:
// the direct gather.  A thread's 8 gathers are independent loads in flight together.
//
// N, the 3 x 3 block of the destination, is read from memory too, and only by a cell whose source value
// is occupied: in a map a cell in a hundred.  A tile with a one-cell halo staged in LDS would serve the
// other ninety-nine for nothing and cost a barrier a tile; the nine reads hit the lines that the
// thread's own row and its neighbours' rows have just loaded.  No LDS, no scratch but stats.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_gridmerge_plan.h"
#include "lslam_wave.h"

namespace lslam {

constexpr int MERGE_TPB = 256;

// 136 bytes
struct MergeArgs {
    lslam_gridmerge_batch b;
    double cell, inv;
    int grid_w, src_w, n_src, occ_min, l_min, l_max;
    int fill, dry_run, min_support, max_permille;
    int n_slices;  // workgroups per pair
    int per;       // tiles per workgroup
};

// Steps 0 and 1 for pair m: 0 and the pair's transform and source grid, or the flag that ends it.
__device__ __forceinline__ int merge_pair(const MergeArgs &a, int m, MergeXform &t, const int16_t *&S) {
    const int k = a.b.src_index ? a.b.src_index[m] : m;
    if (k < 0 || k >= a.n_src) return LSLAM_MERGE_SKIPPED;
    const double *x = a.b.xform + 4 * (int64_t)m, *od = a.b.dst_origin + 2 * (int64_t)m, *os = a.b.src_origin + 2 * (int64_t)k;
    t.c = x[0], t.s = x[1], t.tx = x[2], t.ty = x[3];
    t.oxd = od[0], t.oyd = od[1];
    t.oxs = os[0], t.oys = os[1];
    t.cell = a.cell, t.inv = a.inv;
    t.src_w = a.src_w;
    if (!merge_xform_finite(t)) return LSLAM_MERGE_BAD_XFORM;
    S = a.b.src + (int64_t)k * a.src_w * a.src_w;
    return 0;
}

__device__ __forceinline__ int merge_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int CELLS, bool APPLY>
__global__ __launch_bounds__(MERGE_TPB) void gridmerge_kernel(const MergeArgs a) {
    constexpr int NCNT = APPLY ? 1 : 7;
    constexpr int UPR = MERGE_TW / CELLS;  // units (cells or groups of 8) in a tile's row
    const int tid = (int)threadIdx.x;
    const int m = (int)(blockIdx.x / (unsigned)a.n_slices), slice = (int)(blockIdx.x % (unsigned)a.n_slices);
    int32_t *st = a.b.stats + 8 * (int64_t)m;

    MergeXform t;
    const int16_t *S = nullptr;
    int flag = merge_pair(a, m, t, S);
    if constexpr (APPLY) {
        bool go = false;
        if (!flag) {
            flag = merge_gates(st[MERGE_SUPP], st[MERGE_CONTRA], a.min_support, a.max_permille);
            go = !flag && !a.dry_run;
            if (go) flag = LSLAM_MERGE_MERGED;
        }
        if (slice == 0 && tid == 0) a.b.flags[m] = flag;
        if (!go) return;  // (uniform)
    } else {
        if (flag) return;  // (uniform)
    }

    const int W = a.grid_w, nt = merge_tiles(W);
    int16_t *L = a.b.dst + (int64_t)m * W * W;
    const int t0 = slice * a.per, t1 = t0 + a.per < nt ? t0 + a.per : nt;
    int cnt[NCNT];
#pragma unroll
    for (int k = 0; k < NCNT; k++) cnt[k] = 0;

    for (int ti = t0; ti < t1; ti++) {
        const MergeTile q = merge_tile(W, ti);
        const int n = (q.y1 - q.y0) * UPR;
        for (int u = tid; u < n; u += MERGE_TPB) {
            const int row = u / UPR, X0 = q.x0 + (u - row * UPR) * CELLS, Y = q.y0 + row;
            if (X0 >= q.x1) continue;  // (CELLS = 8: grid_w is a multiple of 8, a group is on the map whole)
            const double wy = merge_world(t.oyd, Y, t.cell);
            int16_t *Lp = L + (int64_t)Y * W + X0;
            int l[CELLS], sc[CELLS], v[CELLS];
            if constexpr (CELLS == 8) {
                const uint4 g = *(const uint4 *)Lp;
                const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int j = 0; j < 8; j++) l[j] = (int)(int16_t)(w[j >> 1] >> ((j & 1) * 16));
            } else {
                l[0] = (int)Lp[0];
            }
#pragma unroll
            for (int j = 0; j < CELLS; j++) sc[j] = merge_src_cell(t, merge_world(t.oxd, X0 + j, t.cell), wy);
#pragma unroll
            for (int j = 0; j < CELLS; j++) v[j] = sc[j] >= 0 ? (int)S[sc[j]] : 0;
            if constexpr (!APPLY) {
                uint32_t occ = 0, neg = 0;  // bit j: the source value is occupied; the destination holds the cell free
#pragma unroll
                for (int j = 0; j < CELLS; j++) {
                    cnt[MERGE_ON] += sc[j] >= 0 ? 1 : 0;
                    cnt[MERGE_NZ] += v[j] != 0 ? 1 : 0;
                    occ |= (v[j] >= a.occ_min ? 1u : 0u) << j;
                    neg |= (l[j] < 0 ? 1u : 0u) << j;
                    const bool both = v[j] != 0 && l[j] != 0;
                    cnt[MERGE_SAME] += both && (v[j] < 0) == (l[j] < 0) ? 1 : 0;
                    cnt[MERGE_OPP] += both && (v[j] < 0) != (l[j] < 0) ? 1 : 0;
                }
                // the occupied ones, a cell in a hundred of a map: one loop, not 8 branches
                while (occ) {
                    const int j = __ffs(occ) - 1;
                    occ &= occ - 1;
                    if (merge_near_occupied(L, W, X0 + j, Y, a.occ_min)) cnt[MERGE_SUPP]++;
                    else if ((neg >> j) & 1u) cnt[MERGE_CONTRA]++;
                    else cnt[MERGE_NEW]++;
                }
            } else {
                int changed = 0;
#pragma unroll
                for (int j = 0; j < CELLS; j++) {
                    const int nv = merge_value(l[j], v[j], a.fill, a.l_min, a.l_max);
                    changed += nv != l[j] ? 1 : 0;
                    l[j] = nv;
                }
                if (changed) {
                    cnt[0] += changed;
                    if constexpr (CELLS == 8) {
                        uint32_t w[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) w[j] = (uint32_t)(uint16_t)l[2 * j] | ((uint32_t)(uint16_t)l[2 * j + 1] << 16);
                        *(uint4 *)Lp = make_uint4(w[0], w[1], w[2], w[3]);
                    } else {
                        Lp[0] = (int16_t)l[0];
                    }
                }
            }
        }
    }

    // one atomic a wave and counter (every wave of the workgroup comes here: no barrier is needed)
#pragma unroll
    for (int k = 0; k < NCNT; k++) {
        const int s = merge_wave_sum(cnt[k]);
        if ((tid & 63) == 0 && s) atomicAdd(&st[APPLY ? MERGE_CHANGED : k], s);
    }
}

}  // namespace lslam
