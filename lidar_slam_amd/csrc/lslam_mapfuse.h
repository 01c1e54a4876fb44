// lslam_mapfuse.h — a scan-to-map match fused into the filter: the match of lslam_mapmatch.h as a
// measurement of the pose, with a covariance taken from the whole score volume, and a gated Kalman
// update of the filter's mean and covariance.  The definition (moments, match covariance,
// innovation, gate, Joseph-form update) is the comment on lslam_map_fuse in include/lidarslam.h;
// tests/mapfuse_ref.py is its NumPy form.
//
// The score volume is mapmatch_search_kernel's (launch_mapmatch_search).  The winner's key, its
// refinement and the match's flags are the functions mapmatch_pick_kernel calls: match_best,
// match_winner (lslam_corr.h) and mapmatch_flags (lslam_mapmatch.h).
//
// Kernel:
//   mapfuse_pick_kernel  one 256-thread workgroup per robot.  Pass 1 is match_best, which leaves
//                        the winner's key in every thread.  Pass 2 walks the
//                        volume again (72 KB at the defaults: L2) and sums the ten int64 moments in
//                        registers, over a wave by shuffles and over the four waves through LDS.
//                        Thread 0 then runs steps 3-4 of the match and steps 6-8 of the fusion, a few
//                        hundred FP64 operations in plain C++, every loop unrolled so that the 3x3
//                        matrices stay in registers.  -ffp-contract=off keeps every operation
//                        rounded on its own; the division and the int64 -> double conversion are
//                        single roundings (tests/test_gpu_mapfuse.py compares bit patterns).
//
// LDS: 4 keys and 4 x 10 partial sums, 352 B.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_mapmatch.h"

namespace lslam {

struct MapFuseArgs {
    MapMatchArgs m;
    const double *P;
    double *P_out, *z, *Rm, *nis;
    int64_t *moments;  // may be null
    double r_scale, nis_max;
    int cut_permille;
};

__device__ __forceinline__ long long mapfuse_shfl_xor(long long v, int o) {
    return (long long)shfl_xor_u64((unsigned long long)v, o);
}

__device__ __forceinline__ unsigned long long mapfuse_word(double v) { return (unsigned long long)__double_as_longlong(v); }

// C = A B, or A B^T with TB, row-major 3x3; every element is (t0 + t1) + t2
template <bool TB>
__device__ __forceinline__ void mapfuse_mul(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double b0 = TB ? B[3 * j] : B[j], b1 = TB ? B[3 * j + 1] : B[3 + j], b2 = TB ? B[3 * j + 2] : B[6 + j];
            C[3 * i + j] = (A[3 * i] * b0 + A[3 * i + 1] * b1) + A[3 * i + 2] * b2;
        }
}

// M v, each element (t0 + t1) + t2
__device__ __forceinline__ void mapfuse_mulv(const double (&M)[9], const double (&v)[3], double (&o)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}

// (A template only for its place in the code object: an instantiation is emitted where it is first
// launched, behind the pipeline's kernel templates, which so keep their distances from each other;
// as a plain kernel it was emitted in front of them.)
template <int kForm>
__global__ __launch_bounds__(MATCH_PICK_TPB) void mapfuse_pick_kernel(const MapFuseArgs f) {
    constexpr int NW = MATCH_PICK_TPB / 64;
    __shared__ unsigned long long wk[NW];
    __shared__ long long ws[NW][10];
    const MapMatchArgs &a = f.m;
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const CorrGeom &g = a.g;
    const int n = g.Nth * g.Nt * g.Nt;
    const int32_t *S = g.scores + (int64_t)r * n;

    // ---- pass 1: the winner's key ----
    MatchWinner win = match_decode(g, match_best(g, S, wk, tid));
    const int s0 = win.s0, ks = win.k, jys = win.jy, jxs = win.jx;

    // ---- pass 2 (step 5): the ten moments about the winner, int64 (each below 5e17) ----
    const long long cut = ((long long)s0 * (long long)f.cut_permille) / 1000ll;
    long long mo[10];
#pragma unroll
    for (int j = 0; j < 10; j++) mo[j] = 0ll;
    for (int i = tid; i < n; i += MATCH_PICK_TPB) {
        const long long w = (long long)S[i] - cut;
        if (w <= 0) continue;
        int k, jy, jx;
        match_unflat(g, i, k, jy, jx);
        const long long da = jx - jxs, db = jy - jys, dc = k - ks;
        const long long wa = w * da, wb = w * db, wc = w * dc;
        mo[0] += w;
        mo[1] += wa;
        mo[2] += wb;
        mo[3] += wc;
        mo[4] += wa * da;
        mo[5] += wa * db;
        mo[6] += wa * dc;
        mo[7] += wb * db;
        mo[8] += wb * dc;
        mo[9] += wc * dc;
    }
#pragma unroll
    for (int j = 0; j < 10; j++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mo[j] += mapfuse_shfl_xor(mo[j], o);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 10; j++) ws[tid >> 6][j] = mo[j];
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int j = 0; j < 10; j++) {
        long long t = ws[0][j];
#pragma unroll
        for (int w = 1; w < NW; w++) t += ws[w][j];
        mo[j] = t;
    }

    // this thread alone reads pose[r] and P[r] and, below, writes pose_out[r] and P_out[r]: each pair
    // may be one buffer
    const unsigned long long *pin = (const unsigned long long *)a.b.pose + 3 * r;
    const unsigned long long *Pin = (const unsigned long long *)f.P + 9 * r;
    unsigned long long xb[3], Pb[9];
    double x[3], P[9];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        xb[i] = pin[i];
        x[i] = mapmatch_bits(xb[i]);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Pb[i] = Pin[i];
        P[i] = mapmatch_bits(Pb[i]);
    }

    // ---- steps 3, 4 of lslam_map_match ----
    match_winner(g, S, win);
    const double (&y)[3] = win.d;
    int flags = mapmatch_flags(a, r, win, x[0], x[1], x[2]);

    unsigned long long zb[3] = {xb[0], xb[1], xb[2]}, xo[3] = {xb[0], xb[1], xb[2]}, Po[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Po[i] = Pb[i];
    double Rm[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double nis = 0.0;
    if (s0 == 0) {
#pragma unroll
        for (int j = 0; j < 10; j++) mo[j] = 0ll;
    } else {
        // ---- step 6: the match covariance ----
        const double Wd = (double)mo[0];
        const double mean[3] = {(double)mo[1] / Wd, (double)mo[2] / Wd, (double)mo[3] / Wd};
        const double sc[3] = {g.cell, g.cell, g.theta_step};
        const long long m2[6] = {mo[4], mo[5], mo[6], mo[7], mo[8], mo[9]};  // aa ab ac bb bc cc
        int q = 0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = i; j < 3; j++, q++) {
                const double c = (double)m2[q] / Wd - mean[i] * mean[j];
                double v = (c * sc[i]) * sc[j];
                if (i == j) v = v + (sc[i] * sc[i]) / 12.0;
                v = v * f.r_scale;
                Rm[3 * i + j] = v;
                Rm[3 * j + i] = v;
            }
#pragma unroll
        for (int i = 0; i < 3; i++) zb[i] = mapfuse_word(x[i] + y[i]);

        // ---- step 7: innovation covariance, its adjugate, the gate ----
        double Sm[9];
        bool finiteP = true;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            Sm[i] = P[i] + Rm[i];
            finiteP = finiteP && __builtin_isfinite(P[i]);
        }
        double A[9];
        A[0] = Sm[4] * Sm[8] - Sm[5] * Sm[7];
        A[1] = Sm[2] * Sm[7] - Sm[1] * Sm[8];
        A[2] = Sm[1] * Sm[5] - Sm[2] * Sm[4];
        A[3] = Sm[5] * Sm[6] - Sm[3] * Sm[8];
        A[4] = Sm[0] * Sm[8] - Sm[2] * Sm[6];
        A[5] = Sm[2] * Sm[3] - Sm[0] * Sm[5];
        A[6] = Sm[3] * Sm[7] - Sm[4] * Sm[6];
        A[7] = Sm[1] * Sm[6] - Sm[0] * Sm[7];
        A[8] = Sm[0] * Sm[4] - Sm[1] * Sm[3];
        const double det = (Sm[0] * A[0] + Sm[1] * A[3]) + Sm[2] * A[6];
        if (!finiteP || !(Sm[0] > 0.0 && A[8] > 0.0 && det > 0.0 && __builtin_isfinite(det))) {
            flags |= LSLAM_MAPFUSE_BAD_COV;
        } else {
            double Si[9], v[3];
#pragma unroll
            for (int i = 0; i < 9; i++) Si[i] = A[i] / det;
            mapfuse_mulv(Si, y, v);
            nis = (y[0] * v[0] + y[1] * v[1]) + y[2] * v[2];
            if (!(nis <= f.nis_max)) flags |= LSLAM_MAPFUSE_OUTLIER;

            // ---- step 8: the update, Joseph form ----
            if (!(flags & (LSLAM_MAPMATCH_WEAK | LSLAM_MAPFUSE_OUTLIER))) {
                double K[9], Ky[3], IK[9], AP[9], U[9], KR[9], V[9];
                mapfuse_mul<false>(P, Si, K);
                mapfuse_mulv(K, y, Ky);
#pragma unroll
                for (int i = 0; i < 3; i++) xo[i] = mapfuse_word(x[i] + Ky[i]);
#pragma unroll
                for (int i = 0; i < 9; i++) IK[i] = ((i & 3) == 0 ? 1.0 : 0.0) - K[i];
                mapfuse_mul<false>(IK, P, AP);
                mapfuse_mul<true>(AP, IK, U);
                mapfuse_mul<false>(K, Rm, KR);
                mapfuse_mul<true>(KR, K, V);
                double T[9];
#pragma unroll
                for (int i = 0; i < 9; i++) T[i] = U[i] + V[i];
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) Po[3 * i + j] = mapfuse_word(0.5 * (T[3 * i + j] + T[3 * j + i]));
            }
        }
    }

    // ---- outputs: after every read of this robot's pose and P ----
    match_store(win, a.b.delta, a.b.best, r);
    a.b.flags[r] = flags;
    unsigned long long *pout = (unsigned long long *)a.b.pose_out + 3 * r, *zout = (unsigned long long *)f.z + 3 * r;
    unsigned long long *Pout = (unsigned long long *)f.P_out + 9 * r;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        pout[i] = xo[i];
        zout[i] = zb[i];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Pout[i] = Po[i];
        f.Rm[9 * r + i] = Rm[i];
    }
    f.nis[r] = nis;
    if (f.moments) {
#pragma unroll
        for (int j = 0; j < 10; j++) f.moments[10 * r + j] = (int64_t)mo[j];
    }
}

}  // namespace lslam
