// lslam_fieldfuse_core.h — the 3 x 3 algebra of lslam_field_fuse (its definition is the comment in
// include/lidarslam.h): the alignment's ten sums and the filter's (x, P) -> the noise variance, the
// alignment's information and its floored form, the gated innovation statistic and the update in
// information form.  Plain C++, no HIP: the kernel of lslam_fieldfuse.h and a CPU program
// (tests/test_fieldfuse_core.py) compile this same text.
//
// Every double operation is written as one statement's worth of one rounding: the library is built
// with -ffp-contract=off, so that nothing is fused, and the order below is the definition's.  Every
// loop has constant bounds and is unrolled, so that in the kernel the matrices stay in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lslam_fieldalign_core.h"

// The matrices are passed by reference: a call that is not inlined would put them in memory (on the
// device: scratch), so every function here is inlined by force.
#define FIELDFUSE_FN LSLAM_GRID_HD static inline __attribute__((always_inline))

enum { FIELDFUSE_OUTLIER = 64, FIELDFUSE_BAD_COV = 128 };  // LSLAM_FIELDFUSE_* (lslam_fieldfuse.h asserts it)

// the host's part of steps 6 and 8, taken once per call
struct FieldFuseConsts {
    double inv;      // 1 / cell
    double smin2;    // sigma_min sigma_min
    double r_scale;
    double w[3];     // (1 / ft, 1 / ft, 1 / fr)
    double nis_max;
};

FIELDFUSE_FN FieldFuseConsts fieldfuse_consts(double cell, double sigma_min, double r_scale, double floor_t, double floor_r,
                                              double nis_max) {
    FieldFuseConsts k;
    k.inv = 1.0 / cell;
    k.smin2 = sigma_min * sigma_min;
    k.r_scale = r_scale;
    const double ft = (floor_t * cell) * (floor_t * cell), fr = floor_r * floor_r;
    k.w[0] = k.w[1] = 1.0 / ft;
    k.w[2] = 1.0 / fr;
    k.nis_max = nis_max;
    return k;
}

// C = A B, row-major 3 x 3; every element is (t0 + t1) + t2
FIELDFUSE_FN void fieldfuse_mul(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// M v, each element (t0 + t1) + t2
FIELDFUSE_FN void fieldfuse_mulv(const double (&M)[9], const double (&v)[3], double (&o)[3]) {
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}

// The adjugate/determinant inverse of lslam_map_fuse step 7 and its pass test.  Si is written whatever
// the test says (not finite where det is zero): the callers select, they do not branch, so that every
// matrix stays a set of registers.
FIELDFUSE_FN bool fieldfuse_inverse(const double (&S)[9], double (&Si)[9]) {
    double A[9];
    A[0] = S[4] * S[8] - S[5] * S[7];
    A[1] = S[2] * S[7] - S[1] * S[8];
    A[2] = S[1] * S[5] - S[2] * S[4];
    A[3] = S[5] * S[6] - S[3] * S[8];
    A[4] = S[0] * S[8] - S[2] * S[6];
    A[5] = S[2] * S[3] - S[0] * S[5];
    A[6] = S[3] * S[7] - S[4] * S[6];
    A[7] = S[1] * S[6] - S[0] * S[7];
    A[8] = S[0] * S[4] - S[1] * S[3];
    const double det = (S[0] * A[0] + S[1] * A[3]) + S[2] * A[6];
#pragma unroll
    for (int i = 0; i < 9; i++) Si[i] = A[i] / det;
    return S[0] > 0.0 && A[8] > 0.0 && fieldalign_pivot_ok(det);
}

FIELDFUSE_FN bool fieldfuse_finite(double v) { return v > -(double)INFINITY && v < (double)INFINITY; }

// 0.5 (M + M^T)
FIELDFUSE_FN void fieldfuse_sym(const double (&M)[9], double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) o[3 * i + j] = 0.5 * (M[3 * i + j] + M[3 * j + i]);
}

// Steps 6-11 for a robot whose alignment was accepted: N the ten sums, n_last the points of the last
// evaluation, (x, P) the filter's mean and covariance, z the aligned pose.  Writes s2, info, info_f
// (zeros if B has no inverse), nis (0.0 with BAD_COV) and the updated (xo, Po), which hold the update iff
// the returned flags are 0.  Returns 0, FIELDFUSE_BAD_COV or FIELDFUSE_OUTLIER.  Straight-line code: the
// tests of steps 8-10 are selects at the end.
FIELDFUSE_FN int fieldfuse_steps(const int64_t N[10], int n_last, const FieldFuseConsts &k, const double (&x)[3],
                                 const double (&P)[9], const double (&z)[3], double &s2, double (&info)[9],
                                 double (&info_f)[9], double &nis, double (&xo)[3], double (&Po)[9]) {
    const double sc = 1.0 / 1048576.0;
    // ---- 6. noise ----
    const double mean = n_last == 0 ? 0.0 : ((double)N[9] * sc) / (double)n_last;
    s2 = fmax(mean, k.smin2) * k.r_scale;
    // ---- 7. the alignment's information, mm and rad ----
    const double hxx = (double)N[0] * sc, hxy = (double)N[1] * sc, hxt = (double)N[2] * sc;
    const double hyy = (double)N[3] * sc, hyt = (double)N[4] * sc, htt = (double)N[5] * sc;
    info[0] = ((hxx * k.inv) * k.inv) / s2;
    info[1] = info[3] = ((hxy * k.inv) * k.inv) / s2;
    info[2] = info[6] = ((hxt * k.inv) * 1.0) / s2;
    info[4] = ((hyy * k.inv) * k.inv) / s2;
    info[5] = info[7] = ((hyt * k.inv) * 1.0) / s2;
    info[8] = ((htt * 1.0) * 1.0) / s2;
    // ---- 8. floor ----
    double B[9], Bi[9], T[9], E[9], Lf[9];
#pragma unroll
    for (int i = 0; i < 9; i++) B[i] = info[i];
    B[0] = info[0] + k.w[0];
    B[4] = info[4] + k.w[1];
    B[8] = info[8] + k.w[2];
    const bool okB = fieldfuse_inverse(B, Bi);
    fieldfuse_mul(info, Bi, T);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        E[3 * i] = T[3 * i] * k.w[0];
        E[3 * i + 1] = T[3 * i + 1] * k.w[1];
        E[3 * i + 2] = T[3 * i + 2] * k.w[2];
    }
    fieldfuse_sym(E, Lf);
#pragma unroll
    for (int i = 0; i < 9; i++) info_f[i] = okB ? Lf[i] : 0.0;
    // ---- 9. prior ----
    bool finiteP = true;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const bool fin = fieldfuse_finite(P[i]);
        finiteP = finiteP && fin;
    }
    double Pi[9], M[9], Mi[9];
    const bool okP = fieldfuse_inverse(P, Pi);
#pragma unroll
    for (int i = 0; i < 9; i++) M[i] = Pi[i] + info_f[i];
    const bool okM = fieldfuse_inverse(M, Mi);
    fieldfuse_sym(Mi, Po);
    const bool d0 = fieldalign_pivot_ok(Po[0]), d1 = fieldalign_pivot_ok(Po[4]), d2 = fieldalign_pivot_ok(Po[8]);
    const bool ok = okB && finiteP && okP && okM && d0 && d1 && d2;
    // ---- 10. innovation and gate ----
    const double y[3] = {z[0] - x[0], z[1] - x[1], z[2] - x[2]};
    double b[3], c[3], e[3];
    fieldfuse_mulv(info_f, y, b);
    fieldfuse_mulv(Po, b, c);
    fieldfuse_mulv(Pi, c, e);
    const double q = (y[0] * e[0] + y[1] * e[1]) + y[2] * e[2];
    nis = ok ? q : 0.0;
    // ---- 11. update ----
#pragma unroll
    for (int i = 0; i < 3; i++) xo[i] = x[i] + c[i];
    return !ok ? FIELDFUSE_BAD_COV : (!(q <= k.nis_max) ? FIELDFUSE_OUTLIER : 0);
}
