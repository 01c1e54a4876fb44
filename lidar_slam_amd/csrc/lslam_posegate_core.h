// lslam_posegate_core.h — the arithmetic of lslam_pose_graph_gate (its definition is the comment in
// include/lidarslam.h) beyond what lslam_posegraph_core.h already holds: a candidate's checks, its right-hand
// sides J^T, one step of either substitution on a block of right-hand sides, and the 3 x 3 tail (J X, the
// innovation covariance, the statistic, the verdict).  Plain C++, no HIP: the kernel of lslam_posegate.h and a
// CPU program (tests/test_posegate_core.py) compile this same text.
//
// Every double operation is written as one statement's worth of one rounding: the library is built with
// -ffp-contract=off, so that nothing is fused, and the order below is the definition's.
//
// The right-hand sides of the candidates solved together are one block X, row-major [n][W]: row r holds
// element r of every column, a candidate's three columns side by side at 3 * slot.  W is the block's width
// in doubles, 3 * (the slots of a block).  Every element is stepped on its own, so how many candidates share
// a block does not reach the bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lslam_fieldfuse_core.h"
#include "lslam_posegraph_core.h"

enum { POSEGATE_MAX_CAND = 64 };
// LSLAM_POSEGATE_* (lslam_posegate.h asserts it)
enum { POSEGATE_ACCEPTED = 1, POSEGATE_OUTLIER = 2, POSEGATE_BAD_EDGE = 4, POSEGATE_BAD_INFO = 8, POSEGATE_APPENDED = 16, POSEGATE_NO_ROOM = 32 };
// the graph's flags, LSLAM_POSEGRAPH_* (likewise)
enum { POSEGATE_G_EMPTY = 1, POSEGATE_G_BAD_GRAPH = 2, POSEGATE_G_SINGULAR = 8 };

// The kernel's LDS in doubles: the triangle, the undivided column, the poses, (cos, sin), the edges' chi, a
// block of `slots` candidates' right-hand sides, and the candidates' flags (two int32 a double).
LSLAM_GRID_HD static inline int posegate_lds_doubles(int N_cap, int E_cap, int C_cap, int slots) {
    const int n = posegraph_dim(N_cap);
    return posegraph_tri_size(n) + n + 3 * N_cap + 2 * N_cap + E_cap + 3 * slots * n + (C_cap + 1) / 2;
}

// step 3's test of a candidate on a graph of N nodes
LSLAM_GRID_HD static inline bool posegate_edge_ok(int i, int j, int N, const double *z, const double *om) {
    if (i == j || i < 0 || i >= N || j < 0 || j >= N) return false;
    return posegraph_finite3(z) && posegraph_finite3(om) && posegraph_finite3(om + 3);
}

// R = J^T into the (zeroed) block: rows 3 (i - 1).. hold A^T, rows 3 (j - 1).. hold B^T, the gauge's none
LSLAM_GRID_HD static inline void posegate_rhs(const double *A, const double *B, int i, int j, double *X, int W, int q0) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (i >= 1) X[(3 * (i - 1) + r) * W + q0 + k] = A[3 * k + r];
            if (j >= 1) X[(3 * (j - 1) + r) * W + q0 + k] = B[3 * k + r];
        }
}

// forward substitution on column q of the block, column b of H done, row a > b: y[a] -= l_ab y[b]
LSLAM_GRID_HD static inline void posegate_forward(const double *H, double *X, int W, int q, int a, int b) {
    const double t = H[posegraph_tri(a, b)] * X[b * W + q];
    X[a * W + q] = X[a * W + q] - t;
}
// z[a] = y[a] / d_a
LSLAM_GRID_HD static inline void posegate_divide(const double *H, double *X, int W, int q, int a) {
    X[a * W + q] = X[a * W + q] / H[posegraph_tri(a, a)];
}
// back substitution, row b done, row a < b: x[a] -= l_ba x[b]
LSLAM_GRID_HD static inline void posegate_backward(const double *H, double *X, int W, int q, int a, int b) {
    const double t = H[posegraph_tri(b, a)] * X[b * W + q];
    X[a * W + q] = X[a * W + q] - t;
}

// The tail of one candidate, straight-line: e, A, B of posegraph_edge, the solved block, Omega and nis_max ->
// Ms = sym(J X) as cov (xx, xy, xt, yy, yt, tt), the statistic, the verdict.  nis is 0.0 with BAD_INFO.
FIELDFUSE_FN int posegate_tail(const double (&e)[3], const double *A, const double *B, int i, int j, const double *X, int W,
                               int q0, const double *om, double nis_max, double &nis, double (&cov)[6]) {
    double M[9], Ms[9];
    // (the gauge's rows are not there: its products are left out, and its reads go to row 0)
    const int ri = i >= 1 ? 3 * (i - 1) : 0, rj = j >= 1 ? 3 * (j - 1) : 0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            double m = 0.0;
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const double t = A[3 * r + q] * X[(ri + q) * W + q0 + k];
                const double s = m + t;
                m = i >= 1 ? s : m;
            }
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const double t = B[3 * r + q] * X[(rj + q) * W + q0 + k];
                const double s = m + t;
                m = j >= 1 ? s : m;
            }
            M[3 * r + k] = m;
        }
    fieldfuse_sym(M, Ms);
    cov[0] = Ms[0], cov[1] = Ms[1], cov[2] = Ms[2], cov[3] = Ms[4], cov[4] = Ms[5], cov[5] = Ms[8];
    const double O[9] = {om[0], om[1], om[2], om[1], om[3], om[4], om[2], om[4], om[5]};
    double Sc[9], S[9], Si[9], w[3];
    const bool ok1 = fieldfuse_inverse(O, Sc);
#pragma unroll
    for (int q = 0; q < 9; q++) S[q] = Ms[q] + Sc[q];
    const bool ok2 = fieldfuse_inverse(S, Si);
    fieldfuse_mulv(Si, e, w);
    const double d2 = (e[0] * w[0] + e[1] * w[1]) + e[2] * w[2];
    const bool ok = ok1 && ok2;
    nis = ok ? d2 : 0.0;
    return !ok ? POSEGATE_BAD_INFO : (d2 <= nis_max ? POSEGATE_ACCEPTED : POSEGATE_OUTLIER);
}

// Step 4 for one graph, in one thread: the accepted candidates become edges while there is room.
LSLAM_GRID_HD static inline int posegate_append(int E, int E_cap, int C, const int32_t *cij, const double *cz, const double *com,
                                                int32_t *cflags, int32_t *eij, double *ez, double *eo) {
    for (int c = 0; c < C; c++) {
        if (cflags[c] != POSEGATE_ACCEPTED) continue;
        if (E < E_cap) {
            eij[2 * E] = cij[2 * c], eij[2 * E + 1] = cij[2 * c + 1];
            for (int q = 0; q < 3; q++) ez[3 * E + q] = cz[3 * c + q];
            for (int q = 0; q < 6; q++) eo[6 * E + q] = com[6 * c + q];
            E++;
            cflags[c] |= POSEGATE_APPENDED;
        } else {
            cflags[c] |= POSEGATE_NO_ROOM;
        }
    }
    return E;
}

// ---- the whole call for one graph in one thread (the CPU program's; the kernel spreads the same element
// steps over its threads between barriers).  Packed arrays of exactly the sizes named; slots: the
// candidates of a block.  Returns the graph's flags; the outputs must come zeroed. ----
struct PosegateWork {
    double *H;   // [tri(3 (N - 1))]
    double *u;   // [3 (N - 1)]
    double *X;   // [3 (N - 1)][3 slots]
    double *chi; // [E]
};

static inline int posegate_graph_serial(int N, int E, int C, int N_cap, int E_cap, int C_cap, int slots, const double *P,
                                        const double *cs, int32_t *eij, double *ez, double *eo, const int32_t *cij,
                                        const double *cz, const double *com, double damp_t, double damp_r, double nis_max,
                                        int append, const PosegateWork &wk, double *chi2, double *nis, double *err, double *cov,
                                        int32_t *cflags, int32_t *n_edges_out) {
    if (N < 0 || E < 0 || N > N_cap || E > E_cap || C < 0 || C > C_cap) return POSEGATE_G_BAD_GRAPH;
    if (N < 2 || E == 0) return POSEGATE_G_EMPTY;
    for (int v = 0; v < N; v++)
        if (!posegraph_finite3(P + 3 * v)) return POSEGATE_G_BAD_GRAPH;
    for (int e = 0; e < E; e++)
        if (!posegate_edge_ok(eij[2 * e], eij[2 * e + 1], N, ez + 3 * e, eo + 6 * e)) return POSEGATE_G_BAD_GRAPH;
    const int n = posegraph_dim(N), nb = N - 1, W = 3 * slots;
    double *H = wk.H, *u = wk.u, *X = wk.X;
    // ---- 1. the evaluation ----
    for (int e = 0; e < E; e++) {
        const int i = eij[2 * e], j = eij[2 * e + 1];
        PosegraphEdge t;
        posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], ez + 3 * e, eo + 6 * e, t);
        wk.chi[e] = t.chi;
    }
    double sum = 0.0;
    for (int e = 0; e < E; e++) sum = sum + wk.chi[e];
    *chi2 = sum;
    for (int blk = 0; blk < nb * (nb + 1) / 2; blk++) {
        int rn, cn;
        posegraph_col_element(-1, blk, rn, cn);
        const int vr = rn + 1, vc = cn + 1;
        if (rn == cn) {
            double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gg[3] = {0.0, 0.0, 0.0};
            for (int e = 0; e < E; e++) {
                const int i = eij[2 * e], j = eij[2 * e + 1];
                if (i != vr && j != vr) continue;
                PosegraphEdge t;
                posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], ez + 3 * e, eo + 6 * e, t);
                posegraph_add_diag(t, i == vr, h, gg);
            }
            h[0] = h[0] + damp_t, h[2] = h[2] + damp_t, h[5] = h[5] + damp_r;
            int q = 0;
            for (int r = 0; r < 3; r++)
                for (int k = 0; k <= r; k++) H[posegraph_tri(3 * rn + r, 3 * rn + k)] = h[q++];
        } else {
            double h[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int e = 0; e < E; e++) {
                const int i = eij[2 * e], j = eij[2 * e + 1];
                if (!((i == vr && j == vc) || (i == vc && j == vr))) continue;
                PosegraphEdge t;
                posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], ez + 3 * e, eo + 6 * e, t);
                posegraph_add_off(t, i == vr, h);
            }
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) H[posegraph_tri(3 * rn + r, 3 * cn + k)] = h[3 * r + k];
        }
    }
    // ---- 2. the factor ----
    for (int p = 0; p < n; p++) {
        const double d = H[posegraph_tri(p, p)];
        if (!fieldalign_pivot_ok(d)) return POSEGATE_G_SINGULAR;
        for (int a = p + 1; a < n; a++) posegraph_col_scale(H, u, p, a, d);
        const int m = n - 1 - p;
        for (int t = 0; t < m * (m + 1) / 2; t++) {
            int a, b;
            posegraph_col_element(p, t, a, b);
            posegraph_col_update(H, u, p, a, b);
        }
    }
    // ---- 3. the candidates, a block at a time ----
    for (int c0 = 0; c0 < C; c0 += slots) {
        const int kb = C - c0 < slots ? C - c0 : slots;
        for (int q = 0; q < n * W; q++) X[q] = 0.0;
        for (int s = 0; s < kb; s++) {
            const int c = c0 + s, i = cij[2 * c], j = cij[2 * c + 1];
            if (!posegate_edge_ok(i, j, N, cz + 3 * c, com + 6 * c)) continue;
            PosegraphEdge t;
            posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], cz + 3 * c, com + 6 * c, t);
            posegate_rhs(t.A, t.B, i, j, X, W, 3 * s);
        }
        for (int b = 0; b < n - 1; b++)
            for (int a = b + 1; a < n; a++)
                for (int q = 0; q < 3 * kb; q++) posegate_forward(H, X, W, q, a, b);
        for (int a = 0; a < n; a++)
            for (int q = 0; q < 3 * kb; q++) posegate_divide(H, X, W, q, a);
        for (int b = n - 1; b > 0; b--)
            for (int a = 0; a < b; a++)
                for (int q = 0; q < 3 * kb; q++) posegate_backward(H, X, W, q, a, b);
        for (int s = 0; s < kb; s++) {
            const int c = c0 + s, i = cij[2 * c], j = cij[2 * c + 1];
            if (!posegate_edge_ok(i, j, N, cz + 3 * c, com + 6 * c)) {
                cflags[c] = POSEGATE_BAD_EDGE;
                continue;
            }
            PosegraphEdge t;
            posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], cz + 3 * c, com + 6 * c, t);
            double v[6];
            cflags[c] = posegate_tail(t.e, t.A, t.B, i, j, X, W, 3 * s, com + 6 * c, nis_max, nis[c], v);
            for (int q = 0; q < 3; q++) err[3 * c + q] = t.e[q];
            for (int q = 0; q < 6; q++) cov[6 * c + q] = v[q];
        }
    }
    // ---- 4. the append ----
    if (append) *n_edges_out = posegate_append(E, E_cap, C, cij, cz, com, cflags, eij, ez, eo);
    return 0;
}
