// lslam_posegraph_core.h — the arithmetic of lslam_pose_graph (its definition is the comment in
// include/lidarslam.h): an edge and its two poses -> the error, the Jacobians and the products with the
// information matrix; the blocks that an edge adds to H and g; the packed lower triangle; one column
// step of its LDL^T and one step of either substitution.  Plain C++, no HIP: the kernel of
// lslam_posegraph.h and a CPU program (tests/test_posegraph_core.py) compile this same text.
//
// Every double operation is written as one statement's worth of one rounding: the library is built
// with -ffp-contract=off, so that nothing is fused, and the order below is the definition's.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lslam_fieldalign_core.h"

enum { POSEGRAPH_MAX_NODES = 64, POSEGRAPH_MAX_EDGES = 1024, POSEGRAPH_MAX_ITER = 32 };

// the reduced system of N nodes (node 0 is the gauge) and its packed lower triangle, row after row
LSLAM_GRID_HD static inline int posegraph_dim(int N) { return 3 * (N - 1); }
LSLAM_GRID_HD static inline int posegraph_tri(int a, int b) { return a * (a + 1) / 2 + b; }  // b <= a
LSLAM_GRID_HD static inline int posegraph_tri_size(int n) { return n * (n + 1) / 2; }

// The kernel's LDS in doubles, from max_nodes and max_edges: the triangle, g, the undivided column, the
// poses, the stepped poses, (cos, sin) and the edges' chi.
LSLAM_GRID_HD static inline int posegraph_lds_doubles(int N_cap, int E_cap) {
    const int n = posegraph_dim(N_cap);
    return posegraph_tri_size(n) + 2 * n + 3 * N_cap + 3 * N_cap + 2 * N_cap + E_cap;
}

// a 3-term product: all three products formed, (t0 + t1) + t2
LSLAM_GRID_HD static inline double posegraph_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
    const double t0 = a0 * b0, t1 = a1 * b1, t2 = a2 * b2;
    return (t0 + t1) + t2;
}

LSLAM_GRID_HD static inline bool posegraph_finite3(const double *v) {
    return __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]);
}

// One edge at one evaluation: e, the Jacobians A = de/dx_i and B = de/dx_j (row-major 3 x 3),
// MA = Omega A, MB = Omega B, w = Omega e and chi = e^T w.
struct PosegraphEdge {
    double A[9], B[9], MA[9], MB[9], w[3], e[3], chi;
};

// pi, pj: the poses (x, y, theta) of nodes i and j; (c, s): the traced cos and sin of theta_i;
// z: the edge's measurement; om: Omega as xx, xy, xt, yy, yt, tt.
LSLAM_GRID_HD static inline void posegraph_edge(const double *pi, const double *pj, double c, double s, const double *z,
                                                const double *om, PosegraphEdge &t) {
    const double dx = pj[0] - pi[0], dy = pj[1] - pi[1];
    const double ux = c * dx + s * dy, uy = c * dy - s * dx;
    t.e[0] = ux - z[0];
    t.e[1] = uy - z[1];
    t.e[2] = remainder((pj[2] - pi[2]) - z[2], 6.283185307179586);
    t.A[0] = -c, t.A[1] = -s, t.A[2] = uy;
    t.A[3] = s, t.A[4] = -c, t.A[5] = -ux;
    t.A[6] = 0.0, t.A[7] = 0.0, t.A[8] = -1.0;
    t.B[0] = c, t.B[1] = s, t.B[2] = 0.0;
    t.B[3] = -s, t.B[4] = c, t.B[5] = 0.0;
    t.B[6] = 0.0, t.B[7] = 0.0, t.B[8] = 1.0;
    const double O[9] = {om[0], om[1], om[2], om[1], om[3], om[4], om[2], om[4], om[5]};
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            t.MA[3 * r + k] = posegraph_dot3(O[3 * r], t.A[k], O[3 * r + 1], t.A[3 + k], O[3 * r + 2], t.A[6 + k]);
            t.MB[3 * r + k] = posegraph_dot3(O[3 * r], t.B[k], O[3 * r + 1], t.B[3 + k], O[3 * r + 2], t.B[6 + k]);
        }
        t.w[r] = posegraph_dot3(O[3 * r], t.e[0], O[3 * r + 1], t.e[1], O[3 * r + 2], t.e[2]);
    }
    t.chi = posegraph_dot3(t.e[0], t.w[0], t.e[1], t.w[1], t.e[2], t.w[2]);
}

// element (r, k) of J^T M and element r of J^T w, J and M row-major 3 x 3
LSLAM_GRID_HD static inline double posegraph_block(const double *J, const double *M, int r, int k) {
    return posegraph_dot3(J[r], M[k], J[3 + r], M[3 + k], J[6 + r], M[6 + k]);
}
LSLAM_GRID_HD static inline double posegraph_gvec(const double *J, const double *w, int r) {
    return posegraph_dot3(J[r], w[0], J[3 + r], w[1], J[6 + r], w[2]);
}

// What an edge adds to the diagonal block of node v (v is the edge's i: A^T MA and A^T w; its j: B^T MB
// and B^T w): h[6] += the lower triangle (00, 10, 11, 20, 21, 22), g[3] += the vector.
LSLAM_GRID_HD static inline void posegraph_add_diag(const PosegraphEdge &t, bool is_i, double *h, double *g) {
    double J[9], M[9];
#pragma unroll
    for (int q = 0; q < 9; q++) {
        J[q] = is_i ? t.A[q] : t.B[q];
        M[q] = is_i ? t.MA[q] : t.MB[q];
    }
    int q = 0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int k = 0; k <= r; k++) h[q++] += posegraph_block(J, M, r, k);
        g[r] += posegraph_gvec(J, t.w, r);
    }
}

// What an edge adds to the block (row node, column node) below the diagonal: the edge's (i, j) block
// A^T MB where the row node is its i, the transpose of it where the row node is its j.  h[9] row-major.
LSLAM_GRID_HD static inline void posegraph_add_off(const PosegraphEdge &t, bool row_is_i, double *h) {
    double v[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) v[3 * r + k] = posegraph_block(t.A, t.MB, r, k);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) h[3 * r + k] += row_is_i ? v[3 * r + k] : v[3 * k + r];
}

// ---- the LDL^T of the packed lower triangle, right-looking; u: the undivided column (n doubles) ----

// column p, first half, row a > p: u[a] = H[a][p], H[a][p] = u[a] / d
LSLAM_GRID_HD static inline void posegraph_col_scale(double *H, double *u, int p, int a, double d) {
    const double v = H[posegraph_tri(a, p)];
    u[a] = v;
    H[posegraph_tri(a, p)] = v / d;
}
// column p, second half, p < b <= a: H[a][b] -= l_ap * (the undivided H[b][p])
LSLAM_GRID_HD static inline void posegraph_col_update(double *H, const double *u, int p, int a, int b) {
    const double t = H[posegraph_tri(a, p)] * u[b];
    H[posegraph_tri(a, b)] = H[posegraph_tri(a, b)] - t;
}
// the t-th element (a, b) of the rows below p, row after row: t in 0 .. m (m + 1) / 2, m = n - 1 - p
LSLAM_GRID_HD static inline void posegraph_col_element(int p, int t, int &a, int &b) {
    int r = (int)((sqrtf((float)(8 * t + 1)) - 1.0f) * 0.5f);
    while (r * (r + 1) / 2 > t) r--;
    while ((r + 1) * (r + 2) / 2 <= t) r++;
    a = p + 1 + r;
    b = p + 1 + (t - r * (r + 1) / 2);
}
// forward substitution, column b done, row a > b: y[a] -= l_ab y[b]
LSLAM_GRID_HD static inline void posegraph_forward(const double *H, double *y, int a, int b) {
    const double t = H[posegraph_tri(a, b)] * y[b];
    y[a] = y[a] - t;
}
// back substitution, row b done, row a < b: x[a] -= l_ba x[b]
LSLAM_GRID_HD static inline void posegraph_backward(const double *H, double *x, int a, int b) {
    const double t = H[posegraph_tri(b, a)] * x[b];
    x[a] = x[a] - t;
}

// The whole solve in one thread (the CPU program's; the kernel spreads the same element steps over its
// threads between barriers): H the damped packed triangle, g the vector, both overwritten; g becomes x
// (delta = -x).  false: a pivot is not finite and > 0 (the first one ends the solve).
static inline bool posegraph_solve_serial(double *H, double *g, double *u, int n) {
    for (int p = 0; p < n; p++) {
        const double d = H[posegraph_tri(p, p)];
        if (!fieldalign_pivot_ok(d)) return false;
        for (int a = p + 1; a < n; a++) posegraph_col_scale(H, u, p, a, d);
        const int m = n - 1 - p;
        for (int t = 0; t < m * (m + 1) / 2; t++) {
            int a, b;
            posegraph_col_element(p, t, a, b);
            posegraph_col_update(H, u, p, a, b);
        }
    }
    for (int b = 0; b < n; b++)
        for (int a = b + 1; a < n; a++) posegraph_forward(H, g, a, b);
    for (int a = 0; a < n; a++) g[a] = g[a] / H[posegraph_tri(a, a)];
    for (int b = n - 1; b > 0; b--)
        for (int a = 0; a < b; a++) posegraph_backward(H, g, a, b);
    return true;
}
