// lslam_posegate.h — chi-square gating of closure candidates against a pose graph, before any solve.  The
// definition is the comment on lslam_pose_graph_gate in include/lidarslam.h; tests/posegate_ref.py is its NumPy
// form; the candidate's checks, the right-hand sides, the element steps of the substitutions on a block of them
// and the 3 x 3 tail are lslam_posegate_core.h, the evaluation and the LDL^T lslam_posegraph_core.h (plain C++,
// also compiled on the CPU).
//
// posegate_kernel: one 256-thread workgroup per graph, the structure of posegraph_kernel with its iteration
// taken out: the checks, one evaluation, one LDL^T, all in dynamic LDS (posegate_lds_doubles: H as a packed
// lower triangle, the undivided column, the poses, (cos, sin), chi per edge).  Behind the factor stand the
// candidates, a block of `slots` at a time: their right-hand sides J^T are a row-major block X [n][3 slots] in
// LDS, which one thread per candidate fills, and a thread owns an element (row, column) of it in every
// substitution step, a barrier per column of H as in posegraph_kernel; adjacent lanes take adjacent columns of
// one row, so the reads of H are broadcasts and those of X lie side by side.  A candidate's 3 x 3 tail is one
// thread's straight-line code.  Each element's operations are its own, so the bits do not depend on `slots`,
// which the host takes from what the LDS leaves: at most 8, one at (64 nodes, 1024 edges).  The candidates'
// flags are gathered in LDS; with append, thread 0 walks them behind a barrier and copies the accepted ones
// to the edge arrays, then every flag is stored.
//
// The only atomics are ORs of flag bits into an LDS word (order-free).  All loops are bounded by max_nodes,
// max_edges and max_cand; every barrier is reached by the whole workgroup (the branches around them are
// uniform: they depend on the graph's counts and on LDS words read behind a barrier).  A flagged graph leaves
// at once: its outputs are the host's memsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_posegate_core.h"
#include "lslam_posegraph.h"

namespace lslam {

constexpr int POSEGATE_TPB = 256;
constexpr int POSEGATE_SLOTS_MAX = 8;

static_assert(POSEGATE_ACCEPTED == LSLAM_POSEGATE_ACCEPTED && POSEGATE_OUTLIER == LSLAM_POSEGATE_OUTLIER &&
                  POSEGATE_BAD_EDGE == LSLAM_POSEGATE_BAD_EDGE && POSEGATE_BAD_INFO == LSLAM_POSEGATE_BAD_INFO &&
                  POSEGATE_APPENDED == LSLAM_POSEGATE_APPENDED && POSEGATE_NO_ROOM == LSLAM_POSEGATE_NO_ROOM,
              "lslam_posegate_core.h's candidate flags are lidarslam.h's");
static_assert(POSEGATE_G_EMPTY == LSLAM_POSEGRAPH_EMPTY && POSEGATE_G_BAD_GRAPH == LSLAM_POSEGRAPH_BAD_GRAPH &&
                  POSEGATE_G_SINGULAR == LSLAM_POSEGRAPH_SINGULAR,
              "lslam_posegate_core.h's graph flags are lidarslam.h's");

struct PoseGateArgs {
    lslam_posegate_batch b;
    lslam_posegate_params p;
    int32_t slots;  // the candidates of a block: posegate_slots
    int32_t reserved;
};

// the dynamic LDS in bytes: posegate_lds_doubles (the candidates' flags last) and a double for the two flag words
static inline int posegate_lds_bytes(int N_cap, int E_cap, int C_cap, int slots) {
    return 8 * (posegate_lds_doubles(N_cap, E_cap, C_cap, slots) + 1);
}
// the candidates solved together: as many as fit POSEGRAPH_LDS_MAX, POSEGATE_SLOTS_MAX and C_cap at most, one at least
static inline int posegate_slots(int N_cap, int E_cap, int C_cap) {
    int s = C_cap < POSEGATE_SLOTS_MAX ? C_cap : POSEGATE_SLOTS_MAX;
    while (s > 1 && posegate_lds_bytes(N_cap, E_cap, C_cap, s) > POSEGRAPH_LDS_MAX) s--;
    return s;
}

// the dynamic LDS of a workgroup (posegate_lds_doubles' parts, in its order)
struct PoseGateLds {
    double *H;    // [tri(3 (N_cap - 1))]
    double *u;    // [3 (N_cap - 1)] the undivided column
    double *P;    // [N_cap][3]
    double *cs;   // [N_cap][2]
    double *chi;  // [E_cap]
    double *X;    // [3 (N_cap - 1)][3 slots] the block of right-hand sides
    int *words;   // two flag words
    int *cf;      // [C_cap] the candidates' flags
};
__device__ static inline PoseGateLds posegate_lds(unsigned char *smem, int Nc, int Ec, int slots) {
    const int ncap = posegraph_dim(Nc);
    PoseGateLds l;
    l.H = (double *)smem;
    l.u = l.H + posegraph_tri_size(ncap);
    l.P = l.u + ncap;
    l.cs = l.P + 3 * Nc;
    l.chi = l.cs + 2 * Nc;
    l.X = l.chi + Ec;
    l.words = (int *)(l.X + 3 * slots * ncap);
    l.cf = l.words + 2;
    return l;
}

// FORM: 0 (a template, so that the kernel takes its place in the code object at launch_posegate)
template <int FORM>
__global__ __launch_bounds__(POSEGATE_TPB) void posegate_kernel(const PoseGateArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x, G = (int64_t)a.b.n_graphs;
    const int Nc = a.p.max_nodes, Ec = a.p.max_edges, Cc = a.p.max_cand, K = a.slots;
    const PoseGateLds L = posegate_lds(smem, Nc, Ec, K);
    double *const H = L.H, *const u = L.u, *const P = L.P, *const cs = L.cs, *const chi = L.chi, *const X = L.X;
    int *const words = L.words, *const cf = L.cf;
    int turn = 0;

    const long long *in = (const long long *)a.b.pose;
    int32_t *eij = a.b.edge_ij + g * Ec * 2;
    double *ez = a.b.edge_z + g * Ec * 3, *eo = a.b.edge_info + g * Ec * 6;
    const int32_t *cij = a.b.cand_ij + g * Cc * 2;
    const double *cz = a.b.cand_z + g * Cc * 3, *co = a.b.cand_info + g * Cc * 6;
    // As in posegraph_kernel: the kernel's arguments fill the scalar registers, so the pointers and the
    // constants are kept in vector registers, of which there are enough, and nothing spills.
    double damp_t = a.p.damp_t, damp_r = a.p.damp_r, nis_max = a.p.nis_max;
    double *trace = a.b.trace + g * Nc * 2, *chi2_out = a.b.chi2 + g;
    double *nis_out = a.b.cand_nis + g * Cc, *err_out = a.b.cand_err + g * Cc * 3, *cov_out = a.b.cand_cov + g * Cc * 6;
    int32_t *cf_out = a.b.cand_flags + g * Cc, *flags_out = a.b.flags + g, *ne_out = a.b.n_edges + g;
    int append = a.p.append;
    asm volatile("" : "+v"(eij), "+v"(ez), "+v"(eo), "+v"(in), "+v"(cij), "+v"(cz), "+v"(co));
    asm volatile("" : "+v"(damp_t), "+v"(damp_r), "+v"(nis_max), "+v"(trace), "+v"(chi2_out), "+v"(append));
    asm volatile("" : "+v"(nis_out), "+v"(err_out), "+v"(cov_out), "+v"(cf_out), "+v"(flags_out), "+v"(ne_out));

    // ---- 0. checks ----
    const int N = a.b.n_nodes[g], E = a.b.n_edges[g], C = a.b.n_cand[g];
    int flags = 0;
    if (N < 0 || E < 0 || N > Nc || E > Ec || C < 0 || C > Cc) {
        flags = LSLAM_POSEGRAPH_BAD_GRAPH;
    } else if (N < 2 || E == 0) {
        flags = LSLAM_POSEGRAPH_EMPTY;
    } else {
        bool bad = false;
        for (int i = tid; i < N; i += POSEGATE_TPB) {
#pragma unroll
            for (int c = 0; c < 3; c++) P[3 * i + c] = __longlong_as_double(in[((int64_t)i * G + g) * 3 + c]);
            bad |= !posegraph_finite3(P + 3 * i);
        }
        for (int e = tid; e < E; e += POSEGATE_TPB) bad |= !posegate_edge_ok(eij[2 * e], eij[2 * e + 1], N, ez + 3 * e, eo + 6 * e);
        if (posegraph_wg_or(words, turn, tid, bad ? 1 : 0)) flags = LSLAM_POSEGRAPH_BAD_GRAPH;  // (the barriers publish P)
    }
    if (flags) {  // (uniform; the other outputs are the memsets' zeros)
        if (tid == 0) *flags_out = flags;
        return;
    }
    const int n = posegraph_dim(N), nblk = (N - 1) * N / 2;

    // ---- 1. the evaluation: posegraph_kernel's, at k = 0 ----
    for (int i = tid; i < N; i += POSEGATE_TPB) {
        const double c = cos(P[3 * i + 2]), s = sin(P[3 * i + 2]);
        cs[2 * i] = c;
        cs[2 * i + 1] = s;
        trace[2 * i] = c;
        trace[2 * i + 1] = s;
    }
    __syncthreads();
    for (int e = tid; e < E; e += POSEGATE_TPB) {
        const int i = eij[2 * e], j = eij[2 * e + 1];
        PosegraphEdge t;
        posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], ez + 3 * e, eo + 6 * e, t);
        chi[e] = t.chi;
    }
    for (int blk = tid; blk < nblk; blk += POSEGATE_TPB) {
        int rn, cn;  // the block's reduced nodes, cn <= rn; their nodes are rn + 1 and cn + 1
        posegraph_col_element(-1, blk, rn, cn);
        const int vr = rn + 1, vc = cn + 1;
        if (rn == cn) {
            double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gg[3] = {0.0, 0.0, 0.0};  // (g is formed and not kept: nothing reads it)
            for (int e = 0; e < E; e++) {
                const int i = eij[2 * e], j = eij[2 * e + 1];
                if (i != vr && j != vr) continue;
                PosegraphEdge t;
                posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], ez + 3 * e, eo + 6 * e, t);
                posegraph_add_diag(t, i == vr, h, gg);
            }
            h[0] = h[0] + damp_t;
            h[2] = h[2] + damp_t;
            h[5] = h[5] + damp_r;
            const int r0 = 3 * rn;
            H[posegraph_tri(r0, r0)] = h[0];
            H[posegraph_tri(r0 + 1, r0)] = h[1];
            H[posegraph_tri(r0 + 1, r0 + 1)] = h[2];
            H[posegraph_tri(r0 + 2, r0)] = h[3];
            H[posegraph_tri(r0 + 2, r0 + 1)] = h[4];
            H[posegraph_tri(r0 + 2, r0 + 2)] = h[5];
        } else {
            double h[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int e = 0; e < E; e++) {
                const int i = eij[2 * e], j = eij[2 * e + 1];
                if (!((i == vr && j == vc) || (i == vc && j == vr))) continue;
                PosegraphEdge t;
                posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], ez + 3 * e, eo + 6 * e, t);
                posegraph_add_off(t, i == vr, h);
            }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) H[posegraph_tri(3 * rn + r, 3 * cn + c)] = h[3 * r + c];
        }
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int e = 0; e < E; e++) sum = sum + chi[e];
        *chi2_out = sum;
    }

    // ---- 2. the LDL^T: posegraph_kernel's ----
    bool singular = false;
    for (int p = 0; p < n; p++) {
        const double d = H[posegraph_tri(p, p)];
        if (!fieldalign_pivot_ok(d)) {  // (uniform: every thread reads the same word)
            singular = true;
            break;
        }
        for (int r = p + 1 + tid; r < n; r += POSEGATE_TPB) posegraph_col_scale(H, u, p, r, d);
        __syncthreads();
        const int m = n - 1 - p, cnt = m * (m + 1) / 2;
        for (int t = tid; t < cnt; t += POSEGATE_TPB) {
            int r, c;
            posegraph_col_element(p, t, r, c);
            posegraph_col_update(H, u, p, r, c);
        }
        __syncthreads();
    }
    if (singular) {
        if (tid == 0) *flags_out = LSLAM_POSEGRAPH_SINGULAR;  // (trace and chi2 stand; the candidates' outputs are the memsets' zeros)
        return;
    }

    // ---- 3. the candidates, a block of K at a time ----
    const int W = 3 * K;
    for (int c0 = 0; c0 < C; c0 += K) {
        const int kb = C - c0 < K ? C - c0 : K, wq = 3 * kb;
        for (int q = tid; q < n * W; q += POSEGATE_TPB) X[q] = 0.0;
        __syncthreads();
        if (tid < kb) {
            const int c = c0 + tid, i = cij[2 * c], j = cij[2 * c + 1];
            if (posegate_edge_ok(i, j, N, cz + 3 * c, co + 6 * c)) {
                PosegraphEdge t;
                posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], cz + 3 * c, co + 6 * c, t);
                posegate_rhs(t.A, t.B, i, j, X, W, 3 * tid);
            }
        }
        __syncthreads();
        for (int b = 0; b < n - 1; b++) {
            const int cnt = (n - 1 - b) * wq;
            for (int t = tid; t < cnt; t += POSEGATE_TPB) posegate_forward(H, X, W, t % wq, b + 1 + t / wq, b);
            __syncthreads();
        }
        for (int t = tid; t < n * wq; t += POSEGATE_TPB) posegate_divide(H, X, W, t % wq, t / wq);
        __syncthreads();
        for (int b = n - 1; b > 0; b--) {
            const int cnt = b * wq;
            for (int t = tid; t < cnt; t += POSEGATE_TPB) posegate_backward(H, X, W, t % wq, t / wq, b);
            __syncthreads();
        }
        if (tid < kb) {
            const int c = c0 + tid, i = cij[2 * c], j = cij[2 * c + 1];
            int verdict = LSLAM_POSEGATE_BAD_EDGE;
            if (posegate_edge_ok(i, j, N, cz + 3 * c, co + 6 * c)) {
                PosegraphEdge t;
                posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], cz + 3 * c, co + 6 * c, t);
                double nis, cov[6];
                verdict = posegate_tail(t.e, t.A, t.B, i, j, X, W, 3 * tid, co + 6 * c, nis_max, nis, cov);
                nis_out[c] = nis;
#pragma unroll
                for (int q = 0; q < 3; q++) err_out[3 * c + q] = t.e[q];
#pragma unroll
                for (int q = 0; q < 6; q++) cov_out[6 * c + q] = cov[q];
            }
            cf[c] = verdict;
        }
        __syncthreads();  // (the next block clears X; cf is published)
    }

    // ---- 4. the append, thread 0's; then the flags ----
    if (tid == 0) {
        if (append) *ne_out = posegate_append(E, Ec, C, cij, cz, co, cf, eij, ez, eo);
        *flags_out = 0;
    }
    __syncthreads();
    for (int c = tid; c < C; c += POSEGATE_TPB) cf_out[c] = cf[c];
}

}  // namespace lslam
