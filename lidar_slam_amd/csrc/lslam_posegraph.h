// lslam_posegraph.h — batched 2-D pose-graph optimisation: Gauss-Newton on one graph of keyframe poses
// and relative-pose edges per robot.  The definition is the comment on lslam_pose_graph in
// include/lidarslam.h; tests/posegraph_ref.py is its NumPy form; the edge terms, the packed triangle and
// the element steps of the LDL^T and of the substitutions are lslam_posegraph_core.h (plain C++, also
// compiled on the CPU).
//
// posegraph_kernel: one 256-thread workgroup per graph, every iteration in one launch.  The reduced
// system (node 0 is the gauge) lives in dynamic LDS, sized from max_nodes and max_edges by
// posegraph_lds_doubles: H as a packed lower triangle, g, the undivided column of the running LDL^T
// step, the poses and the stepped poses, (cos, sin) per node and chi per edge.  At 64 nodes and 1024
// edges that is 155 KiB, one workgroup a CU; at 24 nodes and 256 edges 23 KiB, six.
//
// Order decides the bits, so nothing is added atomically.  An evaluation gives every block of H (a
// node's diagonal block with its part of g, or a pair's block below the diagonal) to one thread, which
// walks the edge list from global memory in ascending order and adds what the edges on its node or
// pair contribute; chi per edge is computed by a thread per edge, and thread 0 adds them up in
// ascending order.  A column of the LDL^T is two passes with a barrier behind each: the rows below the
// pivot are divided (the undivided column is kept beside them), then every element (a, b) of the
// trailing triangle takes its one product and one subtraction.  The substitutions are a barrier per
// column.  The only atomics are ORs of flag bits into an LDS word (order-free).  All loops are bounded
// by n_iter, max_nodes and max_edges; every barrier is reached by the whole workgroup (the branches
// around them are uniform: they depend on LDS words read behind a barrier).
//
// Only the owning workgroup reads a graph's poses, and it writes pose_out at its very end, each thread
// the words it has just read: pose_out may be pose.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_posegraph_core.h"

namespace lslam {

constexpr int POSEGRAPH_TPB = 256;
constexpr int POSEGRAPH_LDS_MAX = 160 * 1024;

struct PoseGraphArgs {
    lslam_posegraph_batch b;
    lslam_posegraph_params p;
};

// the dynamic LDS in bytes: posegraph_lds_doubles and two doubles for the flag words and the chi2 sum
static inline int posegraph_lds_bytes(int N_cap, int E_cap) { return 8 * (posegraph_lds_doubles(N_cap, E_cap) + 2); }

// OR of `bits` over the workgroup.  w: two LDS words used in turn (`turn` flips per call, uniformly), so
// that a call's reset cannot meet the reads of the call before it.
__device__ static inline int posegraph_wg_or(int *w, int &turn, int tid, int bits) {
    int *slot = w + turn;
    turn ^= 1;
    if (tid == 0) *slot = 0;
    __syncthreads();
    if (bits) atomicOr(slot, bits);
    __syncthreads();
    return *slot;
}

// the dynamic LDS of a workgroup (posegraph_lds_doubles' parts, in its order)
struct PoseGraphLds {
    double *H;    // [tri(3 (N_cap - 1))]
    double *gv;   // [3 (N_cap - 1)] g, then y, z, x
    double *u;    // [3 (N_cap - 1)] the undivided column
    double *P;    // [N_cap][3] the poses as they stand
    double *Q;    // [N_cap][3] the stepped poses
    double *cs;   // [N_cap][2]
    double *chi;  // [E_cap]
    double *tot;  // chi2 of the evaluation
    int *words;   // two flag words
};
__device__ static inline PoseGraphLds posegraph_lds(unsigned char *smem, int Nc, int Ec) {
    const int ncap = posegraph_dim(Nc);
    PoseGraphLds l;
    l.H = (double *)smem;
    l.gv = l.H + posegraph_tri_size(ncap);
    l.u = l.gv + ncap;
    l.P = l.u + ncap;
    l.Q = l.P + 3 * Nc;
    l.cs = l.Q + 3 * Nc;
    l.chi = l.cs + 2 * Nc;
    l.tot = l.chi + Ec;
    l.words = (int *)(l.tot + 1);
    return l;
}

// FORM: 0 (a template, so that the kernel takes its place in the code object at launch_posegraph)
template <int FORM>
__global__ __launch_bounds__(POSEGRAPH_TPB) void posegraph_kernel(const PoseGraphArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x, G = (int64_t)a.b.n_graphs;
    const int Nc = a.p.max_nodes, Ec = a.p.max_edges, n_iter = a.p.n_iter;
    const PoseGraphLds L0 = posegraph_lds(smem, Nc, Ec);
    double *const P = L0.P;
    int *const words = L0.words;
    int turn = 0;

    const long long *in = (const long long *)a.b.pose;
    long long *out = (long long *)a.b.pose_out;
    const int32_t *eij = a.b.edge_ij + g * Ec * 2;
    const double *ez = a.b.edge_z + g * Ec * 3, *eo = a.b.edge_info + g * Ec * 6;
    // The kernel's arguments fill the scalar registers, and an edge read at a uniform index would be held
    // in more of them: the edge pointers and the step's constants are kept in vector registers, of which
    // there are enough, so that nothing spills.
    double eps_t = a.p.eps_t, eps_r = a.p.eps_r, damp_t = a.p.damp_t, damp_r = a.p.damp_r;
    double *chi2_out = a.b.chi2 + 2 * g, *echi = a.b.edge_chi2 + g * Ec;
    double *trace = a.b.trace + g * (int64_t)(n_iter + 1) * Nc * 2;
    int32_t *iters_out = a.b.iters + g, *flags_out = a.b.flags + g;
    asm volatile("" : "+v"(eij), "+v"(ez), "+v"(eo), "+v"(in), "+v"(out));
    asm volatile("" : "+v"(eps_t), "+v"(eps_r), "+v"(damp_t), "+v"(damp_r), "+v"(trace), "+v"(echi));
    asm volatile("" : "+v"(chi2_out), "+v"(iters_out), "+v"(flags_out));

    // ---- 0. checks ----
    const int N = a.b.n_nodes[g], E = a.b.n_edges[g];
    int flags = 0;
    if (N < 0 || E < 0 || N > Nc || E > Ec) {
        flags = LSLAM_POSEGRAPH_BAD_GRAPH;
    } else if (N < 2 || E == 0) {
        flags = LSLAM_POSEGRAPH_EMPTY;
    } else {
        bool bad = false;
        for (int i = tid; i < N; i += POSEGRAPH_TPB) {
#pragma unroll
            for (int c = 0; c < 3; c++) P[3 * i + c] = __longlong_as_double(in[((int64_t)i * G + g) * 3 + c]);
            bad |= !posegraph_finite3(P + 3 * i);
        }
        for (int e = tid; e < E; e += POSEGRAPH_TPB) {
            const int i = eij[2 * e], j = eij[2 * e + 1];
            bad |= i == j || i < 0 || i >= N || j < 0 || j >= N;
            bad |= !posegraph_finite3(ez + 3 * e) || !posegraph_finite3(eo + 6 * e) || !posegraph_finite3(eo + 6 * e + 3);
        }
        if (posegraph_wg_or(words, turn, tid, bad ? 1 : 0)) flags = LSLAM_POSEGRAPH_BAD_GRAPH;  // (the barriers publish P)
    }
    // the sizes' copies in vector registers, from which the loop and the outputs take theirs
    int N_v = N, E_v = E, Nc_v = Nc, Ec_v = Ec, G_v = a.b.n_graphs, g_v = (int)blockIdx.x;
    asm volatile("" : "+v"(N_v), "+v"(E_v), "+v"(Nc_v), "+v"(Ec_v), "+v"(G_v), "+v"(g_v));
    int iters = 0;
    double chi_first = 0.0, chi_last = 0.0;
    // (A graph that step 0 flags makes no evaluation: the loop is skipped, uniformly, and the outputs below
    // are its pose and zeros.)
    for (int k = 0; k <= n_iter && !(flags & (LSLAM_POSEGRAPH_EMPTY | LSLAM_POSEGRAPH_BAD_GRAPH)); k++) {
        // (The loop's bounds and the thread index are made opaque once per iteration: the compiler would
        // otherwise hoist every loop's lane masks out of the iteration and hold them, beside cos and sin's
        // constants, in more scalar registers than there are.)
        int tid_k = (int)threadIdx.x, N_k = N_v, E_k = E_v, Nc_k = Nc_v, Ec_k = Ec_v;
        asm volatile("" : "+v"(tid_k), "+v"(N_k), "+v"(E_k), "+v"(Nc_k), "+v"(Ec_k));
        const int tid = tid_k, N = __builtin_amdgcn_readfirstlane(N_k), E = __builtin_amdgcn_readfirstlane(E_k);
        const int Nc = __builtin_amdgcn_readfirstlane(Nc_k), Ec = __builtin_amdgcn_readfirstlane(Ec_k);
        const int n = posegraph_dim(N), nblk = (N - 1) * N / 2;
        const PoseGraphLds L = posegraph_lds(smem, Nc, Ec);
        double *const H = L.H, *const gv = L.gv, *const u = L.u, *const P = L.P, *const Q = L.Q, *const cs = L.cs;
        double *const chi = L.chi, *const tot = L.tot;
        int *const words = L.words;
        // ---- 1. evaluation k ----
        for (int i = tid; i < N; i += POSEGRAPH_TPB) {
            const double c = cos(P[3 * i + 2]), s = sin(P[3 * i + 2]);
            cs[2 * i] = c;
            cs[2 * i + 1] = s;
            trace[((int64_t)k * Nc + i) * 2] = c;
            trace[((int64_t)k * Nc + i) * 2 + 1] = s;
        }
        __syncthreads();
        for (int e = tid; e < E; e += POSEGRAPH_TPB) {
            const int i = eij[2 * e], j = eij[2 * e + 1];
            PosegraphEdge t;
            posegraph_edge(P + 3 * i, P + 3 * j, cs[2 * i], cs[2 * i + 1], ez + 3 * e, eo + 6 * e, t);
            chi[e] = t.chi;
            echi[e] = t.chi;
        }
        for (int blk = tid; blk < nblk; blk += POSEGRAPH_TPB) {
            int rn, cn;  // the block's reduced nodes, cn <= rn; their nodes are rn + 1 and cn + 1
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
                gv[r0] = gg[0];
                gv[r0 + 1] = gg[1];
                gv[r0 + 2] = gg[2];
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
            *tot = sum;
        }
        __syncthreads();
        chi_last = *tot;
        if (k == 0) chi_first = chi_last;
        if (k == n_iter || (flags & LSLAM_POSEGRAPH_CONVERGED)) break;  // the evaluation after the last step

        // ---- 2. step k: LDL^T, the substitutions, the stepped poses ----
        bool singular = false;
        for (int p = 0; p < n; p++) {
            const double d = H[posegraph_tri(p, p)];
            if (!fieldalign_pivot_ok(d)) {  // (uniform: every thread reads the same word)
                singular = true;
                break;
            }
            for (int r = p + 1 + tid; r < n; r += POSEGRAPH_TPB) posegraph_col_scale(H, u, p, r, d);
            __syncthreads();
            const int m = n - 1 - p, cnt = m * (m + 1) / 2;
            for (int t = tid; t < cnt; t += POSEGRAPH_TPB) {
                int r, c;
                posegraph_col_element(p, t, r, c);
                posegraph_col_update(H, u, p, r, c);
            }
            __syncthreads();
        }
        if (singular) {
            flags |= LSLAM_POSEGRAPH_SINGULAR;
            break;
        }
        for (int c = 0; c < n - 1; c++) {
            for (int r = c + 1 + tid; r < n; r += POSEGRAPH_TPB) posegraph_forward(H, gv, r, c);
            __syncthreads();
        }
        for (int r = tid; r < n; r += POSEGRAPH_TPB) gv[r] = gv[r] / H[posegraph_tri(r, r)];
        __syncthreads();
        for (int c = n - 1; c > 0; c--) {
            for (int r = tid; r < c; r += POSEGRAPH_TPB) posegraph_backward(H, gv, r, c);
            __syncthreads();
        }
        int bits = 0;
        for (int q = 3 + tid; q < 3 * N; q += POSEGRAPH_TPB) {  // (node 0 is not stepped)
            const double delta = -gv[q - 3];
            const double v = P[q] + delta;
            Q[q] = v;
            if (!__builtin_isfinite(v)) bits |= 1;
            if (!(fabs(delta) < (q % 3 == 2 ? eps_r : eps_t))) bits |= 2;
        }
        bits = posegraph_wg_or(words, turn, tid, bits);
        if (bits & 1) {
            flags |= LSLAM_POSEGRAPH_SINGULAR;
            break;
        }
        for (int q = 3 + tid; q < 3 * N; q += POSEGRAPH_TPB) P[q] = Q[q];
        iters = k + 1;
        if (!(bits & 2)) flags |= LSLAM_POSEGRAPH_CONVERGED;
        __syncthreads();
    }
    // ---- 3. gate, 4. outputs ----
    if (!(chi_last <= chi_first)) flags |= LSLAM_POSEGRAPH_DIVERGED;  // (0 <= 0 where nothing was evaluated)
    const bool keep = flags & (LSLAM_POSEGRAPH_EMPTY | LSLAM_POSEGRAPH_BAD_GRAPH | LSLAM_POSEGRAPH_SINGULAR | LSLAM_POSEGRAPH_DIVERGED);
    int tid_e = (int)threadIdx.x;  // (opaque, as in the loop: nothing derived is held across it)
    asm volatile("" : "+v"(tid_e), "+v"(N_v), "+v"(Nc_v), "+v"(Ec_v), "+v"(G_v), "+v"(g_v));
    const int Nc_e = __builtin_amdgcn_readfirstlane(Nc_v), N_e = __builtin_amdgcn_readfirstlane(N_v);
    const double *P_e = posegraph_lds(smem, Nc_e, __builtin_amdgcn_readfirstlane(Ec_v)).P;
    const int64_t G_e = (int64_t)__builtin_amdgcn_readfirstlane(G_v), g_e = (int64_t)__builtin_amdgcn_readfirstlane(g_v);
    for (int q = tid_e; q < 3 * Nc_e; q += POSEGRAPH_TPB) {
        const int64_t at = ((int64_t)(q / 3) * G_e + g_e) * 3 + q % 3;
        const long long w = in[at];
        out[at] = (keep || q >= 3 * N_e) ? w : __double_as_longlong(P_e[q]);
    }
    if (tid_e == 0) {
        chi2_out[0] = chi_first;
        chi2_out[1] = chi_last;
        *iters_out = iters;
        *flags_out = flags;
    }
}

}  // namespace lslam
