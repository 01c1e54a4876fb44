// lslam_fieldfuse.h — the field alignment fused into the filter: the aligned pose of lslam_fieldalign.h
// as a measurement of the pose, with an information matrix built from the alignment's own normal
// equations, and a gated Kalman update of the filter's mean and covariance in information form.  The
// definition is the comment on lslam_field_fuse in include/lidarslam.h; tests/fieldfuse_ref.py is its
// NumPy form; the 3 x 3 algebra is lslam_fieldfuse_core.h (plain C++, also compiled on the CPU).
//
// fieldalign_kernel runs first, unchanged, with pose_out := z.  fieldfuse_kernel follows on the same
// stream: one thread per robot, 64 threads to a workgroup, so that a fleet of 4096 spreads over 64
// workgroups rather than 16.  A thread reads its robot's pose, z, P, the ten sums, n_last and the flags,
// runs steps 5-11 (some three hundred FP64 operations, every loop unrolled: the matrices stay in
// registers, there is no scratch and no LDS), writes the outputs and ORs its two flags into the word.
// The thread that writes a robot's pose_out and P_out is the one that read its pose and P, and writes
// after it: each pair may be one buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lidarslam.h"
#include "lslam_fieldalign.h"
#include "lslam_fieldfuse_core.h"

namespace lslam {

static_assert(FIELDFUSE_OUTLIER == LSLAM_FIELDFUSE_OUTLIER && FIELDFUSE_BAD_COV == LSLAM_FIELDFUSE_BAD_COV, "flags");

constexpr int FIELDFUSE_TPB = 64;

struct FieldFuseArgs {
    int n_robots;
    const double *pose, *P, *z;
    const int64_t *normal;
    const int32_t *n_used;
    int32_t *flags;
    double *pose_out, *P_out, *info, *info_f, *s2, *nis;
    FieldFuseConsts k;
};

// (A template only for its place in the code object, as mapfuse_pick_kernel is: the code object's last.
// The rule is at the include of lslam_launch_map.h in lslam_launch.h.)
template <int kForm>
__global__ __launch_bounds__(FIELDFUSE_TPB) void fieldfuse_kernel(const FieldFuseArgs a) {
    const int r = (int)blockIdx.x * FIELDFUSE_TPB + (int)threadIdx.x;
    if (r >= a.n_robots) return;
    const int64_t r3 = 3 * (int64_t)r, r9 = 9 * (int64_t)r;
    const unsigned long long *pin = (const unsigned long long *)a.pose + r3;
    const unsigned long long *Pin = (const unsigned long long *)a.P + r9;
    unsigned long long xb[3], Pb[9];
    double x[3], P[9], z[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        xb[i] = pin[i];
        x[i] = __longlong_as_double((long long)xb[i]);
        z[i] = a.z[r3 + i];
    }
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Pb[i] = Pin[i];
        P[i] = __longlong_as_double((long long)Pb[i]);
    }
    const int flags = a.flags[r];
    int64_t N[10];
#pragma unroll
    for (int i = 0; i < 10; i++) N[i] = a.normal[10 * (int64_t)r + i];
    // ---- 5. a rejected alignment: straight-line code, the steps' results are dropped by selects ----
    const int keep = LSLAM_FIELDALIGN_BAD_POSE | LSLAM_FIELDALIGN_SINGULAR | LSLAM_FIELDALIGN_FEW |
                     LSLAM_FIELDALIGN_DIVERGED | LSLAM_FIELDALIGN_WEAK;
    const bool rej = (flags & keep) != 0;
    double s2, nis, info[9], info_f[9], xo[3], Po[9];
    const int got = fieldfuse_steps(N, a.n_used[r3 + 1], a.k, x, P, z, s2, info, info_f, nis, xo, Po);
    const int add = rej ? 0 : got;
    const bool update = !rej && got == 0;
    // ---- outputs: after every read of this robot's pose and P ----
    unsigned long long *pout = (unsigned long long *)a.pose_out + r3, *Pout = (unsigned long long *)a.P_out + r9;
#pragma unroll
    for (int i = 0; i < 3; i++) pout[i] = update ? (unsigned long long)__double_as_longlong(xo[i]) : xb[i];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        Pout[i] = update ? (unsigned long long)__double_as_longlong(Po[i]) : Pb[i];
        a.info[r9 + i] = rej ? 0.0 : info[i];
        a.info_f[r9 + i] = rej ? 0.0 : info_f[i];
    }
    a.s2[r] = rej ? 0.0 : s2;
    a.nis[r] = rej ? 0.0 : nis;
    if (add) a.flags[r] = flags | add;
}

}  // namespace lslam
