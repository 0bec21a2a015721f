// Camera-IMU extrinsic rotation from pairs of relative rotations on gfx950: the closed-form rotation
// calibration of VINS-Mono (CalibrationExRotation) on the motion-mode rotations the integrator already returns and the camera's
// relative rotations.  The definition is in include/islam_hip.h (islam_imu_extrinsic_rot_solve).
//
// A rigid mount q satisfies qb_i (x) q = q (x) qc_i for every pair, M_i q = 0 with M_i = L(qb_i) - R(qc_i); q is the unit eigenvector of
// the smallest eigenvalue of A = sum_i w_i rho_i M_i^T M_i.  Kernels (float64 arithmetic whatever the I/O type; the fixed-order sum
// between them and the launch sequence of the rounds on the host are imu_terms.h)
//   ex_pair_kernel     one lane per pair: the two quaternions normalised with w >= 0, in rounds >= 1 the Huber weight rho_i from the
//                      previous round's estimate (read from scratch), the pair's terms w rho M^T M (upper triangle, 10) | excluded
//                      (0 or 1) | takes part (0 or 1)
//   ex_partial_kernel  more than REACH pairs: the partial sums
//   ex_solve_kernel    the sum; lane 0 runs a cyclic Jacobi eigen-decomposition of the 4x4 in LDS, sorts the eigenvalues, writes the
//                      estimate for the next round and, after the last, the outputs
//   ex_res_kernel      one lane per pair: the angular residual under the final estimate (only when it is asked for)
// The 4x4 and its eigenvectors live in LDS and are indexed there: no private memory.  FMA contraction stays on (results are checked to
// a tolerance, not to the bit, against the numpy restatement of tests/test_imu_extrinsic_gpu.py).
#include <hip/hip_runtime.h>

#include <cmath>

#include "imu_terms.h"

using namespace islam;
using namespace islam::tsum;

namespace {

constexpr int NT = 12;                // per-pair terms: A upper triangle by rows (10) | excluded (1) | takes part (1)
constexpr int MAX_SWEEPS = 16;        // cap on the Jacobi sweeps (a 4x4 is at rounding level after 4 to 6)
constexpr double OFF_REL = 0x1p-56;   // a sweep that finds every off-diagonal entry at or below this share of the largest diagonal ends

// o = a (x) b, quaternions xyzw
__device__ __forceinline__ void qmul(const double (&a)[4], const double (&b)[4], double (&o)[4]) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}

// the quaternion at p, normalised, negated if its w < 0; false for a norm that is zero or not finite
template <class T>
__device__ __forceinline__ bool canonical(const T* __restrict__ p, double (&q)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = (double)p[k];
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const bool neg = q[3] < 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        q[k] = q[k] / n;
        if (neg) q[k] = -q[k];
    }
    return n > 0.0 && isfinite(n);
}

// theta = angle(b^-1 (x) q (x) c (x) q^-1) as 2 atan2(|vec|, |w|): resolved far below 1e-8, where acos of w is not
__device__ __forceinline__ double residual_angle(const double (&b)[4], const double (&c)[4], const double (&q)[4]) {
    const double qi[4] = {-q[0], -q[1], -q[2], q[3]}, bi[4] = {-b[0], -b[1], -b[2], b[3]};
    double t[4], u[4], e[4];
    qmul(q, c, t);
    qmul(t, qi, u);
    qmul(bi, u, e);
    return 2.0 * atan2(sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), fabs(e[3]));
}

// One lane per pair.  qhat: the previous round's estimate, NULL in round 0 (rho = 1).
template <class T>
__global__ __launch_bounds__(BLOCK) void ex_pair_kernel(const T* __restrict__ rot_imu, const T* __restrict__ rot_cam,
                                                        const double* __restrict__ weight, int P, double delta,
                                                        const double* __restrict__ qhat, double* __restrict__ terms) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const size_t s = (size_t)i;
    double t[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) t[q] = 0.0;
    const double w = weight ? weight[s] : 1.0;
    if (w != 0.0) {                                       // a pair of weight zero takes no part, whatever its data holds
        double b[4], c[4];
        const bool okb = canonical(rot_imu + 4 * s, b), okc = canonical(rot_cam + 4 * s, c);
        bool ok = okb && okc && isfinite(w) && w > 0.0;
        double wr = w;
        if (qhat && ok) {                                 // Huber on the angular residual under the previous estimate
            const double q[4] = {qhat[0], qhat[1], qhat[2], qhat[3]};
            const double th = residual_angle(b, c, q);
            wr = w * fmin(1.0, delta / th);               // (theta = 0: delta / 0 = inf, rho = 1)
        }
        // M = L(b) - R(c) with d = bw - cw, s = vec(b) + vec(c), m = vec(b) - vec(c)
        const double d = b[3] - c[3];
        const double sx = b[0] + c[0], sy = b[1] + c[1], sz = b[2] + c[2];
        const double mx = b[0] - c[0], my = b[1] - c[1], mz = b[2] - c[2];
        const double M[4][4] = {{d, -sz, sy, mx}, {sz, d, -sx, my}, {-sy, sx, d, mz}, {-mx, -my, -mz, d}};
        int idx = 0;
        double tf = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = a; e < 4; ++e) {
                const double v = wr * (M[0][a] * M[0][e] + M[1][a] * M[1][e] + M[2][a] * M[2][e] + M[3][a] * M[3][e]);
                tf += fabs(v);
                t[idx++] = v;
            }
        ok = ok && isfinite(tf);
        if (ok) {
            t[NT - 1] = 1.0;
        } else {                                          // excluded and counted
#pragma unroll
            for (int q = 0; q < NT - 2; ++q) t[q] = 0.0;
            t[NT - 2] = 1.0;
        }
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) terms[(size_t)q * P + s] = t[q];
}

__global__ __launch_bounds__(BLOCK) void ex_partial_kernel(const double* __restrict__ terms, int P, int nblocks, double* __restrict__ partial) {
    partial_sum<NT>(terms, P, nblocks, partial);
}

struct EigLds {
    double A[16], V[16], lam[4], q[4];
    int ord[4];
};

// Cyclic Jacobi on the symmetric 4x4 E.A (destroyed: its diagonal ends as the eigenvalues), E.V = the eigenvectors by columns.
// Every array lives in LDS.
__device__ void jacobi4(EigLds& E) {
    for (int k = 0; k < 16; ++k) E.V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int p = 0; p < 4; ++p) {
            dg = fmax(dg, fabs(E.A[5 * p]));
            for (int q = p + 1; q < 4; ++q) off = fmax(off, fabs(E.A[4 * p + q]));
        }
        if (!(off > OFF_REL * dg)) break;                 // (also ends on a NaN)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = E.A[4 * p + q];
                if (apq == 0.0) continue;
                const double th = (E.A[5 * q] - E.A[5 * p]) / (2.0 * apq);
                const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
                for (int k = 0; k < 4; ++k) {             // columns p, q of A and of V
                    const double akp = E.A[4 * k + p], akq = E.A[4 * k + q];
                    E.A[4 * k + p] = c * akp - sn * akq;
                    E.A[4 * k + q] = sn * akp + c * akq;
                    const double vkp = E.V[4 * k + p], vkq = E.V[4 * k + q];
                    E.V[4 * k + p] = c * vkp - sn * vkq;
                    E.V[4 * k + q] = sn * vkp + c * vkq;
                }
                for (int k = 0; k < 4; ++k) {             // rows p, q of A
                    const double apk = E.A[4 * p + k], aqk = E.A[4 * q + k];
                    E.A[4 * p + k] = c * apk - sn * aqk;
                    E.A[4 * q + k] = sn * apk + c * aqk;
                }
                E.A[4 * p + q] = E.A[4 * q + p] = 0.0;
            }
    }
}

// One workgroup: the fixed-order sum of `count` term vectors (src[q ld + c]), then the eigen-decomposition on lane 0.  The estimate goes
// to qhat (scratch) for the next round, and with `last` to out_q / out_eig.
__global__ __launch_bounds__(BLOCK) void ex_solve_kernel(const double* __restrict__ src, int ld, int count, int last, int* __restrict__ status,
                                                         double* __restrict__ qhat, double* __restrict__ out_q, double* __restrict__ out_eig) {
    __shared__ double wsum[4 * NT], tot[NT];
    __shared__ EigLds E;
    block_sum<NT>(src, (size_t)ld, 0, (size_t)count, wsum, tot);
    if (threadIdx.x != 0) return;
    const bool any = tot[NT - 1] > 0.0;
    int idx = 0;
    for (int a = 0; a < 4; ++a)
        for (int b = a; b < 4; ++b) { E.A[4 * a + b] = E.A[4 * b + a] = tot[idx]; ++idx; }
    jacobi4(E);
    for (int k = 0; k < 4; ++k) { E.lam[k] = E.A[5 * k]; E.ord[k] = k; }
    for (int a = 1; a < 4; ++a)                           // ascending; equal values keep their order
        for (int b = a; b > 0 && E.lam[E.ord[b]] < E.lam[E.ord[b - 1]]; --b) {
            const int o = E.ord[b];
            E.ord[b] = E.ord[b - 1];
            E.ord[b - 1] = o;
        }
    const int c0 = E.ord[0];
    const double x = E.V[c0], y = E.V[4 + c0], z = E.V[8 + c0], w = E.V[12 + c0];
    const double n = sqrt(x * x + y * y + z * z + w * w);
    const double sg = w < 0.0 ? -1.0 : 1.0;
    E.q[0] = sg * (x / n); E.q[1] = sg * (y / n); E.q[2] = sg * (z / n); E.q[3] = sg * (w / n);
    for (int k = 0; k < 4; ++k) {
        qhat[k] = any ? E.q[k] : 0.0;
        if (last) {
            out_q[k] = any ? E.q[k] : 0.0;
            out_eig[k] = any ? E.lam[E.ord[k]] : 0.0;
        }
    }
    status[0] = any ? 0 : 1;
    status[1] = (int)tot[NT - 2];
}

// One lane per pair: theta_i under the final estimate, NaN for an invalid quaternion; zeros when no pair took part.
template <class T>
__global__ __launch_bounds__(BLOCK) void ex_res_kernel(const T* __restrict__ rot_imu, const T* __restrict__ rot_cam, int P,
                                                       const double* __restrict__ qhat, const int* __restrict__ status,
                                                       double* __restrict__ out_res) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const size_t s = (size_t)i;
    double th = 0.0;
    if (status[0] == 0) {
        double b[4], c[4];
        const bool okb = canonical(rot_imu + 4 * s, b), okc = canonical(rot_cam + 4 * s, c);
        const double q[4] = {qhat[0], qhat[1], qhat[2], qhat[3]};
        th = okb && okc ? residual_angle(b, c, q) : nan("");
    }
    out_res[s] = th;
}

template <class T>
int run(const void* rot_imu_v, const void* rot_cam_v, const double* weight, int P, double delta, int rounds, double* out_q, double* out_eig,
        double* out_res, void* scratch, hipStream_t s) {
    const T *rot_imu = (const T*)rot_imu_v, *rot_cam = (const T*)rot_cam_v;
    const Scratch sc(scratch, NT, P);
    const dim3 grid((P + BLOCK - 1) / BLOCK);
    return run_rounds(
        sc, P, ex_partial_kernel, delta, rounds, s,
        [&](const double* qhat) {
            hipLaunchKernelGGL(ex_pair_kernel<T>, grid, dim3(BLOCK), 0, s, rot_imu, rot_cam, weight, P, delta, qhat, sc.terms);
        },
        [&](int, int last) {
            hipLaunchKernelGGL(ex_solve_kernel, dim3(1), dim3(BLOCK), 0, s, sc.src, sc.count, sc.count, last, sc.status, sc.est, out_q, out_eig);
        },
        [&] {
            if (out_res && P > 0)
                hipLaunchKernelGGL(ex_res_kernel<T>, grid, dim3(BLOCK), 0, s, rot_imu, rot_cam, P, (const double*)sc.est, (const int*)sc.status,
                                   out_res);
        },
        [&](int excluded) {
            return fail(ISLAM_ENOTPD, "islam_imu_extrinsic_rot_solve: no pair of %d takes part (%d excluded)", P, excluded);
        });
}

}  // namespace

extern "C" {

size_t islam_imu_extrinsic_rot_solve_scratch_bytes(int rows) {
    return Scratch::bytes(NT, rows > 0 ? rows : 0);
}

int islam_imu_extrinsic_rot_solve(const void* rot_imu, const void* rot_cam, const double* weight, int rows, double delta, int rounds,
                                  double* out_q, double* out_eig, double* out_res, void* scratch, int dtype, void* stream) {
    if (const int rc = check_entry("islam_imu_extrinsic_rot_solve", rows, dtype, delta, rounds)) return rc;
    if (!out_q || !out_eig || !scratch) return fail(ISLAM_EARG, "islam_imu_extrinsic_rot_solve: out_q / out_eig / scratch is NULL");
    if (rows > 0 && (!rot_imu || !rot_cam)) return fail(ISLAM_EARG, "islam_imu_extrinsic_rot_solve: rot_imu / rot_cam is NULL (rows=%d)", rows);
    return (dtype == ISLAM_F64 ? run<double> : run<float>)(rot_imu, rot_cam, weight, rows, delta, rounds, out_q, out_eig, out_res, scratch,
                                                           as_stream(stream));
}

}  // extern "C"
