// Gravity, accelerometer-bias and velocity solve from pre-integrated increments on gfx950: the linear
// visual-inertial alignment of ORB-SLAM-VI / VINS-Mono on the increments, bias Jacobians (section 3.12) and covariances (section 3.11)
// the library already produces.  The definition is in include/islam_hip.h (islam_imu_gravity_bias_solve).
//
// For every pair of consecutive intervals i, i + 1 the velocities drop out of (P_i), (P_{i+1}), (V_i) and leave three equations
// A_i x = r_i in x = [g; b].  Kernels (float64 arithmetic whatever the I/O type; the fixed-order sum between them is imu_terms.h)
//   ga_pair_kernel     one lane per pair: A_i, r_i, the pair's covariance C_i = L L^T, the whitened L^-1 [A | r] and the pair's terms
//                      w A^T C^-1 A (upper triangle, 21) | w A^T C^-1 r (6) | excluded (0 or 1)
//   ga_partial_kernel  more than REACH pairs: the partial sums
//   ga_solve_kernel    the sum; lane 0 solves by Cholesky in LDS: the free 6x6 (3x3 without Jacobians), then the four rounds of the
//                      gravity-norm constraint on the same (H, c)
//   ga_vel_kernel      one lane per pose: v_i from (P_i), the last one from (V_{n-1})
// The small matrices of the solve live in LDS and are indexed there: no private memory.  FMA contraction stays on (results are
// checked to a tolerance, not to the bit, against the numpy restatement of tests/test_imu_align_gpu.py).
#include <hip/hip_runtime.h>

#include <cmath>

#include "imu_mat.h"
#include "imu_terms.h"

using namespace islam;
using namespace islam::imat;
using namespace islam::tsum;

namespace {

constexpr int NT = 28;                // per-pair terms: H upper triangle by rows (21) | c (6) | excluded (1)

// One lane per pair of consecutive intervals i, i + 1 (P = rows - 1 pairs).
template <class T>
__global__ __launch_bounds__(BLOCK) void ga_pair_kernel(const T* __restrict__ rot, const T* __restrict__ pos, const T* __restrict__ dts,
                                                        const T* __restrict__ dvel, const T* __restrict__ dpos, const double* __restrict__ jac,
                                                        const double* __restrict__ cov, const double* __restrict__ weight, int P,
                                                        double* __restrict__ terms) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const size_t s = (size_t)i;
    double t[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) t[q] = 0.0;
    const double w = weight ? weight[s] : 1.0;
    if (w != 0.0) {                                       // a pair of weight zero takes no part, whatever its data holds
        const double d0 = (double)dts[s], d1 = (double)dts[s + 1];
        double R0[9], R1[9], p0[3], p1[3], p2[3], dv0[3], dp0[3], dp1[3];
        quat_mat(rot + 4 * s, R0);
        quat_mat(rot + 4 * (s + 1), R1);
        ld_vec(pos + 3 * s, p0); ld_vec(pos + 3 * (s + 1), p1); ld_vec(pos + 3 * (s + 2), p2);
        ld_vec(dvel + 3 * s, dv0); ld_vec(dpos + 3 * s, dp0); ld_vec(dpos + 3 * (s + 1), dp1);
        // r = (p1 - p0) / d0 - (p2 - p1) / d1 + R1 dp1 / d1 - R0 (dp0 / d0 - dv0)
        double u[3], a1[3], a0[3], Y[3][7];               // Y = [A | r], whitened in place below
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = dp0[k] / d0 - dv0[k];
        mat_vec(R1, dp1, a1);
        mat_vec(R0, u, a0);
#pragma unroll
        for (int k = 0; k < 3; ++k) Y[k][6] = (p1[k] - p0[k]) / d0 - (p2[k] - p1[k]) / d1 + a1[k] / d1 - a0[k];
        // A = [ -(d0 + d1) / 2 I | R0 (Jp0 / d0 - Jv0) - R1 Jp1 / d1 ]
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 6; ++c) Y[k][c] = 0.0;
        Y[0][0] = Y[1][1] = Y[2][2] = -0.5 * (d0 + d1);
        if (jac) {
            double Jv0[9], Jp0[9], Jp1[9], U[9], B0[9], B1[9];
            ld_block(jac + 54 * s, 6, 3, 3, Jv0);
            ld_block(jac + 54 * s, 6, 6, 3, Jp0);
            ld_block(jac + 54 * (s + 1), 6, 6, 3, Jp1);
#pragma unroll
            for (int k = 0; k < 9; ++k) U[k] = Jp0[k] / d0 - Jv0[k];
            mat_mat(R0, U, B0);
            mat_mat(R1, Jp1, B1);
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) Y[k][3 + c] = B0[3 * k + c] - B1[3 * k + c] / d1;
        }
        double fin = 0.0;                                 // finite iff every entry of A and r is
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 7; ++c) fin += fabs(Y[k][c]);
        bool ok = isfinite(w) && d0 > 0.0 && d1 > 0.0 && isfinite(fin);
        if (cov) {
            // C = R1 Spp1 R1^T / d1^2 + R0 (Spp0 / d0^2 - (Spv0 + Svp0) / d0 + Svv0) R0^T, error state [phi, v, p]
            double Spp[9], Spv[9], Svp[9], Svv[9], M[9], RM[9], C0[9], C1[9];
            const double* S0 = cov + 81 * s;
            ld_block(S0, 9, 6, 6, Spp); ld_block(S0, 9, 6, 3, Spv); ld_block(S0, 9, 3, 6, Svp); ld_block(S0, 9, 3, 3, Svv);
#pragma unroll
            for (int k = 0; k < 9; ++k) M[k] = Spp[k] / (d0 * d0) - (Spv[k] + Svp[k]) / d0 + Svv[k];
            mat_mat(R0, M, RM);
            mat_matT(RM, R0, C0);
            ld_block(cov + 81 * (s + 1), 9, 6, 6, Spp);
            mat_mat(R1, Spp, RM);
            mat_matT(RM, R1, C1);
            // the symmetric part, C = L L^T
            const double c00 = C0[0] + C1[0] / (d1 * d1), c11 = C0[4] + C1[4] / (d1 * d1), c22 = C0[8] + C1[8] / (d1 * d1);
            const double c10 = 0.5 * (C0[3] + C0[1]) + 0.5 * (C1[3] + C1[1]) / (d1 * d1);
            const double c20 = 0.5 * (C0[6] + C0[2]) + 0.5 * (C1[6] + C1[2]) / (d1 * d1);
            const double c21 = 0.5 * (C0[7] + C0[5]) + 0.5 * (C1[7] + C1[5]) / (d1 * d1);
            const bool k0 = c00 > 0.0 && isfinite(c00);
            const double l00 = sqrt(c00), l10 = c10 / l00, l20 = c20 / l00;
            const double q1 = c11 - l10 * l10;
            const bool k1 = q1 > PIVOT_REL * c11 && isfinite(q1);
            const double l11 = sqrt(q1), l21 = (c21 - l20 * l10) / l11;
            const double q2 = c22 - l20 * l20 - l21 * l21;
            const bool k2 = q2 > PIVOT_REL * c22 && isfinite(q2);
            const double l22 = sqrt(q2);
            ok = ok && k0 && k1 && k2;
#pragma unroll
            for (int c = 0; c < 7; ++c) {                 // L Y' = Y
                const double y0 = Y[0][c] / l00;
                const double y1 = (Y[1][c] - l10 * y0) / l11;
                Y[2][c] = (Y[2][c] - l20 * y0 - l21 * y1) / l22;
                Y[1][c] = y1;
                Y[0][c] = y0;
            }
        }
        int idx = 0;
        double tf = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 7; ++b) {
                const double v = w * (Y[0][a] * Y[0][b] + Y[1][a] * Y[1][b] + Y[2][a] * Y[2][b]);
                tf += fabs(v);
                if (b < 6) t[idx++] = v; else t[21 + a] = v;
            }
        ok = ok && isfinite(tf);
        if (!ok) {                                        // excluded and counted
#pragma unroll
            for (int q = 0; q < NT - 1; ++q) t[q] = 0.0;
            t[NT - 1] = 1.0;
        }
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) terms[(size_t)q * P + s] = t[q];
}

__global__ __launch_bounds__(BLOCK) void ga_partial_kernel(const double* __restrict__ terms, int P, int nblocks, double* __restrict__ partial) {
    partial_sum<NT>(terms, P, nblocks, partial);
}

struct SolveLds {
    double H[36], c[6], L[36], x[6], B[36], HB[36], M[36], rr[6], z[6], gh[3];
};

// The gravity-norm rounds on lane 0: x = [G gh; 0] + B z with B = [ b1 b2 0 ; 0 I ] (n x (n - 1)), z from the projected system.
__device__ bool norm_rounds(SolveLds& S, int n, double G) {
    const int m = n - 1;
    double gn = sqrt(S.x[0] * S.x[0] + S.x[1] * S.x[1] + S.x[2] * S.x[2]);
    if (!(gn > 0.0) || !isfinite(gn)) return false;
    for (int k = 0; k < 3; ++k) S.gh[k] = S.x[k] / gn;
    for (int round = 0; round < 4; ++round) {
        int e = 0;                                        // the axis with the smallest |gh . e|, the lowest index on a tie
        for (int k = 1; k < 3; ++k)
            if (fabs(S.gh[k]) < fabs(S.gh[e])) e = k;
        const double ge = S.gh[e];
        double b1[3], b2[3];
        b1[0] = -ge * S.gh[0]; b1[1] = -ge * S.gh[1]; b1[2] = -ge * S.gh[2];
        if (e == 0) b1[0] += 1.0; else if (e == 1) b1[1] += 1.0; else b1[2] += 1.0;
        const double bn = sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
        b1[0] /= bn; b1[1] /= bn; b1[2] /= bn;
        b2[0] = S.gh[1] * b1[2] - S.gh[2] * b1[1];
        b2[1] = S.gh[2] * b1[0] - S.gh[0] * b1[2];
        b2[2] = S.gh[0] * b1[1] - S.gh[1] * b1[0];
        for (int k = 0; k < 36; ++k) S.B[k] = 0.0;
        for (int k = 0; k < 3; ++k) { S.B[6 * k] = b1[k]; S.B[6 * k + 1] = b2[k]; }
        for (int k = 3; k < n; ++k) S.B[6 * k + k - 1] = 1.0;
        for (int i = 0; i < n; ++i)                       // HB = H B
            for (int j = 0; j < m; ++j) {
                double v = 0.0;
                for (int k = 0; k < n; ++k) v += S.H[6 * i + k] * S.B[6 * k + j];
                S.HB[6 * i + j] = v;
            }
        for (int i = 0; i < m; ++i) {                     // M = B^T H B,  rr = B^T (c - H [G gh; 0])
            for (int j = 0; j < m; ++j) {
                double v = 0.0;
                for (int k = 0; k < n; ++k) v += S.B[6 * k + i] * S.HB[6 * k + j];
                S.M[6 * i + j] = v;
            }
            double v = 0.0;
            for (int k = 0; k < n; ++k)
                v += S.B[6 * k + i] * (S.c[k] - G * (S.H[6 * k] * S.gh[0] + S.H[6 * k + 1] * S.gh[1] + S.H[6 * k + 2] * S.gh[2]));
            S.rr[i] = v;
        }
        for (int i = 0; i < m; ++i)                       // the exactly symmetric part: M_ij and M_ji differ by rounding
            for (int j = 0; j < i; ++j) S.M[6 * i + j] = S.M[6 * j + i] = 0.5 * (S.M[6 * i + j] + S.M[6 * j + i]);
        if (!chol_solve<6>(S.M, S.rr, m, S.L, S.z)) return false;
        double g[3];
        for (int k = 0; k < 3; ++k) g[k] = G * S.gh[k] + b1[k] * S.z[0] + b2[k] * S.z[1];
        gn = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
        if (!(gn > 0.0) || !isfinite(gn)) return false;
        for (int k = 0; k < 3; ++k) S.gh[k] = g[k] / gn;
    }
    for (int k = 0; k < 3; ++k) S.x[k] = G * S.gh[k];
    for (int k = 3; k < n; ++k) S.x[k] = S.z[k - 1];
    return true;
}

// One workgroup: the fixed-order sum of `count` term vectors (src[q ld + c]), then the solve on lane 0.  n = 6, or 3 without Jacobians.
__global__ __launch_bounds__(BLOCK) void ga_solve_kernel(const double* __restrict__ src, int ld, int count, int n, double G,
                                                         int* __restrict__ status, double* __restrict__ out_x, double* __restrict__ out_H) {
    __shared__ double wsum[4 * NT], tot[NT];
    __shared__ SolveLds S;
    block_sum<NT>(src, (size_t)ld, 0, (size_t)count, wsum, tot);
    if (threadIdx.x != 0) return;
    int idx = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { S.H[6 * a + b] = S.H[6 * b + a] = tot[idx]; ++idx; }
    for (int a = 0; a < 6; ++a) { S.c[a] = tot[21 + a]; S.x[a] = 0.0; }
    bool pd = chol_solve<6>(S.H, S.c, n, S.L, S.x);
    if (pd && G > 0.0) pd = norm_rounds(S, n, G);
    for (int a = 0; a < 6; ++a) out_x[a] = pd && a < n ? S.x[a] : 0.0;
    if (out_H)
        for (int a = 0; a < 36; ++a) out_H[a] = S.H[a];
    status[0] = pd ? 0 : 1;
    status[1] = (int)tot[NT - 1];
}

// One lane per pose.  v_i of an interval with d_i > 0 comes from (P_i); a pose whose own interval is missing or empty (the last pose,
// a frame without samples) takes (P_{i-1}) and (V_{i-1}) of the interval in front of it; with neither it is NaN.  A failed solve: zeros.
template <class T>
__global__ __launch_bounds__(BLOCK) void ga_vel_kernel(const T* __restrict__ rot, const T* __restrict__ pos, const T* __restrict__ dts,
                                                       const T* __restrict__ dvel, const T* __restrict__ dpos, const double* __restrict__ jac,
                                                       int rows, const double* __restrict__ x, const int* __restrict__ status,
                                                       double* __restrict__ out_vel) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i > rows) return;
    double v[3] = {0.0, 0.0, 0.0};
    if (status[0] == 0) {
        int k = -1;
        if (i < rows && (double)dts[i] > 0.0) k = i;
        else if (i > 0 && (double)dts[i - 1] > 0.0) k = i - 1;
        if (k < 0) {
            v[0] = v[1] = v[2] = nan("");
        } else {
            const size_t s = (size_t)k;
            const double d = (double)dts[s];
            const double g[3] = {x[0], x[1], x[2]}, b[3] = {x[3], x[4], x[5]};
            double R[9], p0[3], p1[3], dp[3], dv[3], rp[3];
            quat_mat(rot + 4 * s, R);
            ld_vec(pos + 3 * s, p0); ld_vec(pos + 3 * (s + 1), p1);
            ld_vec(dpos + 3 * s, dp); ld_vec(dvel + 3 * s, dv);
            if (jac) {
                double Jv[9], Jp[9], jb[3];
                ld_block(jac + 54 * s, 6, 3, 3, Jv);
                ld_block(jac + 54 * s, 6, 6, 3, Jp);
                mat_vec(Jp, b, jb);
#pragma unroll
                for (int c = 0; c < 3; ++c) dp[c] += jb[c];
                mat_vec(Jv, b, jb);
#pragma unroll
                for (int c = 0; c < 3; ++c) dv[c] += jb[c];
            }
            mat_vec(R, dp, rp);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (p1[c] - p0[c] - 0.5 * g[c] * d * d - rp[c]) / d;
            if (k != i) {
                mat_vec(R, dv, rp);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] += g[c] * d + rp[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out_vel[3 * (size_t)i + c] = v[c];
}

template <class T>
int run(const T* rot, const T* pos, const T* dts, const T* dvel, const T* dpos, const double* jac, const double* cov, const double* weight,
        int rows, double G, double* out_x, double* out_H, double* out_vel, void* scratch, hipStream_t s) {
    const int P = rows > 1 ? rows - 1 : 0;
    const Scratch sc(scratch, NT, P);
    if (P > 0)
        hipLaunchKernelGGL(ga_pair_kernel<T>, dim3((P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, rot, pos, dts, dvel, dpos, jac, cov, weight, P, sc.terms);
    if (sc.blocks > 0) hipLaunchKernelGGL(ga_partial_kernel, dim3(sc.blocks), dim3(BLOCK), 0, s, (const double*)sc.terms, P, sc.blocks, sc.partial);
    hipLaunchKernelGGL(ga_solve_kernel, dim3(1), dim3(BLOCK), 0, s, sc.src, sc.count, sc.count, jac ? 6 : 3, G, sc.status, out_x, out_H);
    if (out_vel)
        hipLaunchKernelGGL(ga_vel_kernel<T>, dim3(rows / BLOCK + 1), dim3(BLOCK), 0, s, rot, pos, dts, dvel, dpos, jac, rows, (const double*)out_x,
                           (const int*)sc.status, out_vel);
    int host[2];
    if (const int rc = read_status(sc.status, s, host)) return rc;
    if (host[0] != 0)
        return fail(ISLAM_ENOTPD, "islam_imu_gravity_bias_solve: the normal matrix of %d pairs (%d excluded) is not positive definite", P, host[1]);
    return host[1];
}

}  // namespace

extern "C" {

size_t islam_imu_gravity_bias_solve_scratch_bytes(int rows) {
    return Scratch::bytes(NT, rows > 1 ? rows - 1 : 0);
}

int islam_imu_gravity_bias_solve(const void* rot_ref, const void* pos_ref, const void* dts, const void* dvel, const void* dpos,
                                 const double* jac, const double* cov, const double* weight, int rows, double gravity_norm, double* out_x,
                                 double* out_H, double* out_vel, void* scratch, int dtype, void* stream) {
    if (rows < 0) return fail(ISLAM_EARG, "islam_imu_gravity_bias_solve: rows=%d", rows);
    if (dtype != ISLAM_F64 && dtype != ISLAM_F32) return fail(ISLAM_EARG, "islam_imu_gravity_bias_solve: dtype %d", dtype);
    if (!(gravity_norm >= 0.0) || !std::isfinite(gravity_norm))
        return fail(ISLAM_EARG, "islam_imu_gravity_bias_solve: gravity_norm %g (0 = free, > 0 = the known magnitude)", gravity_norm);
    if (!out_x || !scratch) return fail(ISLAM_EARG, "islam_imu_gravity_bias_solve: out_x / scratch is NULL");
    if (!rot_ref || !pos_ref) return fail(ISLAM_EARG, "islam_imu_gravity_bias_solve: rot_ref / pos_ref is NULL (rows + 1 = %d poses)", rows + 1);
    if (rows > 0 && (!dts || !dvel || !dpos)) return fail(ISLAM_EARG, "islam_imu_gravity_bias_solve: dts / dvel / dpos is NULL (rows=%d)", rows);
    hipStream_t s = as_stream(stream);
    if (dtype == ISLAM_F64)
        return run<double>((const double*)rot_ref, (const double*)pos_ref, (const double*)dts, (const double*)dvel, (const double*)dpos, jac, cov,
                           weight, rows, gravity_norm, out_x, out_H, out_vel, scratch, s);
    return run<float>((const float*)rot_ref, (const float*)pos_ref, (const float*)dts, (const float*)dvel, (const float*)dpos, jac, cov, weight,
                      rows, gravity_norm, out_x, out_H, out_vel, scratch, s);
}

}  // extern "C"
