// The closed-form alignment solves from pre-integrated increments on gfx950: the linear visual-inertial alignment of ORB-SLAM-VI /
// VINS-Mono on the increments, bias Jacobians (section 3.12) and covariances (section 3.11) the library already produces.  One kernel
// family templated on the number of unknowns NX:
//   NX = 6   x = [g; b]          gravity, accelerometer bias and velocities (islam_imu_gravity_bias_solve)
//   NX = 10  x = [g; b; t; s]    the same with the lever arm t of the camera-IMU mount and the scale s of monocular positions as
//                                further linear unknowns (section 3.15, islam_imu_lever_scale_solve)
// The definitions are in include/islam_hip.h.
//
// For every pair of consecutive intervals i, i + 1 the velocities drop out of (P_i), (P_{i+1}), (V_i) and leave three equations
// A_i [g; b] = r_i; with the body position p_i = s q_i - R_i t (q_i the camera position, R_i the body rotation) they read
//   A_i [g; b] + T_i t - s Q_i = m_i.
// Kernels (float64 arithmetic whatever the I/O type; the term layout is imu_normal.h, the fixed-order sum between them and the launch
// sequence on the host imu_terms.h: one round, the velocities where the Huber solves have their residuals)
//   ga_pair_kernel     one lane per pair: Y = [A | r] (3 x 7) or [A | T | -Q | rhs] (3 x 11; the columns of unknowns that are not
//                      solved are exact zeros, and with s = 1 given Q moves to the right-hand side), the pair's covariance
//                      C_i = L L^T, the whitened L^-1 Y and the pair's terms w Y^T Y: H upper triangle | c | excluded (0 or 1)
//   ga_partial_kernel  more than REACH pairs: the partial sums
//   ga_solve_kernel    the sum; lane 0 compacts the unknowns that are solved (order g, b, t, s), solves by Cholesky in LDS, runs the
//                      four rounds of the gravity-norm constraint on the same (H, c) and scatters back into the layout of NX
//   ga_vel_kernel      one lane per pose: the body velocity v_i from (P_i), the last one from (V_{n-1})
// The small matrices of the solve live in LDS and are indexed there: no private memory.  FMA contraction stays on (results are
// checked to a tolerance, not to the bit, against the numpy restatements of tests/test_imu_align_gpu.py and tests/test_imu_lever_gpu.py).
#include <hip/hip_runtime.h>

#include <cmath>

#include "imu_mat.h"
#include "imu_normal.h"
#include "imu_terms.h"

using namespace islam;
using namespace islam::imat;
using namespace islam::normal;
using namespace islam::tsum;

namespace {

// The layout of the unknowns: g (0..2) | b (3..5) | t (6..8) | s (9); NX = 6 ends after b.
// One lane per pair of consecutive intervals i, i + 1 (P = rows - 1 pairs); it reads the poses i, i + 1, i + 2 <= rows.  lever, scale:
// which of t and s are solved (NX = 10 only).
template <int NX, class T>
__global__ __launch_bounds__(BLOCK) void ga_pair_kernel(const T* __restrict__ rot, const T* __restrict__ pos, const T* __restrict__ dts,
                                                        const T* __restrict__ dvel, const T* __restrict__ dpos, const double* __restrict__ jac,
                                                        const double* __restrict__ cov, const double* __restrict__ weight, int P, int lever,
                                                        int scale, double* __restrict__ terms) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= P) return;
    const size_t s = (size_t)i;
    double t[NT<NX>];
#pragma unroll
    for (int q = 0; q < NT<NX>; ++q) t[q] = 0.0;
    const double w = weight ? weight[s] : 1.0;
    if (w != 0.0) {                                       // a pair of weight zero takes no part, whatever its data holds
        const double d0 = (double)dts[s], d1 = (double)dts[s + 1];
        double R0[9], R1[9], p0[3], p1[3], p2[3], dv0[3], dp0[3], dp1[3];
        quat_mat(rot + 4 * s, R0);
        quat_mat(rot + 4 * (s + 1), R1);
        ld_vec(pos + 3 * s, p0); ld_vec(pos + 3 * (s + 1), p1); ld_vec(pos + 3 * (s + 2), p2);
        ld_vec(dvel + 3 * s, dv0); ld_vec(dpos + 3 * s, dp0); ld_vec(dpos + 3 * (s + 1), dp1);
        double u[3], a1[3], a0[3], Y[3][NX + 1];          // Y = [A | T | -Q | rhs], whitened in place below
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < NX + 1; ++c) Y[k][c] = 0.0;
        // r = Q + m,  Q = (p1 - p0) / d0 - (p2 - p1) / d1 of the positions,  m = R1 dp1 / d1 - R0 (dp0 / d0 - dv0);
        // with s solved the positions are the camera's, -Q is the column of s and m alone is the right-hand side
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = dp0[k] / d0 - dv0[k];
        mat_vec(R1, dp1, a1);
        mat_vec(R0, u, a0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double Q = (p1[k] - p0[k]) / d0 - (p2[k] - p1[k]) / d1;
            Y[k][NX] = Q + a1[k] / d1 - a0[k];
            if constexpr (NX == 10)
                if (scale) { Y[k][9] = -Q; Y[k][NX] = a1[k] / d1 - a0[k]; }
        }
        // A = [ -(d0 + d1) / 2 I | R0 (Jp0 / d0 - Jv0) - R1 Jp1 / d1 ]
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
        // T = (R1 - R0) / d0 - (R2 - R1) / d1
        if constexpr (NX == 10)
            if (lever) {
                double R2[9];
                quat_mat(rot + 4 * (s + 2), R2);
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) Y[k][6 + c] = (R1[3 * k + c] - R0[3 * k + c]) / d0 - (R2[3 * k + c] - R1[3 * k + c]) / d1;
            }
        double fin = 0.0;                                 // finite iff every entry of Y is
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < NX + 1; ++c) fin += fabs(Y[k][c]);
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
            for (int c = 0; c < NX + 1; ++c) {            // L Y' = Y
                const double y0 = Y[0][c] / l00;
                const double y1 = (Y[1][c] - l10 * y0) / l11;
                Y[2][c] = (Y[2][c] - l20 * y0 - l21 * y1) / l22;
                Y[1][c] = y1;
                Y[0][c] = y0;
            }
        }
        normal_terms<NX>(Y, w, ok, t);
    }
#pragma unroll
    for (int q = 0; q < NT<NX>; ++q) terms[(size_t)q * P + s] = t[q];
}

template <int NX>
__global__ __launch_bounds__(BLOCK) void ga_partial_kernel(const double* __restrict__ terms, int P, int nblocks, double* __restrict__ partial) {
    partial_sum<NT<NX>>(terms, P, nblocks, partial);
}

// the compacted system of the n unknowns that are solved, row stride NX
template <int NX>
struct SolveLds {
    double H[NX * NX], c[NX], L[NX * NX], x[NX], M[NX * NX], rr[NX], z[NX], r[NX], W[NX * 2], bb[6], gh[3];
    int at[NX];                       // the place of compact unknown a in the layout of NX
};

// The gravity-norm rounds on lane 0: x = [G gh; 0] + B z with B = [ b1 b2 0 ; 0 I ] (n x (n - 1)), z from the projected system
// M = B^T H B, rr = B^T (c - H [G gh; 0]); the other unknowns are carried along.  B is the identity outside its 3 x 2 block, so only the
// first two rows and columns of M are computed and the rest of it is H itself: the sums of the full products without the terms that the
// zeros and ones of B contribute (at n = 10 those were four fifths of the rounds' time on lane 0).
template <int NX>
__device__ bool norm_rounds(SolveLds<NX>& S, int n, double G) {
    const int m = n - 1;
    double gn = sqrt(S.x[0] * S.x[0] + S.x[1] * S.x[1] + S.x[2] * S.x[2]);
    if (!(gn > 0.0) || !isfinite(gn)) return false;
    for (int k = 0; k < 3; ++k) S.gh[k] = S.x[k] / gn;
    for (int round = 0; round < 4; ++round) {
        int e = 0;                                        // the axis with the smallest |gh . e|, the lowest index on a tie
        for (int k = 1; k < 3; ++k)
            if (fabs(S.gh[k]) < fabs(S.gh[e])) e = k;
        const double ge = S.gh[e], g0 = S.gh[0], g1 = S.gh[1], g2 = S.gh[2];
        double b10 = -ge * g0, b11 = -ge * g1, b12 = -ge * g2;
        if (e == 0) b10 += 1.0; else if (e == 1) b11 += 1.0; else b12 += 1.0;
        const double bn = sqrt(b10 * b10 + b11 * b11 + b12 * b12);
        b10 /= bn; b11 /= bn; b12 /= bn;
        S.bb[0] = b10; S.bb[1] = b11; S.bb[2] = b12;      // b1, then b2 = gh x b1
        S.bb[3] = g1 * b12 - g2 * b11;
        S.bb[4] = g2 * b10 - g0 * b12;
        S.bb[5] = g0 * b11 - g1 * b10;
        for (int k = 0; k < n; ++k) {                     // r = c - H [G gh; 0],  W = H [b1 b2; 0]
            const double h0 = S.H[NX * k], h1 = S.H[NX * k + 1], h2 = S.H[NX * k + 2];
            S.r[k] = S.c[k] - G * (h0 * g0 + h1 * g1 + h2 * g2);
            for (int j = 0; j < 2; ++j) S.W[2 * k + j] = h0 * S.bb[3 * j] + h1 * S.bb[3 * j + 1] + h2 * S.bb[3 * j + 2];
        }
        for (int i = 0; i < 2; ++i) {                     // the two rows and columns of M = B^T H B and of rr = B^T r that B touches
            const double c0 = S.bb[3 * i], c1 = S.bb[3 * i + 1], c2 = S.bb[3 * i + 2];
            for (int j = 0; j < 2; ++j) S.M[NX * i + j] = c0 * S.W[j] + c1 * S.W[2 + j] + c2 * S.W[4 + j];
            for (int j = 2; j < m; ++j) S.M[NX * i + j] = S.M[NX * j + i] = S.W[2 * (j + 1) + i];
            S.rr[i] = c0 * S.r[0] + c1 * S.r[1] + c2 * S.r[2];
        }
        S.M[1] = S.M[NX] = 0.5 * (S.M[1] + S.M[NX]);      // the exactly symmetric part: M_01 and M_10 differ by rounding
        for (int i = 2; i < m; ++i) {                     // the rest of M is H itself (none of it at n = 3)
            for (int j = 2; j < m; ++j) S.M[NX * i + j] = S.H[NX * (i + 1) + j + 1];
            S.rr[i] = S.r[i + 1];
        }
        if (!chol_solve<NX>(S.M, S.rr, m, S.L, S.z)) return false;
        const double u0 = G * g0 + S.bb[0] * S.z[0] + S.bb[3] * S.z[1];
        const double u1 = G * g1 + S.bb[1] * S.z[0] + S.bb[4] * S.z[1];
        const double u2 = G * g2 + S.bb[2] * S.z[0] + S.bb[5] * S.z[1];
        gn = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
        if (!(gn > 0.0) || !isfinite(gn)) return false;
        S.gh[0] = u0 / gn; S.gh[1] = u1 / gn; S.gh[2] = u2 / gn;
    }
    for (int k = 0; k < 3; ++k) S.x[k] = G * S.gh[k];
    for (int k = 3; k < n; ++k) S.x[k] = S.z[k - 1];
    return true;
}

// One workgroup: the fixed-order sum of `count` term vectors (src[q ld + c]), then the solve on lane 0.  has_b / lever / scale say
// which unknowns beside g are solved; the others come out as exact 0.0 (b, t) and 1.0 (s).
template <int NX>
__global__ __launch_bounds__(BLOCK) void ga_solve_kernel(const double* __restrict__ src, int ld, int count, int has_b, int lever, int scale,
                                                         double G, int* __restrict__ status, double* __restrict__ out_x,
                                                         double* __restrict__ out_H) {
    __shared__ double wsum[4 * NT<NX>], tot[NT<NX>];
    __shared__ SolveLds<NX> S;
    block_sum<NT<NX>>(src, (size_t)ld, 0, (size_t)count, wsum, tot);
    if (threadIdx.x != 0) return;
    int at[NX];
    const int n = list_solved<NX>([=](int a) { return a < 3 || (a < 6 ? has_b != 0 : (a < 9 ? lever != 0 : scale != 0)); }, S.at, at);
    gather_solved<NX>(tot, at, S.H, S.c);
    bool pd = chol_solve<NX>(S.H, S.c, n, S.L, S.x);
    if (pd && G > 0.0) pd = norm_rounds(S, n, G);
    for (int a = 0; a < NX; ++a) out_x[a] = pd && a == 9 ? 1.0 : 0.0;
    if (pd) scatter_solved<NX>(S.x, at, n, out_x);
    if (out_H) write_full_H<NX>(tot, out_H);
    status[0] = pd ? 0 : 1;
    status[1] = (int)tot[NT<NX> - 1];
}

// One lane per pose: the velocity of the body.  v_i of an interval with d_i > 0 comes from (P_i), with p = s q - R t at NX = 10; a pose
// whose own interval is missing or empty (the last pose, a frame without samples) takes (P_{i-1}) and (V_{i-1}) of the interval in
// front of it; with neither it is NaN.  Either way it reads the poses k and k + 1 <= rows.  A failed solve: zeros.
template <int NX, class T>
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
            double R[9], p0[3], p1[3], dp[3], dv[3], rp[3], step[3];
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
#pragma unroll
            for (int c = 0; c < 3; ++c) step[c] = p1[c] - p0[c];   // of the body
            if constexpr (NX == 10) {                     // s (q1 - q0) - (R1 - R) t
                const double t[3] = {x[6], x[7], x[8]}, sc = x[9];
                double R1[9], rt[3];
                quat_mat(rot + 4 * (s + 1), R1);
#pragma unroll
                for (int c = 0; c < 9; ++c) R1[c] -= R[c];
                mat_vec(R1, t, rt);
#pragma unroll
                for (int c = 0; c < 3; ++c) step[c] = sc * step[c] - rt[c];
            }
            mat_vec(R, dp, rp);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (step[c] - 0.5 * g[c] * d * d - rp[c]) / d;
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

template <int NX, class T>
int run(const char* name, const void* rot_v, const void* pos_v, const void* dts_v, const void* dvel_v, const void* dpos_v, const double* jac,
        const double* cov, const double* weight, int rows, int lever, int scale, double G, double* out_x, double* out_H, double* out_vel,
        void* scratch, hipStream_t s) {
    const T *rot = (const T*)rot_v, *pos = (const T*)pos_v, *dts = (const T*)dts_v, *dvel = (const T*)dvel_v, *dpos = (const T*)dpos_v;
    const int P = rows > 1 ? rows - 1 : 0;
    const Scratch sc(scratch, NT<NX>, P);
    return run_rounds(
        sc, P, ga_partial_kernel<NX>, 0.0, 0, s,
        [&](const double*) {
            hipLaunchKernelGGL((ga_pair_kernel<NX, T>), dim3((P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, rot, pos, dts, dvel, dpos, jac, cov,
                               weight, P, lever, scale, sc.terms);
        },
        [&](int, int) {
            hipLaunchKernelGGL(ga_solve_kernel<NX>, dim3(1), dim3(BLOCK), 0, s, sc.src, sc.count, sc.count, jac ? 1 : 0, lever, scale, G,
                               sc.status, out_x, out_H);
        },
        [&] {
            if (out_vel)
                hipLaunchKernelGGL((ga_vel_kernel<NX, T>), dim3(rows / BLOCK + 1), dim3(BLOCK), 0, s, rot, pos, dts, dvel, dpos, jac, rows,
                                   (const double*)out_x, (const int*)sc.status, out_vel);
        },
        [&](int excluded) {
            return fail(ISLAM_ENOTPD, "%s: the normal matrix of %d pairs (%d excluded) is not positive definite", name, P, excluded);
        });
}

// What the two entry points check alike, then the call.  poses: the names of the two pose arguments in the messages.
template <int NX>
int solve(const char* name, const char* poses, const void* rot, const void* pos, const void* dts, const void* dvel, const void* dpos,
          const double* jac, const double* cov, const double* weight, int rows, int lever, int scale, double gravity_norm, double* out_x,
          double* out_H, double* out_vel, void* scratch, int dtype, void* stream) {
    if (const int rc = check_entry(name, rows, dtype)) return rc;
    if (!(gravity_norm >= 0.0) || !std::isfinite(gravity_norm))
        return fail(ISLAM_EARG, "%s: gravity_norm %g (0 = free, > 0 = the known magnitude)", name, gravity_norm);
    if (!out_x || !scratch) return fail(ISLAM_EARG, "%s: out_x / scratch is NULL", name);
    if (!rot || !pos) return fail(ISLAM_EARG, "%s: %s is NULL (rows + 1 = %d poses)", name, poses, rows + 1);
    if (rows > 0 && (!dts || !dvel || !dpos)) return fail(ISLAM_EARG, "%s: dts / dvel / dpos is NULL (rows=%d)", name, rows);
    return (dtype == ISLAM_F64 ? run<NX, double> : run<NX, float>)(name, rot, pos, dts, dvel, dpos, jac, cov, weight, rows, lever, scale,
                                                                   gravity_norm, out_x, out_H, out_vel, scratch, as_stream(stream));
}

}  // namespace

extern "C" {

size_t islam_imu_gravity_bias_solve_scratch_bytes(int rows) {
    return Scratch::bytes(NT<6>, rows > 1 ? rows - 1 : 0);
}

int islam_imu_gravity_bias_solve(const void* rot_ref, const void* pos_ref, const void* dts, const void* dvel, const void* dpos,
                                 const double* jac, const double* cov, const double* weight, int rows, double gravity_norm, double* out_x,
                                 double* out_H, double* out_vel, void* scratch, int dtype, void* stream) {
    return solve<6>("islam_imu_gravity_bias_solve", "rot_ref / pos_ref", rot_ref, pos_ref, dts, dvel, dpos, jac, cov, weight, rows, 0, 0,
                    gravity_norm, out_x, out_H, out_vel, scratch, dtype, stream);
}

size_t islam_imu_lever_scale_solve_scratch_bytes(int rows) {
    return Scratch::bytes(NT<10>, rows > 1 ? rows - 1 : 0);
}

int islam_imu_lever_scale_solve(const void* rot_body, const void* pos_cam, const void* dts, const void* dvel, const void* dpos,
                                const double* jac, const double* cov, const double* weight, int rows, int solve_lever, int solve_scale,
                                double gravity_norm, double* out_x, double* out_H, double* out_vel, void* scratch, int dtype, void* stream) {
    if ((solve_lever != 0 && solve_lever != 1) || (solve_scale != 0 && solve_scale != 1))
        return fail(ISLAM_EARG, "islam_imu_lever_scale_solve: solve_lever=%d, solve_scale=%d (0 or 1 each)", solve_lever, solve_scale);
    if (solve_lever == 0 && solve_scale == 0)
        return fail(ISLAM_EARG, "islam_imu_lever_scale_solve: neither the lever arm nor the scale is solved: that solve is "
                                "islam_imu_gravity_bias_solve, on the positions of the body");
    return solve<10>("islam_imu_lever_scale_solve", "rot_body / pos_cam", rot_body, pos_cam, dts, dvel, dpos, jac, cov, weight, rows,
                     solve_lever, solve_scale, gravity_norm, out_x, out_H, out_vel, scratch, dtype, stream);
}

}  // extern "C"
