// Camera-IMU time offset and gyro bias from relative rotations on gfx950: section 3.12's gyro-bias solve with
// the offset td between the two clocks as a fourth linear unknown (the rotation-only temporal calibration that Kalibr starts from, the td
// state of VINS-Mono restricted to rotations).  The definition is in include/islam_hip.h (islam_imu_time_offset_solve).
//
// An image stamped t was taken at t + td on the IMU's clock.  Under the integrator's zero-order hold the pre-integrated rotation of row
// i over the moved window is Exp(-ws td) DR_i Exp(we td) = DR_i Exp(u_i td + O(td^2)), u_i = we - DR_i^T ws, with ws, we the samples that
// start at the row's two boundaries; with DR(b) = DR Exp(J_phig b) that leaves three equations per row, linear in x = [dbg(3); td]:
//   e_i = Log(DR_i^T DRref_i) = J_phig,i dbg + u_i td.
// Kernels (float64 arithmetic whatever the I/O type; the fixed-order sum between them and the launch sequence of the rounds on the host
// are imu_terms.h)
//   td_row_kernel      one lane per row: Y = [J_phig | u | e] (3 x 5; without the bias the columns of J are exact zeros), in rounds >= 1
//                      the Huber weight rho_i from the previous round's x (read from scratch), the row's terms w rho Y^T Y: upper
//                      triangle of the 4 x 4 (10) | c (4) | excluded (0 or 1)
//   td_partial_kernel  more than REACH rows: the partial sums
//   td_solve_kernel    the sum; lane 0 compacts the unknowns that are solved (4, or td alone), solves by Cholesky in LDS, scatters back,
//                      writes x for the next round and, after the last, the outputs
//   td_res_kernel      one lane per row: |e_i - Y_i x| under the final x (only when it is asked for)
//   td_shift_kernel    one lane per row: Exp(-ws tau) (x) rot (x) Exp(we tau), islam_imu_time_shift
// The small matrices of the solve live in LDS and are indexed there: no private memory.  FMA contraction stays on (results are checked
// to a tolerance, not to the bit, against the numpy restatement of tests/test_imu_time_offset_gpu.py).
#include <hip/hip_runtime.h>

#include <cmath>

#include "imu_mat.h"
#include "imu_normal.h"
#include "imu_terms.h"
#include "lie_dev.h"

using namespace islam;
using namespace islam::imat;
using namespace islam::normal;
using namespace islam::tsum;

namespace {

constexpr int NX = 4;                 // the layout of the unknowns: dbg (0..2) | td (3); NT<NX> terms per row (imu_normal.h): 10 | 4 | 1

// Y = [J_phig | u | e] of row s; jac NULL: the columns of J are exact zeros.  True iff every entry is finite.
template <class T>
__device__ __forceinline__ bool row_system(const double* __restrict__ jac, const T* __restrict__ rot_imu, const T* __restrict__ rot_ref,
                                           const T* __restrict__ rate_start, const T* __restrict__ rate_end, size_t s, double (&Y)[3][NX + 1]) {
    const T* a = rot_imu + 4 * s;
    const T* b = rot_ref + 4 * s;
    // e = Log(DR^T DRref) as islam_imu_gyro_bias_solve takes it: the quaternion with w >= 0, k = 2 atan2(|vec|, w) / |vec|
    // (a copy of gyro_bias_solve_kernel's lines: behind one shared function some instantiation of the kernels compiles differently)
    const double ax = -(double)a[0], ay = -(double)a[1], az = -(double)a[2], aw = (double)a[3];
    const double bx = (double)b[0], by = (double)b[1], bz = (double)b[2], bw = (double)b[3];
    double qx = aw * bx + ax * bw + ay * bz - az * by;
    double qy = aw * by - ax * bz + ay * bw + az * bx;
    double qz = aw * bz + ax * by - ay * bx + az * bw;
    double qw = aw * bw - ax * bx - ay * by - az * bz;
    if (qw < 0.0) { qx = -qx; qy = -qy; qz = -qz; qw = -qw; }
    const double vn = sqrt(qx * qx + qy * qy + qz * qz);
    const double k = vn > 1e-8 * qw ? 2.0 * atan2(vn, qw) / vn : 2.0 / qw;
    Y[0][NX] = k * qx; Y[1][NX] = k * qy; Y[2][NX] = k * qz;
    // u = we - DR^T ws
    double R[9], ws[3], we[3];
    quat_mat(a, R);
    ld_vec(rate_start + 3 * s, ws);
    ld_vec(rate_end + 3 * s, we);
#pragma unroll
    for (int c = 0; c < 3; ++c) Y[c][3] = we[c] - (R[c] * ws[0] + R[3 + c] * ws[1] + R[6 + c] * ws[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Y[r][c] = jac ? jac[54 * s + 6 * r + c] : 0.0;
    double fin = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < NX + 1; ++c) fin += fabs(Y[r][c]);
    return isfinite(fin);
}

// |e - Y x|
__device__ __forceinline__ double residual_norm(const double (&Y)[3][NX + 1], const double* __restrict__ x) {
    const double x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3];
    double n2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double v = Y[r][NX] - (Y[r][0] * x0 + Y[r][1] * x1 + Y[r][2] * x2 + Y[r][3] * x3);
        n2 += v * v;
    }
    return sqrt(n2);
}

// One lane per row.  xhat: the previous round's x, NULL in round 0 (rho = 1).
template <class T>
__global__ __launch_bounds__(BLOCK) void td_row_kernel(const double* __restrict__ jac, const T* __restrict__ rot_imu,
                                                       const T* __restrict__ rot_ref, const T* __restrict__ rate_start,
                                                       const T* __restrict__ rate_end, const double* __restrict__ weight, int rows,
                                                       double delta, const double* __restrict__ xhat, double* __restrict__ terms) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= rows) return;
    const size_t s = (size_t)i;
    double t[NT<NX>];
#pragma unroll
    for (int q = 0; q < NT<NX>; ++q) t[q] = 0.0;
    const double w = weight ? weight[s] : 1.0;
    if (w != 0.0) {                                       // a row of weight zero takes no part, whatever its data holds
        double Y[3][NX + 1];
        bool ok = row_system(jac, rot_imu, rot_ref, rate_start, rate_end, s, Y);
        ok = ok && isfinite(w) && w > 0.0;
        double wr = w;
        if (xhat && ok) wr = w * fmin(1.0, delta / residual_norm(Y, xhat));   // (a residual of 0: delta / 0 = inf, rho = 1)
        normal_terms<NX>(Y, wr, ok, t);
    }
#pragma unroll
    for (int q = 0; q < NT<NX>; ++q) terms[(size_t)q * rows + s] = t[q];
}

__global__ __launch_bounds__(BLOCK) void td_partial_kernel(const double* __restrict__ terms, int rows, int nblocks, double* __restrict__ partial) {
    partial_sum<NT<NX>>(terms, rows, nblocks, partial);
}

// the compacted system of the n unknowns that are solved, row stride NX
struct SolveLds {
    double H[NX * NX], c[NX], L[NX * NX], x[NX];
    int at[NX];                       // the place of compact unknown a in the layout of four
};

// One workgroup: the fixed-order sum of `count` term vectors (src[q ld + c]), then the solve on lane 0.  x goes to xhat (scratch) for the
// next round, and with `last` to out_x / out_H.  A round that fails leaves the call failed (`first`: there is no earlier round to read).
__global__ __launch_bounds__(BLOCK) void td_solve_kernel(const double* __restrict__ src, int ld, int count, int solve_bias, int first, int last,
                                                         int* __restrict__ status, double* __restrict__ xhat, double* __restrict__ out_x,
                                                         double* __restrict__ out_H) {
    __shared__ double wsum[4 * NT<NX>], tot[NT<NX>];
    __shared__ SolveLds S;
    block_sum<NT<NX>>(src, (size_t)ld, 0, (size_t)count, wsum, tot);
    if (threadIdx.x != 0) return;
    int at[NX];
    const int n = list_solved<NX>([=](int a) { return a == NX - 1 || solve_bias != 0; }, S.at, at);
    gather_solved<NX>(tot, at, S.H, S.c);
    bool pd = chol_solve<NX>(S.H, S.c, n, S.L, S.x);
    if (!first && status[0] != 0) pd = false;
    for (int a = 0; a < NX; ++a) xhat[a] = 0.0;
    if (pd) scatter_solved<NX>(S.x, at, n, xhat);
    if (last) {
        for (int a = 0; a < NX; ++a) out_x[a] = xhat[a];
        if (out_H) write_full_H<NX>(tot, out_H);
    }
    status[0] = pd ? 0 : 1;
    status[1] = (int)tot[NT<NX> - 1];
}

// One lane per row: |e_i - Y_i x| under the final x, NaN for a row with non-finite data; zeros when the solve failed.
template <class T>
__global__ __launch_bounds__(BLOCK) void td_res_kernel(const double* __restrict__ jac, const T* __restrict__ rot_imu,
                                                       const T* __restrict__ rot_ref, const T* __restrict__ rate_start,
                                                       const T* __restrict__ rate_end, int rows, const double* __restrict__ xhat,
                                                       const int* __restrict__ status, double* __restrict__ out_res) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= rows) return;
    const size_t s = (size_t)i;
    double r = 0.0;
    if (status[0] == 0) {
        double Y[3][NX + 1];
        const bool ok = row_system(jac, rot_imu, rot_ref, rate_start, rate_end, s, Y);
        r = ok ? residual_norm(Y, xhat) : nan("");
    }
    out_res[s] = r;
}

// One lane per row: Exp(-ws tau) (x) rot (x) Exp(we tau), renormalised.  Everything is read before anything is written: out may be rot.
template <class T>
__global__ __launch_bounds__(BLOCK) void td_shift_kernel(const T* rot, const T* __restrict__ rate_start, const T* __restrict__ rate_end, int rows,
                                                         double tau, T* out_rot) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= rows) return;
    const size_t s = (size_t)i;
    const Q4<double> q{(double)rot[4 * s], (double)rot[4 * s + 1], (double)rot[4 * s + 2], (double)rot[4 * s + 3]};
    const V3<double> ws{(double)rate_start[3 * s], (double)rate_start[3 * s + 1], (double)rate_start[3 * s + 2]};
    const V3<double> we{(double)rate_end[3 * s], (double)rate_end[3 * s + 1], (double)rate_end[3 * s + 2]};
    const Q4<double> o = qmul(qmul(so3_exp(-tau * ws), q), so3_exp(tau * we));
    const double n = 1.0 / sqrt(o.x * o.x + o.y * o.y + o.z * o.z + o.w * o.w);
    out_rot[4 * s] = (T)(o.x * n); out_rot[4 * s + 1] = (T)(o.y * n); out_rot[4 * s + 2] = (T)(o.z * n); out_rot[4 * s + 3] = (T)(o.w * n);
}

template <class T>
int run(const double* jac, const void* rot_imu_v, const void* rot_ref_v, const void* rate_start_v, const void* rate_end_v, const double* weight,
        int rows, int solve_bias, double delta, int rounds, double* out_x, double* out_H, double* out_res, void* scratch, hipStream_t s) {
    const T *rot_imu = (const T*)rot_imu_v, *rot_ref = (const T*)rot_ref_v, *rate_start = (const T*)rate_start_v, *rate_end = (const T*)rate_end_v;
    const Scratch sc(scratch, NT<NX>, rows);
    const dim3 grid((rows + BLOCK - 1) / BLOCK);
    return run_rounds(
        sc, rows, td_partial_kernel, delta, rounds, s,
        [&](const double* xhat) {
            hipLaunchKernelGGL(td_row_kernel<T>, grid, dim3(BLOCK), 0, s, jac, rot_imu, rot_ref, rate_start, rate_end, weight, rows, delta, xhat,
                               sc.terms);
        },
        [&](int first, int last) {
            hipLaunchKernelGGL(td_solve_kernel, dim3(1), dim3(BLOCK), 0, s, sc.src, sc.count, sc.count, solve_bias, first, last, sc.status, sc.est,
                               out_x, out_H);
        },
        [&] {
            if (out_res && rows > 0)
                hipLaunchKernelGGL(td_res_kernel<T>, grid, dim3(BLOCK), 0, s, jac, rot_imu, rot_ref, rate_start, rate_end, rows,
                                   (const double*)sc.est, (const int*)sc.status, out_res);
        },
        [&](int excluded) {
            return fail(ISLAM_ENOTPD, "islam_imu_time_offset_solve: the normal matrix of %d rows (%d excluded) is not positive definite "
                                      "(the offset needs a changing angular rate)", rows, excluded);
        });
}

}  // namespace

extern "C" {

size_t islam_imu_time_offset_solve_scratch_bytes(int rows) {
    return Scratch::bytes(NT<NX>, rows > 0 ? rows : 0);
}

int islam_imu_time_offset_solve(const double* jac, const void* rot_imu, const void* rot_ref, const void* rate_start, const void* rate_end,
                                const double* weight, int rows, int solve_bias, double delta, int rounds, double* out_x, double* out_H,
                                double* out_res, void* scratch, int dtype, void* stream) {
    const char* name = "islam_imu_time_offset_solve";
    if (const int rc = check_entry(name, rows, dtype)) return rc;                     // solve_bias is reported before delta and rounds
    if (solve_bias != 0 && solve_bias != 1) return fail(ISLAM_EARG, "islam_imu_time_offset_solve: solve_bias=%d (0 or 1)", solve_bias);
    if (const int rc = check_entry(name, rows, dtype, delta, rounds)) return rc;
    if (!out_x || !scratch) return fail(ISLAM_EARG, "islam_imu_time_offset_solve: out_x / scratch is NULL");
    if (rows > 0 && (!rot_imu || !rot_ref || !rate_start || !rate_end))
        return fail(ISLAM_EARG, "islam_imu_time_offset_solve: rot_imu / rot_ref / rate_start / rate_end is NULL (rows=%d)", rows);
    if (rows > 0 && solve_bias == 1 && !jac) return fail(ISLAM_EARG, "islam_imu_time_offset_solve: jac is NULL with solve_bias=1 (rows=%d)", rows);
    const double* j = solve_bias ? jac : nullptr;         // without the bias the Jacobians are not read
    return (dtype == ISLAM_F64 ? run<double> : run<float>)(j, rot_imu, rot_ref, rate_start, rate_end, weight, rows, solve_bias, delta, rounds, out_x,
                                                           out_H, out_res, scratch, as_stream(stream));
}

int islam_imu_time_shift(const void* rot, const void* rate_start, const void* rate_end, int rows, double tau, void* out_rot, int dtype,
                         void* stream) {
    if (const int rc = check_entry("islam_imu_time_shift", rows, dtype)) return rc;
    if (!std::isfinite(tau)) return fail(ISLAM_EARG, "islam_imu_time_shift: tau %g", tau);
    if (rows > 0 && (!rot || !rate_start || !rate_end || !out_rot))
        return fail(ISLAM_EARG, "islam_imu_time_shift: rot / rate_start / rate_end / out_rot is NULL (rows=%d)", rows);
    if (rows == 0) return ISLAM_OK;
    hipStream_t s = as_stream(stream);
    const dim3 grid((rows + BLOCK - 1) / BLOCK);
    if (dtype == ISLAM_F64)
        hipLaunchKernelGGL(td_shift_kernel<double>, grid, dim3(BLOCK), 0, s, (const double*)rot, (const double*)rate_start, (const double*)rate_end,
                           rows, tau, (double*)out_rot);
    else
        hipLaunchKernelGGL(td_shift_kernel<float>, grid, dim3(BLOCK), 0, s, (const float*)rot, (const float*)rate_start, (const float*)rate_end, rows,
                           tau, (float*)out_rot);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

}  // extern "C"
