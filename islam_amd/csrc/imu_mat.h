// The 3x3 helpers and the small Cholesky solve of the closed-form IMU solves (DESIGN.md sections 3.13 and 3.15: imu_align.hip at 6 and
// at 10 unknowns; section 3.16: imu_time_offset.hip).  Device code only; every function is inlined or instantiated where it is used.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace islam {
namespace imat {

constexpr double PIVOT_REL = 1e-13;   // islam_imu_gyro_bias_solve's rule: a pivot at or below this share of its diagonal entry fails

// rotation matrix (by rows) of a unit quaternion xyzw
template <class T>
__device__ __forceinline__ void quat_mat(const T* q, double (&R)[9]) {
    const double x = (double)q[0], y = (double)q[1], z = (double)q[2], w = (double)q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w); R[2] = 2.0 * (x * z + y * w);
    R[3] = 2.0 * (x * y + z * w); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
    R[6] = 2.0 * (x * z - y * w); R[7] = 2.0 * (y * z + x * w); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

template <class T>
__device__ __forceinline__ void ld_vec(const T* p, double (&v)[3]) { v[0] = (double)p[0]; v[1] = (double)p[1]; v[2] = (double)p[2]; }

__device__ __forceinline__ void mat_vec(const double (&R)[9], const double (&v)[3], double (&o)[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = R[3 * k] * v[0] + R[3 * k + 1] * v[1] + R[3 * k + 2] * v[2];
}

__device__ __forceinline__ void mat_mat(const double (&a)[9], const double (&b)[9], double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// o = a b^T
__device__ __forceinline__ void mat_matT(const double (&a)[9], const double (&b)[9], double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}

// the 3x3 block (r0.., c0..) of a row-major matrix with `ld` columns
__device__ __forceinline__ void ld_block(const double* m, int ld, int r0, int c0, double (&o)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = m[(r0 + i) * ld + c0 + j];
}

// M (n x n, row stride LD) = L L^T under the pivot rule, then L L^T x = rhs.  Every array lives in LDS.
template <int LD>
__device__ bool chol_solve(const double* M, const double* rhs, int n, double* L, double* x) {
    for (int j = 0; j < n; ++j) {
        double p = M[LD * j + j];
        for (int k = 0; k < j; ++k) p -= L[LD * j + k] * L[LD * j + k];
        if (!(p > PIVOT_REL * M[LD * j + j]) || !isfinite(p)) return false;
        const double l = sqrt(p);
        L[LD * j + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double v = M[LD * i + j];
            for (int k = 0; k < j; ++k) v -= L[LD * i + k] * L[LD * j + k];
            L[LD * i + j] = v / l;
        }
    }
    bool fin = true;
    for (int i = 0; i < n; ++i) {
        double v = rhs[i];
        for (int k = 0; k < i; ++k) v -= L[LD * i + k] * x[k];
        x[i] = v / L[LD * i + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double v = x[i];
        for (int k = i + 1; k < n; ++k) v -= L[LD * k + i] * x[k];
        x[i] = v / L[LD * i + i];
        fin = fin && isfinite(x[i]);
    }
    return fin;
}

}  // namespace imat
}  // namespace islam
