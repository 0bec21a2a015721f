// The normal-equation terms of the closed-form IMU solves that are linear in NX unknowns (DESIGN.md sections 3.13 and 3.15: imu_align.hip
// at NX = 6 and 10; section 3.16: imu_time_offset.hip at NX = 4): what a pair kernel stores for imu_terms.h's sum and what lane 0 of the
// solve kernel reads back from the totals.  Device code only; every function is inlined where it is used.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace islam {
namespace normal {

// A pair (or row) is three equations Y = [the columns of the NX unknowns | right-hand side] (3 x (NX + 1)) of weight w; its terms are
// w Y^T Y:  H upper triangle by rows (NH) | c (NX) | excluded (0 or 1)
// The column of an unknown that is not solved is exact zeros; the solve kernel compacts the others before it factorises.
template <int NX>
constexpr int NH = NX * (NX + 1) / 2;
template <int NX>
constexpr int NT = NH<NX> + NX + 1;

// where H_ab (a <= b) sits among the terms
template <int NX>
__device__ __forceinline__ int tri(int a, int b) { return a * NX - a * (a - 1) / 2 + (b - a); }

// The terms of the system Y.  A system that is not ok, or has a term that is not finite, is excluded and counted: zeros and a one.
template <int NX>
__device__ __forceinline__ void normal_terms(const double (&Y)[3][NX + 1], double w, bool ok, double (&t)[NT<NX>]) {
    double tf = 0.0;
#pragma unroll
    for (int a = 0; a < NX; ++a)
#pragma unroll
        for (int b = a; b < NX + 1; ++b) {
            const double v = w * (Y[0][a] * Y[0][b] + Y[1][a] * Y[1][b] + Y[2][a] * Y[2][b]);
            tf += fabs(v);
            t[b < NX ? tri<NX>(a, b) : NH<NX> + a] = v;
        }
    t[NT<NX> - 1] = 0.0;
    if (!(ok && isfinite(tf))) {
#pragma unroll
        for (int q = 0; q < NT<NX> - 1; ++q) t[q] = 0.0;
        t[NT<NX> - 1] = 1.0;
    }
}

// Lane 0 of a solve kernel: the list of the n unknowns that are solved (on(a) says whether unknown a is), p[a] = the place of compact
// unknown a among the NX.  The list is built in LDS (NX ints: it is indexed by n), filled up to NX entries with NX - 1, a valid place, so
// that the gather below does not depend on n, and read into registers.  Returns n.
template <int NX, class On>
__device__ __forceinline__ int list_solved(On on, int* at, int (&p)[NX]) {
    int n = 0;
    for (int a = 0; a < NX; ++a)
        if (on(a)) at[n++] = a;
    for (int a = n; a < NX; ++a) at[a] = NX - 1;
#pragma unroll
    for (int a = 0; a < NX; ++a) p[a] = at[a];
    return n;
}

// The compact (H, c), row stride NX, of the unknowns that are solved, from the totals.  Unrolled and free of branches, so the reads
// of the totals are in flight together; what lands in rows and columns n and beyond comes from the fill and is never read.
template <int NX>
__device__ __forceinline__ void gather_solved(const double* tot, const int (&p)[NX], double* H, double* c) {
#pragma unroll
    for (int a = 0; a < NX; ++a) {
#pragma unroll
        for (int b = a; b < NX; ++b) H[NX * a + b] = H[NX * b + a] = tot[tri<NX>(p[a], p[b])];
        c[a] = tot[NH<NX> + p[a]];
    }
}

// The solved unknowns back into the layout of NX.
template <int NX>
__device__ __forceinline__ void scatter_solved(const double* x, const int (&p)[NX], int n, double* out) {
#pragma unroll
    for (int a = 0; a < NX; ++a)
        if (a < n) out[p[a]] = x[a];
}

// The full symmetric H of all NX unknowns, zero rows and columns for those that are not solved.
template <int NX>
__device__ __forceinline__ void write_full_H(const double* tot, double* out_H) {
#pragma unroll
    for (int a = 0; a < NX; ++a)
#pragma unroll
        for (int b = a; b < NX; ++b) out_H[NX * a + b] = out_H[NX * b + a] = tot[tri<NX>(a, b)];
}

}  // namespace normal
}  // namespace islam
