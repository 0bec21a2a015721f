// What the dense fp64 Cholesky (dense_chol.hip) and the in-place inverse of its factor (dense_inverse.hip, section
// 3.18) share: the block sizes, the f64 MFMA fragments and their operand loads, a diagonal block in registers, the entry points' checks.
//
// f64 MFMA fragments (16 x 16 x 4, one double per lane per operand; NOT the f32 C/D map), q = lane >> 4, m = lane & 15:
//   A[m][k = q]   B[k = q][n = m]   C/D register i in [0, 4): row = q + 4 i, col = m
// Both update kernels compute X (rows x K) times Y^T, both row-major with K contiguous, so both operands are "row m, column k" loads.  A lane
// loads four consecutive doubles (columns k0 + 4 q .. + 3) of its row and MFMA number kk of the chunk takes element kk from both
// operands: it sums over k0 + 4 q + kk, q = 0..3, and the four MFMAs of a chunk cover its 16 columns (any pairing of k is a valid
// order for a sum).  The map was checked with exact small-integer data (tests/test_dense_chol_gpu.py does it on every run: an integer
// matrix whose factor is exact).
#pragma once
#include "common.h"

namespace islam::tile {

constexpr int NB = 64;           // block-column width
constexpr int TM = 128;          // rows of one update workgroup: 4 waves x 32 rows

typedef double d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ d4 ld4(const double* p) { return d4{p[0], p[1], p[2], p[3]}; }

// v of lane `lane` (wave-uniform) to every lane
__device__ __forceinline__ double lane_bcast(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// Where a lane's four operand doubles of a chunk start: row r of the row-major n x n array A, column k0 + 4 q.  A row past the end is
// clamped: it loads valid memory and its results are not stored.
__device__ __forceinline__ const double* operand_row(const double* A, int n, int r, int k0, int q) {
    return A + (size_t)min(r, n - 1) * (size_t)n + k0 + 4 * q;
}

// chunk(fa, fb): acc += fa fb^T over one 16-column chunk of k, 2 x NC tiles of 16 x 16, a chain of 4 MFMAs each.  An update kernel binds its
// accumulators once, `const MfmaChunk<NC> chunk{acc};` (by reference: with acc as a function argument the compiler schedules both differently).
template <int NC>
struct MfmaChunk {
    d4 (&acc)[2][NC];
    __device__ __forceinline__ void operator()(const d4 (&fa)[2], const d4 (&fb)[NC]) const {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a][kk], fb[c][kk], acc[a][c], 0, 0, 0);
    }
};

// One wave holds the lower triangle of a diagonal block (jb = min(64, n - c0) rows) with row r in the registers x[NB] of lane r, p = where
// that row starts (row min(r, jb - 1): valid memory).  The entries right of the diagonal and the rows past jb load as zero and are not stored.
__device__ __forceinline__ void load_diag_row(const double* p, int jb, int r, double (&x)[NB]) {
#pragma unroll
    for (int k = 0; k < NB; ++k) x[k] = (r < jb && k <= r) ? p[k] : 0.0;
}

__device__ __forceinline__ void store_diag_row(double* p, int jb, int r, const double (&x)[NB]) {
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if (r < jb && k <= r) p[k] = x[k];
}

// Host side, an entry point `fn` that takes a workspace: ISLAM_OK, or ISLAM_EARG with the message set (null: a required pointer, `names`, is).
inline int check_workspace_args(const char* fn, int n, bool null, const char* names, size_t workspace_bytes, size_t needed) {
    if (n < 1) return fail(ISLAM_EARG, "%s: n=%d", fn, n);
    if (null) return fail(ISLAM_EARG, "%s: %s is NULL", fn, names);
    if (workspace_bytes < needed) return fail(ISLAM_EARG, "%s: workspace of %zu bytes, n=%d needs %zu", fn, workspace_bytes, n, needed);
    return ISLAM_OK;
}

}  // namespace islam::tile
