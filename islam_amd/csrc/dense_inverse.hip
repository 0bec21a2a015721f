// Inverse of the dense Cholesky factor, in place, and covariance blocks from it.  The definition is in
// include/islam_hip.h (islam_dense_chol_invert_factor / islam_pvgo_dense_cov_blocks).
//
// Storage: the array islam_dense_chol_factor left -- L in the lower triangle and the diagonal, the matrix's own entries in the strict
// upper triangle.  W = L^-1 replaces L; the strict upper triangle is never written and never read as data: every load whose column can
// exceed its row is predicated on col <= row and gives 0 otherwise.
//
// With L = [L11 0; L21 L22]:  L^-1 = [W11 0; -W22 L21 W11  W22].  Block columns of NB = 64.  Every diagonal block W_jj = L_jj^-1 depends on
// its own L_jj only: one launch inverts them all.  Then the block columns j = [c0, c1), DESCENDING, so that the trailing inverse
// W22 = W[c1:, c1:] is complete when block column j needs it, two launches each:
//   trinv_diag_kernel    (once, one workgroup per block) W_jj = L_jj^-1, one wave, row r in the registers of lane r, unblocked column sweep
//                        (descending), operands of the other rows by v_readlane
//   trinv_panel_kernel   T = -L[c1:, j] W_jj on v_mfma_f64_16x16x4_f64, computed and stored TRANSPOSED in the workspace (64 x n, the row index
//                        of L contiguous) so that the product below loads both operands as "row m, four consecutive k"
//   trinv_update_kernel  W[c1:, j] = tril(W[c1:, c1:]) T on the matrix cores, 128 rows per workgroup, 32 rows per wave.  The sum of a wave
//                        with first row rw runs over k in [c1, rw + 31]: the columns below rw in 16-column chunks as chol_update_kernel
//                        loads them (rw - c1 is a multiple of 32), then the two chunks [rw, rw + 32) that straddle the diagonal of W with
//                        predicated loads (col <= row, and k < n for T).
// The last block column has nothing below it: 2 ceil(n / 64) - 1 launches.  Dependencies are the launch boundaries: no atomic, no
// hand-off, no loop whose trip count depends on data; a NaN in the factor propagates and every launch terminates.
//
// Fragment map and operand loads: see csrc/dense_tile.h (A[m][k = q], B[k = q][n = m], C/D register i: row = q + 4 i, col = m).
//
// Covariance blocks: Sigma = A^-1 = W^T W, so block (a, b) is sum_{i >= 9 max(a, b)} W[i, 9a : 9a+9]^T W[i, 9b : 9b+9] over the lower
// triangle.  One workgroup of 256 per block, rows strided over the threads, 81 sums per thread, then a butterfly over the wave and the
// four waves added in a fixed order.  Block (b, a) forms the same products in the same order: it is the transpose of (a, b) to the bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dense_tile.h"

using namespace islam;
using namespace islam::tile;

namespace {

constexpr int WIDE = 8192;       // rows below a block column above which its update takes 32 columns per workgroup instead of 16
constexpr int CB = 384;          // pairs per launch of cov_pair_kernel (passed by value: 3 KB of kernel arguments)

// One wave: the diagonal block L_jj (lower triangle, jb = min(64, n - c0) rows) -> W_jj = L_jj^-1 in place, row r in the registers of
// lane r.  Column c, descending: w_cc = 1 / l_cc, w_rc = -(sum_{k = c+1..r} w_rk l_kc) / l_cc; column c of L is still in place in every
// lane when it is read (it is overwritten at the end of its own step), the columns right of it already hold W.
__global__ __launch_bounds__(64) void trinv_diag_kernel(double* __restrict__ A, int n) {
    const int r = threadIdx.x;
    const int c0 = blockIdx.x * NB;
    const int jb = min(NB, n - c0);
    double* p = A + (size_t)(c0 + min(r, jb - 1)) * (size_t)n + c0;
    double x[NB];
    load_diag_row(p, jb, r, x);
#pragma unroll
    for (int c = NB - 1; c >= 0; --c) {
        if (c < jb) {                                      // (uniform)
            const double d = lane_bcast(x[c], c);
            double s = 0.0;
#pragma unroll
            for (int k = c + 1; k < NB; ++k) s += x[k] * lane_bcast(x[c], k);    // w_rk l_kc (w_rk = 0 for k > r)
            x[c] = r == c ? 1.0 / d : r > c ? -s / d : 0.0;
        }
    }
    store_diag_row(p, jb, r, x);
}

// T = -L[c1:, c0:c1] W_jj for the rows r >= c1 = c0 + 64 (the block is full there), computed transposed on the matrix cores as it is stored:
// Tt (64 x rows) = -W_jj^T L[c1:, c0:c1]^T.  A operand W_jj^T[c][k] = w_kc (one predicated load per element: c <= k, else 0), B operand
// L[r][k] as "row m, four consecutive k".  A wave takes all 64 columns c (four groups of 16) of 32 rows; a 16-column chunk of k lies wholly
// above the column groups right of it (w_kc = 0 for k < c), which skip it.  Tt[c * ldt + (r - c1)]: 16 lanes store 128 contiguous bytes.
__global__ __launch_bounds__(256) void trinv_panel_kernel(const double* __restrict__ A, int n, int c0, double* __restrict__ Tt, int ldt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int c1 = c0 + NB, below = n - c1;
    const int r0 = blockIdx.x * TM + wave * 32;           // first row of this wave, counted from c1
    if (r0 >= below) return;                               // (wave-uniform; no barrier in this kernel)
    const size_t ld = (size_t)n;
    const double* pw = A + (size_t)c0 * ld + c0;           // W_jj
    const double* pl[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) pl[b] = operand_row(A, n, c1 + r0 + 16 * b + m, c0, q);
    d4 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        d4 fb[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) fb[b] = ld4(pl[b] + 16 * ch);
#pragma unroll
        for (int a = 0; a <= ch; ++a) {
            d4 fa;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int k = 16 * ch + 4 * q + kk, c = 16 * a + m;
                fa[kk] = c <= k ? pw[(size_t)k * ld + c] : 0.0;
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[kk], fb[b][kk], acc[a][b], 0, 0, 0);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 16 * a + q + 4 * i, r = r0 + 16 * b + m;
                if (r < below) Tt[(size_t)c * ldt + r] = -acc[a][b][i];
            }
}

// W[c1 + 128 bx .., c0 + 16 NC by : + 16 NC] = tril(W[.., c1:]) T, T from Tt (64 x ldt, k - c1 contiguous).  c1 = c0 + 64 <= n - 1.  NC: the
// 16-column groups of one workgroup; 4 / NC workgroups share a 128-row tile, each with a chain of 8 NC MFMAs per 16-column chunk.
template <int NC, int D>
__global__ __launch_bounds__(256, 2) void trinv_update_kernel(double* __restrict__ A, int n, int c0, const double* __restrict__ Tt, int ldt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int c1 = c0 + NB;
    const int rw = c1 + blockIdx.x * TM + wave * 32;      // first row of this wave
    if (rw >= n) return;                                   // (wave-uniform; no barrier in this kernel)
    const size_t ld = (size_t)n;
    int ra[2];                                             // (clamped like the operand rows: what the straddling chunks compare k with)
    const double* pa[2];
    const double* pb[NC];
    const int cg = blockIdx.y * NC;                        // first 16-column group of this workgroup
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        ra[a] = min(rw + 16 * a + m, n - 1);
        pa[a] = operand_row(A, n, ra[a], c1, q);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) pb[c] = Tt + (size_t)(16 * (cg + c) + m) * ldt + 4 * q;
    d4 acc[2][NC];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
    // columns k in [c1, rw): below every row of this wave, so wholly inside the lower triangle; rw - c1 is a multiple of 32.  A ring of D
    // register sets: the loads of chunk i + D go out when chunk i has fed the matrix core, so D - 1 chunks of MFMAs cover the latency of a
    // load (a chunk is only 8 NC MFMAs here).
    const MfmaChunk<NC> chunk{acc};
    d4 fa[D][2], fb[D][NC];
    const int nch = (rw - c1) / 16;
    auto load = [&](int d, int i) {                        // chunk min(i, nch - 1): the last sets reload the last chunk instead of reading past rw
        const int k = 16 * (i < nch ? i : nch - 1);
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[d][a] = ld4(pa[a] + k);
#pragma unroll
        for (int c = 0; c < NC; ++c) fb[d][c] = ld4(pb[c] + k);
    };
    if (nch > 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) load(d, d);
    }
    for (int i0 = 0; i0 < nch; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (i0 + d < nch) {                            // (uniform)
                chunk(fa[d], fb[d]);
                load(d, i0 + d + D);
            }
        }
    }
    const int klen = rw - c1;
    d4 sa[2], sb[NC];
    // columns k in [rw, rw + 32): the tile that straddles the diagonal of W.  W[row][k] only where k <= row (the strict upper triangle holds the
    // matrix and is not read), T only where k < n; 0 otherwise.
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int kb = rw + 16 * h + 4 * q;               // first of this lane's four columns
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e) sa[a][e] = kb + e <= ra[a] ? pa[a][klen + 16 * h + e] : 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) sb[c][e] = kb + e < n ? pb[c][klen + 16 * h + e] : 0.0;
        chunk(sa, sb);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rw + 16 * a + q + 4 * i, col = c0 + 16 * (cg + c) + m;      // col < c1 <= row
                if (row < n) A[(size_t)row * ld + col] = acc[a][c][i];
            }
}

struct PairBatch {
    int a[CB], b[CB];
};

// out (9 x 9) = sum_{i >= 9 max(a, b)} W[i, 9a..]^T W[i, 9b..] over the lower triangle; the pose rows of a == anchor and the pose columns of
// b == anchor are written as zero.
__device__ __forceinline__ void cov_block(const double* __restrict__ W, int n, int a, int b, int anchor, double* __restrict__ out) {
    __shared__ double red[4][81];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ca = 9 * a, cb = 9 * b;
    double acc[9][9];
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int q = 0; q < 9; ++q) acc[p][q] = 0.0;
    for (int i = 9 * max(a, b) + t; i < n; i += 256) {    // (trip count: a function of n, a, b only)
        const double* row = W + (size_t)i * (size_t)n;
        double u[9], v[9];
#pragma unroll
        for (int p = 0; p < 9; ++p) {
            u[p] = ca + p <= i ? row[ca + p] : 0.0;
            v[p] = cb + p <= i ? row[cb + p] : 0.0;
        }
#pragma unroll
        for (int p = 0; p < 9; ++p)
#pragma unroll
            for (int q = 0; q < 9; ++q) acc[p][q] = fma(u[p], v[q], acc[p][q]);
    }
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            double s = acc[p][q];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
            if (lane == 0) red[wave][9 * p + q] = s;
        }
    __syncthreads();
    if (t < 81) {
        const int p = t / 9, q = t % 9;
        const bool fixed = (a == anchor && p < 6) || (b == anchor && q < 6);
        out[t] = fixed ? 0.0 : (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
}

__global__ __launch_bounds__(256) void cov_node_kernel(const double* __restrict__ W, int n, int anchor, double* __restrict__ node_cov) {
    cov_block(W, n, blockIdx.x, blockIdx.x, anchor, node_cov + (size_t)blockIdx.x * 81);
}

__global__ __launch_bounds__(256) void cov_pair_kernel(const double* __restrict__ W, int n, int anchor, PairBatch pb, double* __restrict__ pair_cov) {
    cov_block(W, n, pb.a[blockIdx.x], pb.b[blockIdx.x], anchor, pair_cov + (size_t)blockIdx.x * 81);
}

}  // namespace

extern "C" {

size_t islam_dense_chol_inverse_workspace_bytes(int n) {
    return n > 0 ? align_up((size_t)NB * (size_t)n * sizeof(double)) : 0;
}

int islam_dense_chol_invert_factor(double* L, int n, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_workspace_args(__func__, n, !L || !workspace, "L / workspace", workspace_bytes, islam_dense_chol_inverse_workspace_bytes(n)))
        return rc;
    hipStream_t s = as_stream(stream);
    double* Tt = (double*)workspace;
    const int nb = (n + NB - 1) / NB;
    hipLaunchKernelGGL(trinv_diag_kernel, dim3(nb), dim3(64), 0, s, L, n);     // every W_jj depends on its own L_jj only
    for (int j = nb - 2; j >= 0; --j) {
        const int c0 = j * NB, below = n - c0 - NB;
        hipLaunchKernelGGL(trinv_panel_kernel, dim3((below + TM - 1) / TM), dim3(256), 0, s, L, n, c0, Tt, n);
        // 16 columns per workgroup keep the dependent MFMA chain of a wave short (8 per chunk) while the launch has few workgroups; with many,
        // the operand traffic through the caches counts and 32 columns per workgroup halve the re-reads of W (measured: DESIGN.md 3.18).
        // The order of every sum is the same in both.
        if (below > WIDE)
            hipLaunchKernelGGL((trinv_update_kernel<2, 4>), dim3((below + TM - 1) / TM, 2), dim3(256), 0, s, L, n, c0, Tt, n);
        else
            hipLaunchKernelGGL((trinv_update_kernel<1, 4>), dim3((below + TM - 1) / TM, 4), dim3(256), 0, s, L, n, c0, Tt, n);
    }
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_dense_cov_blocks(const double* W, int n, int anchor, const int64_t* pairs, int P, double* node_cov, double* pair_cov,
                                void* stream) {
    if (n < 1 || n % 9 != 0) return fail(ISLAM_EARG, "islam_pvgo_dense_cov_blocks: n=%d is not a positive multiple of 9", n);
    if (!W) return fail(ISLAM_EARG, "islam_pvgo_dense_cov_blocks: W is NULL");
    const int N = n / 9;
    if (anchor < -1 || anchor >= N) return fail(ISLAM_EARG, "islam_pvgo_dense_cov_blocks: anchor=%d, N=%d", anchor, N);
    if (P < 0 || (P > 0 && !pairs)) return fail(ISLAM_EARG, "islam_pvgo_dense_cov_blocks: P=%d, pairs=%p", P, (const void*)pairs);
    for (int p = 0; p < P; ++p)
        if (pairs[2 * p] < 0 || pairs[2 * p] >= N || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= N)
            return fail(ISLAM_EARG, "islam_pvgo_dense_cov_blocks: pair %d = (%lld, %lld), N=%d", p, (long long)pairs[2 * p],
                        (long long)pairs[2 * p + 1], N);
    hipStream_t s = as_stream(stream);
    if (node_cov) hipLaunchKernelGGL(cov_node_kernel, dim3(N), dim3(256), 0, s, W, n, anchor, node_cov);
    if (pair_cov) {
        PairBatch pb;
        for (int base = 0; base < P; base += CB) {
            const int cnt = P - base < CB ? P - base : CB;
            for (int p = 0; p < CB; ++p) {
                pb.a[p] = p < cnt ? (int)pairs[2 * (base + p)] : 0;
                pb.b[p] = p < cnt ? (int)pairs[2 * (base + p) + 1] : 0;
            }
            hipLaunchKernelGGL(cov_pair_kernel, dim3(cnt), dim3(256), 0, s, W, n, anchor, pb, pair_cov + (size_t)base * 81);
        }
    }
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

}  // extern "C"
