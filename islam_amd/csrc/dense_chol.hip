// Dense fp64 Cholesky A = L L^T and the two triangular solves for the general-topology PVGO normal matrix (n = 9N, never a multiple of
// 16 in general) on gfx950.  The definition is in include/islam_hip.h (islam_dense_chol_factor / _solve).
//
// Storage: A is row-major n x n.  The factorisation READS the strict upper triangle and diag[n] and WRITES L into the lower triangle
// and the diagonal of the same array; the strict upper triangle and diag are never written, so a retry with another diag (the LM's
// growing damping) needs no restoration and no second matrix.
//
// Left-looking by block columns of NB = 64.  For block column j (columns c0 = 64 j .. c0 + 63), three launches:
//   chol_update_kernel   S_ij = A_ij - sum_{k < c0} L_ik L_jk^T for every row at or below the block, 128 rows x 64 columns per workgroup,
//                        the sum over ALL previous columns accumulated in registers by v_mfma_f64_16x16x4_f64 and the tile written once
//                        (n^2 / 2 doubles written in total; a right-looking schedule would rewrite the trailing matrix n / 64 times)
//   chol_diag_kernel     one workgroup: S_jj -> L_jj in LDS (right-looking inside the 64 x 64 block), the pivot test, info
//   chol_panel_kernel    L_ij = S_ij L_jj^-T for the rows below the block by substitution, one lane per row, L_jj broadcast from LDS
// The last block column has no panel: 3 ceil(n / 64) - 1 launches.  Dependencies are the launch boundaries; there is no atomic, no
// hand-off and no data-dependent loop, so a second call gives the same bits and a failed pivot (NaN below it) cannot hang anything.
//
// Pivot rule: the pivot of column c is d = a_cc - sum_k l_ck^2 as computed; d <= 0 or d not finite fails, and info receives c + 1 for the
// FIRST such column (LAPACK's potrf numbering), 0 when there is none.  After a failure the remaining launches run on whatever the
// square root of that pivot gave; what they leave in the lower triangle is unspecified.
//
// Fragment map and operand loads of the update (L_i times L_j^T): see csrc/dense_tile.h.
//
// Solves (one right-hand side): w = b; for each block j ascending one launch of chol_fwd_kernel: every workgroup solves L_jj y_j = w_j
// itself (64 x 64, one wave by column substitution), workgroup 0 stores y_j, every workgroup subtracts L_ij y_j from its 64 rows below.
// Then descending chol_bwd_kernel: L_jj^T x_j = y_j, workgroup 0 stores x_j, every workgroup subtracts L_j,c^T x_j from its 256 columns
// left of the block.  The vector a launch reads at block j is never written by that launch (results go to another array), so there is
// no race between workgroups.  2 ceil(n / 64) launches and one device-to-device copy of b.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dense_tile.h"

using namespace islam;
using namespace islam::tile;

namespace {

constexpr int NW = 512;          // wide block column of the two-level update (a multiple of NB)
constexpr int LDP = NB + 1;      // padded LDS row (doubles): lanes that walk down a column hit different banks

// S <- S0 - L_i L_j^T over the columns [kbeg, kend) of L, for rows [cfirst + 128 bx, + 128) x columns [c0, c0 + 64), c0 = cfirst + 64 by,
// written to the lower triangle (col <= row only).  from_upper: S0 is A (its upper triangle transposed, diag on the diagonal), otherwise
// the tile's own present content (the second level of the blocking).  kbeg, kend, cfirst: multiples of 64, kend <= cfirst.
__global__ __launch_bounds__(256, 2) void chol_update_kernel(double* __restrict__ A, const double* __restrict__ diag, int n, int cfirst, int kbeg,
                                                          int kend, int from_upper) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int c0 = cfirst + blockIdx.y * NB;
    const int rw = cfirst + blockIdx.x * TM + wave * 32;  // first row of this wave
    if (rw >= n || rw + 31 < c0) return;                   // past the end, or wholly above the diagonal (wave-uniform; no barrier here)
    const size_t ld = (size_t)n;
    const double* pa[2];
    const double* pb[4];
#pragma unroll
    for (int a = 0; a < 2; ++a) pa[a] = operand_row(A, n, rw + 16 * a + m, kbeg, q);
#pragma unroll
    for (int c = 0; c < 4; ++c) pb[c] = operand_row(A, n, c0 + 16 * c + m, kbeg, q);
    d4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = d4{0.0, 0.0, 0.0, 0.0};
    // columns k < kend <= cfirst <= every row read here: the part of the lower triangle the earlier block columns wrote.  kend - kbeg is a
    // multiple of 64, so the 16-column chunks come in pairs: two register sets, each loaded while the other feeds the matrix core.
    const MfmaChunk<4> chunk{acc};
    d4 fa[2], fb[4], ga[2], gb[4];
    const int klen = kend - kbeg;
    if (klen > 0) {
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[a] = ld4(pa[a]);
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[c] = ld4(pb[c]);
    }
    for (int k0 = 0; k0 < klen; k0 += 32) {
#pragma unroll
        for (int a = 0; a < 2; ++a) ga[a] = ld4(pa[a] + k0 + 16);
#pragma unroll
        for (int c = 0; c < 4; ++c) gb[c] = ld4(pb[c] + k0 + 16);
        chunk(fa, fb);
        const int kn = k0 + 32 < klen ? k0 + 32 : k0;     // the last pair reloads its own first chunk instead of reading past column kend
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[a] = ld4(pa[a] + kn);
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[c] = ld4(pb[c] + kn);
        chunk(ga, gb);
    }
    // S = S0 - acc where col <= row < n.  from_upper: S0 comes from the upper triangle, transposed (diag on the diagonal).  An element that
    // is not stored loads diag[0] instead, so that the 32 loads of a lane go out together.
    double av[2][4][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rw + 16 * a + q + 4 * i, col = c0 + 16 * c + m;
                const bool in = row < n && col <= row;
                const double* src = !in ? diag : !from_upper ? A + (size_t)row * ld + col : col < row ? A + (size_t)col * ld + row : diag + row;
                av[a][c][i] = *src;
            }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rw + 16 * a + q + 4 * i, col = c0 + 16 * c + m;
                if (row < n && col <= row) A[(size_t)row * ld + col] = av[a][c][i] - acc[a][c][i];
            }
}

// One wave: the diagonal block S_jj (lower triangle, jb = min(64, n - c0) rows) -> L_jj, right-looking, row r in the registers of lane r
// (the entries right of the diagonal are carried along and never used).  info: set to 0 by the first block column, then to the 1-based
// index of the first failing pivot.
__global__ __launch_bounds__(64) void chol_diag_kernel(double* __restrict__ A, int n, int c0, int* __restrict__ info) {
    const int r = threadIdx.x;
    const int jb = min(NB, n - c0);
    double* p = A + (size_t)(c0 + min(r, jb - 1)) * (size_t)n + c0;
    double x[NB];
    load_diag_row(p, jb, r, x);
    int bad = 0;
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        if (c < jb) {                                      // (uniform)
            const double d = lane_bcast(x[c], c);
            if (bad == 0 && !(d > 0.0 && isfinite(d))) bad = c0 + c + 1;
            const double piv = sqrt(d);
            const double l = r == c ? piv : x[c] / piv;
            x[c] = l;
#pragma unroll
            for (int k = c + 1; k < NB; ++k) x[k] -= l * lane_bcast(l, k);       // l_rc l_kc
        }
    }
    store_diag_row(p, jb, r, x);
    if (r == 0) {
        const int prev = c0 == 0 ? 0 : info[0];
        info[0] = prev != 0 ? prev : bad;
    }
}

// L_ij = S_ij L_jj^-T for rows r >= c0 + 64 (the block is full there): x_c = (s_c - sum_{k<c} x_k L_jj[c][k]) / L_jj[c][c], one lane per row,
// the sum in four interleaved parts (four short dependent chains instead of one long one).
__global__ __launch_bounds__(64) void chol_panel_kernel(double* __restrict__ A, int n, int c0) {
    __shared__ double Ljj[NB * NB];
    const int t = threadIdx.x;
    const size_t ld = (size_t)n;
    for (int e = t; e < NB * NB; e += 64) {
        const int rr = e >> 6, cc = e & 63;
        Ljj[e] = cc <= rr ? A[(size_t)(c0 + rr) * ld + c0 + cc] : 0.0;
    }
    __syncthreads();
    const int row = c0 + NB + blockIdx.x * 64 + t;
    if (row >= n) return;
    double* p = A + (size_t)row * ld + c0;
    double x[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) x[c] = p[c];
#pragma unroll
    for (int c = 0; c < NB; ++c) {
        double s[4] = {x[c], 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < c; ++k) s[k & 3] -= x[k] * Ljj[c * NB + k];
        x[c] = ((s[0] + s[1]) + (s[2] + s[3])) / Ljj[c * NB + c];
    }
#pragma unroll
    for (int c = 0; c < NB; ++c) p[c] = x[c];
}

// The 64 x 64 diagonal block of L (rows / columns c0 .. c0 + jb - 1) into LDS, lower triangle; wave 0 then solves with it.
__device__ __forceinline__ void load_diag_block(const double* __restrict__ L, size_t ld, int c0, int jb, double* S) {
    for (int e = threadIdx.x; e < NB * NB; e += blockDim.x) {
        const int rr = e >> 6, cc = e & 63;
        if (rr < jb && cc <= rr) S[rr * LDP + cc] = L[(size_t)(c0 + rr) * ld + c0 + cc];
    }
}

// Forward step of block j: y_j = L_jj^-1 w_j (every workgroup, wave 0), y[c0..] = y_j (workgroup 0), w_i -= L_ij y_j for this workgroup's
// 64 rows below the block.  w at block j is only read here.
__global__ __launch_bounds__(256) void chol_fwd_kernel(const double* __restrict__ L, int n, int c0, double* __restrict__ w, double* __restrict__ y) {
    __shared__ double S[NB * LDP];
    __shared__ double ys[NB];
    const int t = threadIdx.x;
    const int jb = min(NB, n - c0);
    const size_t ld = (size_t)n;
    load_diag_block(L, ld, c0, jb, S);
    __syncthreads();
    if (t < 64) {
        double v = t < jb ? w[c0 + t] : 0.0;
        double out = 0.0;
        for (int c = 0; c < jb; ++c) {
            const double yc = __shfl(v, c) / S[c * LDP + c];
            if (t == c) out = yc;
            if (t > c && t < jb) v -= S[t * LDP + c] * yc;
        }
        ys[t] = out;
        if (blockIdx.x == 0 && t < jb) y[c0 + t] = out;
    }
    __syncthreads();
    // rows below the block (jb == 64 whenever there are any): 4 lanes per row, 16 columns each, combined in a fixed order
    const int row = c0 + NB + blockIdx.x * 64 + (t >> 2), part = t & 3;
    double s = 0.0;
    if (row < n) {
        const double* p = L + (size_t)row * ld + c0 + 16 * part;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += p[k] * ys[16 * part + k];
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (row < n && part == 0) w[row] -= s;
}

// Backward step of block j: x_j = L_jj^-T v_j (every workgroup, wave 0), x[c0..] = x_j (workgroup 0), v_c -= sum_r L[c0 + r][c] x_j[r] for
// this workgroup's 256 columns left of the block.  v at block j is only read here.
__global__ __launch_bounds__(256) void chol_bwd_kernel(const double* __restrict__ L, int n, int c0, double* __restrict__ v, double* __restrict__ x) {
    __shared__ double S[NB * LDP];
    __shared__ double xs[NB];
    const int t = threadIdx.x;
    const int jb = min(NB, n - c0);
    const size_t ld = (size_t)n;
    load_diag_block(L, ld, c0, jb, S);
    __syncthreads();
    if (t < 64) {
        double u = t < jb ? v[c0 + t] : 0.0;
        double out = 0.0;
        for (int c = jb - 1; c >= 0; --c) {
            const double xc = __shfl(u, c) / S[c * LDP + c];
            if (t == c) out = xc;
            if (t < c) u -= S[c * LDP + t] * xc;
        }
        xs[t] = out;
        if (blockIdx.x == 0 && t < jb) x[c0 + t] = out;
    }
    __syncthreads();
    const int col = blockIdx.x * 256 + t;
    if (col >= c0) return;
    const double* p = L + (size_t)c0 * ld + col;
    double s = 0.0;
    for (int r = 0; r < jb; ++r) s += p[(size_t)r * ld] * xs[r];
    v[col] -= s;
}

}  // namespace

extern "C" {

size_t islam_dense_chol_workspace_bytes(int n) {
    return n > 0 ? align_up(2 * (size_t)n * sizeof(double)) : 0;
}

int islam_dense_chol_factor(double* A, const double* diag, int n, void* workspace, size_t workspace_bytes, int* info, void* stream) {
    if (int rc = check_workspace_args(__func__, n, !A || !diag || !workspace || !info, "A / diag / workspace / info", workspace_bytes,
                                      islam_dense_chol_workspace_bytes(n)))
        return rc;
    hipStream_t s = as_stream(stream);
    for (int C0 = 0; C0 < n; C0 += NW) {                  // wide block column [C0, C0 + we): everything left of it in one launch
        const int we = n - C0 < NW ? n - C0 : NW;
        if (C0 > 0)
            hipLaunchKernelGGL(chol_update_kernel, dim3((n - C0 + TM - 1) / TM, (we + NB - 1) / NB), dim3(256), 0, s, A, diag, n, C0, 0, C0, 1);
        for (int c0 = C0; c0 < C0 + we; c0 += NB) {       // its 64-wide block columns: what the wide block column itself contributes
            if (c0 > C0 || C0 == 0)
                hipLaunchKernelGGL(chol_update_kernel, dim3((n - c0 + TM - 1) / TM, 1), dim3(256), 0, s, A, diag, n, c0, C0, c0, C0 == 0 ? 1 : 0);
            hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(64), 0, s, A, n, c0, info);
            const int below = n - c0 - NB;
            if (below > 0) hipLaunchKernelGGL(chol_panel_kernel, dim3((below + 63) / 64), dim3(64), 0, s, A, n, c0);
        }
    }
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_dense_chol_solve(const double* L, int n, const double* b, double* x, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_workspace_args(__func__, n, !L || !b || !x || !workspace, "L / b / x / workspace", workspace_bytes,
                                      islam_dense_chol_workspace_bytes(n)))
        return rc;
    hipStream_t s = as_stream(stream);
    double* w = (double*)workspace;       // the running right-hand side of the forward sweep
    double* y = w + n;                    // its result, and the running right-hand side of the backward sweep
    ISLAM_HIP_CHECK(hipMemcpyAsync(w, b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    const int nb = (n + NB - 1) / NB;
    for (int j = 0; j < nb; ++j) {
        const int c0 = j * NB, below = n - c0 - NB;
        hipLaunchKernelGGL(chol_fwd_kernel, dim3(below > 0 ? (below + 63) / 64 : 1), dim3(256), 0, s, L, n, c0, w, y);
    }
    for (int j = nb - 1; j >= 0; --j) {
        const int c0 = j * NB;
        hipLaunchKernelGGL(chol_bwd_kernel, dim3(c0 > 0 ? (c0 + 255) / 256 : 1), dim3(256), 0, s, L, n, c0, y, x);
    }
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

}  // extern "C"
