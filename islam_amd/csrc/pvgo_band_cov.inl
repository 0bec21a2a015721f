// pvgo_band_cov.inl -- part of the pvgo.hip translation unit (textually included there; not compiled on its own).
// Marginal covariances of a loop-closure graph from its band form A = B + R: B = (Hd, Ho) block-tridiagonal, R the
// off-band couplings of the closure edges, both with the anchor's six pose rows / columns taken out (B_a, and M = R on the closure ends'
// pose DoF `cols_c`).  Woodbury:
//   Sigma = B_a^-1 - Y_c G Y_c^T,   Y_c = B_a^-1[:, cols_c],   G = (I + M Y_S)^-1 M,   Y_S = Y_c[cols_c, :]
// The blocks of B_a^-1 on and next to the diagonal come from the chain's selected inverse (pvgo_marginals.inl), its columns from the chain
// solver (pvgo_solver.inl, one unit right-hand side each), G (Rc x Rc, symmetric) from the caller.  New here:
//   band_anchor_kernel     the anchored copy of (Hd, Ho): identity on the anchor's pose rows / columns (what m_ldD / m_ldO do on load)
//   band_rhs_kernel        the next unit right-hand side: one entry cleared, one set
//   band_transpose_kernel  the solutions, stored one per row as the solver writes them, into Y (9N x ldy): column r = B_a^-1 e_cols[r]
//   band_project_kernel    V = Y[:, :Rc] G on v_mfma_f64_16x16x4_f64 (fragments and operand loads of dense_tile.h: both operands "row m,
//                          K contiguous" -- the rows of the symmetric G are the transposed operand); 128 rows x 64 columns per workgroup
//   band_node_kernel /     node_cov[k] = Sd[k] - V_k Y_k^T (symmetrised), pair_cov[p] = base(a, b) - V_a Y_b^T over the first Rc columns;
//   band_pair_kernel       one workgroup per block, entry (p, q) by one lane, its sum over the columns in ascending order
// No atomics, every sum in an order fixed by the shapes: the same inputs give the same bits.
#include <unordered_map>

#include "dense_tile.h"

namespace {

namespace bt = islam::tile;

constexpr int BC_NC = 4;             // 16-column groups of V per workgroup of band_project_kernel
constexpr int BC_CB = 160;           // pairs per launch of band_pair_kernel and the distinct far second nodes among them (passed by value:
constexpr int BC_NF = 48;            // 3.6 KB of kernel arguments)
constexpr int BC_KC = 64;            // columns of V and Y per LDS stage of the block kernels
constexpr int BC_T = 128;            // threads of a block kernel (81 of them own an entry)

__global__ __launch_bounds__(256) void band_anchor_kernel(const double* __restrict__ Hd, const double* __restrict__ Ho, int N, int anchor,
                                                          double* __restrict__ Ha, double* __restrict__ Hoa) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * 81) return;
    const int k = (int)(i / 81), e = (int)(i - (size_t)k * 81), r = e / 9, c = e - r * 9;
    Ha[i] = (k == anchor && (r < 6 || c < 6)) ? (r == c ? 1.0 : 0.0) : Hd[i];
    const bool cut = k == N - 1 || (k == anchor && r < 6) || (k + 1 == anchor && c < 6);     // (block N - 1 couples nothing)
    Hoa[i] = cut ? 0.0 : Ho[i];
}

__global__ void band_rhs_kernel(double* __restrict__ rhs, long long prev, long long cur) {
    if (threadIdx.x != 0) return;
    if (prev >= 0) rhs[prev] = 0.0;
    rhs[cur] = 1.0;
}

// Y[i * ldy + r] = Yt[r * n + i] (Yt: R rows of n = 9N), the anchor's pose rows as zero; 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void band_transpose_kernel(const double* __restrict__ Yt, int n, int R, int anchor, double* __restrict__ Y,
                                                             int ldy) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = r0 + ty + 8 * j, i = i0 + tx;
        tile[ty + 8 * j][tx] = (r < R && i < n) ? Yt[(size_t)r * n + i] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = i0 + ty + 8 * j, r = r0 + tx;
        if (i < n && r < R) {
            const bool fixed = anchor >= 0 && i >= 9 * anchor && i < 9 * anchor + 6;
            Y[(size_t)i * ldy + r] = fixed ? 0.0 : tile[tx][ty + 8 * j];
        }
    }
}

__global__ void band_status_kernel(const int* __restrict__ flags, int* __restrict__ status) {
    if (threadIdx.x == 0) status[0] = flags[0] ? ISLAM_ENOTPD : ISLAM_OK;
}

// V (n x ldv, ldv = 16 ceil(Rc / 16)) = Y[:, :Rc] G.  G: ldv rows of ldg >= ldv doubles, symmetric, zero outside its leading Rc x Rc.
// Workgroup (bx, by): rows [128 bx, +128), 32 per wave, columns [64 by, +64).  Rows past n are clamped and not stored (operand_row), column
// groups past ldv / 16 likewise; the last chunk of a ragged Rc reads Y only where the column is < Rc.
__global__ __launch_bounds__(256) void band_project_kernel(const double* __restrict__ Y, int ldy, int n, int Rc, const double* __restrict__ G,
                                                           int ldg, double* __restrict__ V, int ldv) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, q = lane >> 4;
    const int rw = blockIdx.x * bt::TM + wave * 32;       // first row of this wave
    if (rw >= n) return;                                   // (wave-uniform; no barrier in this kernel)
    const int ncg = ldv / 16, cg = blockIdx.y * BC_NC;
    const double* pa[2];
    const double* pb[BC_NC];
#pragma unroll
    for (int a = 0; a < 2; ++a) pa[a] = Y + (size_t)min(rw + 16 * a + m, n - 1) * (size_t)ldy + 4 * q;
#pragma unroll
    for (int c = 0; c < BC_NC; ++c) pb[c] = G + (size_t)(16 * min(cg + c, ncg - 1) + m) * (size_t)ldg + 4 * q;
    bt::d4 acc[2][BC_NC];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < BC_NC; ++c) acc[a][c] = bt::d4{0.0, 0.0, 0.0, 0.0};
    const bt::MfmaChunk<BC_NC> chunk{acc};
    // the chunks wholly inside the first Rc columns, two register sets: the loads of chunk i + 2 go out when chunk i has fed the matrix core
    bt::d4 fa[2][2], fb[2][BC_NC];
    const int nch = Rc / 16;
    auto load = [&](int d, int i) {                        // chunk min(i, nch - 1): the last sets reload the last chunk instead of reading past it
        const int k = 16 * (i < nch ? i : nch - 1);
#pragma unroll
        for (int a = 0; a < 2; ++a) fa[d][a] = bt::ld4(pa[a] + k);
#pragma unroll
        for (int c = 0; c < BC_NC; ++c) fb[d][c] = bt::ld4(pb[c] + k);
    };
    if (nch > 0) {
        load(0, 0);
        load(1, 1);
    }
    for (int i0 = 0; i0 < nch; i0 += 2) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            if (i0 + d < nch) {                            // (uniform)
                chunk(fa[d], fb[d]);
                load(d, i0 + d + 2);
            }
        }
    }
    if (Rc & 15) {                                         // the ragged chunk: columns [16 nch, Rc) of Y, zero beyond; G is padded
        const int k0 = 16 * nch;
        bt::d4 sa[2], sb[BC_NC];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e) sa[a][e] = k0 + 4 * q + e < Rc ? pa[a][k0 + e] : 0.0;
#pragma unroll
        for (int c = 0; c < BC_NC; ++c) sb[c] = bt::ld4(pb[c] + k0);
        chunk(sa, sb);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < BC_NC; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rw + 16 * a + q + 4 * i, col = 16 * (cg + c) + m;
                if (row < n && cg + c < ncg) V[(size_t)row * (size_t)ldv + col] = acc[a][c][i];
            }
}

struct BandBlocks {                  // what every block reads
    const double *Sd, *So, *Y, *V;
    int ldy, ldv, Rc, anchor;
};
struct BandPairs {                   // a far pair (more than one node apart) is computed as block (a, b), stored transposed when tr is set.
    int a[BC_CB], b[BC_CB], slot[BC_CB];      // slot: the row of `pos` that belongs to its node b (-1: not a far pair), + BC_TR when tr is set;
    int pos[BC_NF][9];                        // pos[slot][c]: where `cols` holds DoF c of that node (-1: it does not, the anchor's pose DoF)
};
constexpr int BC_TR = 1 << 16;

// out (9 x 9) = base(a, b) - V_a Y_b^T over the first Rc columns.  base: Sd[a] (a == b; the result is then symmetrised like the chain's
// Sigma_tt: the average of entries (p, q) and (q, p)), So[a] (b == a + 1), So[b]^T (a == b + 1), else the rows of node a of Y at the
// columns of node b.  The pose rows of a == anchor and the pose columns of b == anchor are written as zero.  Returns, on the lanes that own
// a diagonal entry outside the anchor's pose DoF of a block with a == b, whether that entry is not finite or not positive.
// tr: the block is stored transposed (the caller asked for (b, a)); col: where `cols` holds this lane's column q of node b (far pairs).
__device__ __forceinline__ bool band_cov_block(const BandBlocks& g, int a, int b, int col, bool tr, double* __restrict__ out) {
    __shared__ double sv[9][BC_KC + 1], sy[9][BC_KC + 1], res[81];
    const int t = threadIdx.x, p = t / 9, q = t - p * 9;
    const double* va = g.V + (size_t)(9 * a) * (size_t)g.ldv;
    const double* yb = g.Y + (size_t)(9 * b) * (size_t)g.ldy;
    double s = 0.0;
    for (int k0 = 0; k0 < g.Rc; k0 += BC_KC) {             // (trip count: a function of Rc only)
        const int w = min(BC_KC, g.Rc - k0);
        for (int i = t; i < 9 * BC_KC; i += BC_T) {
            const int r = i / BC_KC, k = i - r * BC_KC;
            sv[r][k] = k < w ? va[(size_t)r * g.ldv + k0 + k] : 0.0;
            sy[r][k] = k < w ? yb[(size_t)r * g.ldy + k0 + k] : 0.0;
        }
        __syncthreads();
        if (t < 81)
            for (int k = 0; k < w; ++k) s = fma(sv[p][k], sy[q][k], s);
        __syncthreads();
    }
    if (t < 81) {
        double base;
        if (a == b) base = g.Sd[(size_t)a * 81 + t];
        else if (b == a + 1) base = g.So[(size_t)a * 81 + t];
        else if (a == b + 1) base = g.So[(size_t)b * 81 + q * 9 + p];
        else {
            base = col >= 0 ? g.Y[(size_t)(9 * a + p) * (size_t)g.ldy + col] : 0.0;
        }
        res[t] = base - s;
    }
    __syncthreads();
    if (t >= 81) return false;
    const double v = a == b ? 0.5 * (res[p * 9 + q] + res[q * 9 + p]) : res[t];
    const bool fixed = (a == g.anchor && p < 6) || (b == g.anchor && q < 6);
    out[tr ? q * 9 + p : t] = fixed ? 0.0 : v;
    return a == b && p == q && !fixed && !(v > 0.0 && v - v == 0.0);
}

// status[0] was cleared before the launch; every lane that finds a bad diagonal stores the same word (plain stores, no atomic)
__global__ __launch_bounds__(BC_T) void band_node_kernel(BandBlocks g, double* __restrict__ node_cov, int* __restrict__ status) {
    const int k = blockIdx.x;
    if (band_cov_block(g, k, k, -1, false, node_cov + (size_t)k * 81) && status) status[0] = ISLAM_ENOTPD;
}

__global__ __launch_bounds__(BC_T) void band_pair_kernel(BandBlocks g, BandPairs pb, double* __restrict__ pair_cov) {
    const int i = blockIdx.x;
    const bool tr = pb.slot[i] >= BC_TR;
    const int slot = max(pb.slot[i], 0) & (BC_TR - 1), q = threadIdx.x % 9;
    int col = -1;                                          // where `cols` holds this lane's column of node b (read only for a far pair)
#pragma unroll
    for (int c = 0; c < 9; ++c) col = q == c ? pb.pos[slot][c] : col;
    (void)band_cov_block(g, pb.a[i], pb.b[i], col, tr, pair_cov + (size_t)i * 81);
}

constexpr int BAND_MAX_N = 200000000;      // 9 N + 255 fits an int

inline int band_pad16(int r) { return (r + 15) / 16 * 16; }

// the workspace of both calls: the chain solver's, the anchored band, one right-hand side, and R solutions of 9N doubles (rounded up to
// 9N x 16 ceil(R / 16): islam_pvgo_band_cov_blocks keeps V there)
struct BandWork { Workspace solve; double *Ha, *Hoa, *rhs, *Yt; size_t bytes; };
BandWork band_carve(void* base, int N, int R) {
    BandWork w;
    w.solve = carve(base, N);
    char* p = (char*)base + align_up(w.solve.bytes);
    auto take = [&](size_t nd) { double* r = (double*)p; p += align_up(nd * sizeof(double)); return r; };
    w.Ha = take((size_t)N * 81);
    w.Hoa = take((size_t)N * 81);
    w.rhs = take((size_t)N * 9);
    w.Yt = take((size_t)N * 9 * (size_t)band_pad16(R));
    w.bytes = (size_t)(p - (char*)base);
    return w;
}

// cols (host, R entries, the first Rc of them pose DoF): every index inside [0, 9N) and outside the anchor's pose DoF
int band_check_cols(const char* fn, const int64_t* cols, int R, int Rc, int N, int anchor) {
    for (int r = 0; r < R; ++r) {
        const long long c = (long long)cols[r];
        if (c < 0 || c >= 9LL * N) return fail(ISLAM_EARG, "%s: cols[%d] = %lld outside [0, %lld)", fn, r, c, 9LL * N);
        if (anchor >= 0 && c / 9 == anchor && c % 9 < 6) return fail(ISLAM_EARG, "%s: cols[%d] = %lld is a pose DoF of the anchor %d", fn, r, c, anchor);
        if (r < Rc && c % 9 >= 6) return fail(ISLAM_EARG, "%s: cols[%d] = %lld among the first Rc = %d is not a pose DoF", fn, r, c, Rc);
    }
    return ISLAM_OK;
}

}  // namespace

extern "C" {

size_t islam_pvgo_band_inverse_workspace_bytes(int N, int R) {
    if (N < 2 || N > BAND_MAX_N || R < 0) return 0;
    return band_carve(nullptr, N, R).bytes + 256;
}

int islam_pvgo_band_inverse_columns(const double* Hd, const double* Ho, int N, int anchor, const int64_t* cols, int R, const int seg_len[2],
                                    void* workspace, size_t workspace_bytes, double* Y, int ldy, int* status, void* stream) {
    const char* fn = "islam_pvgo_band_inverse_columns";
    if (N < 2 || N > BAND_MAX_N) return fail(ISLAM_EARG, "%s: N=%d outside [2, %d]", fn, N, BAND_MAX_N);
    if (R < 0 || ldy < R) return fail(ISLAM_EARG, "%s: R=%d, ldy=%d (0 <= R <= ldy expected)", fn, R, ldy);
    if (anchor < -1 || anchor >= N) return fail(ISLAM_EARG, "%s: anchor=%d outside [-1, %d)", fn, anchor, N);
    if (!Hd || !Ho || !workspace || (R > 0 && (!cols || !Y))) return fail(ISLAM_EARG, "%s: Hd / Ho / workspace / cols / Y is NULL", fn);
    const size_t need = islam_pvgo_band_inverse_workspace_bytes(N, R);
    if (workspace_bytes < need) return fail(ISLAM_EARG, "%s: workspace of %zu bytes, N=%d R=%d needs %zu", fn, workspace_bytes, N, R, need);
    if (int rc = band_check_cols(fn, cols, R, 0, N, anchor)) return rc;
    const int zero_seg[2] = {0, 0};
    if (!seg_len) seg_len = zero_seg;
    hipStream_t s = as_stream(stream);
    const BandWork w = band_carve((void*)align_up((size_t)workspace), N, R);
    const int n = 9 * N;
    ISLAM_HIP_CHECK(hipMemsetAsync(w.solve.flags, 0, 4 * sizeof(double), s));
    ISLAM_HIP_CHECK(hipMemsetAsync(w.solve.ready, 0, w.solve.ready_bytes, s));
    ISLAM_HIP_CHECK(hipMemsetAsync(w.rhs, 0, (size_t)n * sizeof(double), s));
    hipLaunchKernelGGL(band_anchor_kernel, dim3((unsigned)(((size_t)N * 81 + 255) / 256)), dim3(256), 0, s, Hd, Ho, N, anchor, w.Ha, w.Hoa);
    for (int r = 0; r < R; ++r) {
        hipLaunchKernelGGL(band_rhs_kernel, dim3(1), dim3(64), 0, s, w.rhs, r > 0 ? (long long)cols[r - 1] : -1LL, (long long)cols[r]);
        if (int rc = enqueue_solve(w.solve, w.Ha, w.Hoa, w.rhs, nullptr, 0.0, N, seg_len, w.Yt + (size_t)r * n, s)) return rc;
    }
    if (R > 0)
        hipLaunchKernelGGL(band_transpose_kernel, dim3((n + 31) / 32, (R + 31) / 32), dim3(256), 0, s, w.Yt, n, R, anchor, Y, ldy);
    if (status) hipLaunchKernelGGL(band_status_kernel, dim3(1), dim3(64), 0, s, w.solve.flags, status);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_band_cov_blocks(const double* Sd, const double* So, const double* Y, int ldy, int N, int anchor, const int64_t* cols, int R,
                               int Rc, const double* G, int ldg, const int64_t* pairs, int P, void* workspace, size_t workspace_bytes,
                               double* node_cov, double* pair_cov, int* status, void* stream) {
    const char* fn = "islam_pvgo_band_cov_blocks";
    if (N < 2 || N > BAND_MAX_N) return fail(ISLAM_EARG, "%s: N=%d outside [2, %d]", fn, N, BAND_MAX_N);
    if (R < 0 || Rc < 0 || Rc > R || ldy < R) return fail(ISLAM_EARG, "%s: R=%d, Rc=%d, ldy=%d (0 <= Rc <= R <= ldy expected)", fn, R, Rc, ldy);
    if (anchor < -1 || anchor >= N) return fail(ISLAM_EARG, "%s: anchor=%d outside [-1, %d)", fn, anchor, N);
    const int ldv = band_pad16(Rc);
    if (!Sd || !So || (R > 0 && (!cols || !Y)) || (Rc > 0 && (!G || !workspace)))
        return fail(ISLAM_EARG, "%s: Sd / So / Y / cols / G / workspace is NULL", fn);
    if (Rc > 0 && ldg < ldv) return fail(ISLAM_EARG, "%s: ldg=%d, G padded to %d rows and columns expected (Rc=%d)", fn, ldg, ldv, Rc);
    const size_t need = Rc > 0 ? align_up((size_t)N * 9 * (size_t)ldv * sizeof(double)) + 256 : 0;
    if (workspace_bytes < need) return fail(ISLAM_EARG, "%s: workspace of %zu bytes, N=%d Rc=%d needs %zu", fn, workspace_bytes, N, Rc, need);
    if (P < 0 || (P > 0 && !pairs)) return fail(ISLAM_EARG, "%s: P=%d, pairs=%p", fn, P, (const void*)pairs);
    if (int rc = band_check_cols(fn, cols, R, Rc, N, anchor)) return rc;
    std::unordered_map<int64_t, int> where;               // DoF index -> its position in cols
    for (int r = 0; r < R; ++r) where[cols[r]] = r;
    auto far = [](int64_t a, int64_t b) { return a - b > 1 || b - a > 1; };
    auto holds = [&](int64_t node) {                       // every DoF of the node but the anchor's pose
        for (int c = node == anchor ? 6 : 0; c < 9; ++c)
            if (!where.count(9 * node + c)) return false;
        return true;
    };
    for (int p = 0; p < P; ++p) {
        const int64_t a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a < 0 || a >= N || b < 0 || b >= N) return fail(ISLAM_EARG, "%s: pair %d = (%lld, %lld), N=%d", fn, p, (long long)a, (long long)b, N);
        if (!far(a, b)) continue;
        if (!holds(b))
            return fail(ISLAM_EARG, "%s: pair %d = (%lld, %lld) couples nodes more than one apart and cols does not hold every DoF of node %lld",
                        fn, p, (long long)a, (long long)b, (long long)b);
    }
    hipStream_t s = as_stream(stream);
    const int n = 9 * N;
    double* V = Rc > 0 ? (double*)align_up((size_t)workspace) : nullptr;
    if (status) ISLAM_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int), s));
    if (Rc > 0)
        hipLaunchKernelGGL(band_project_kernel, dim3((n + bt::TM - 1) / bt::TM, (ldv / 16 + BC_NC - 1) / BC_NC), dim3(256), 0, s, Y, ldy, n, Rc, G,
                           ldg, V, ldv);
    const BandBlocks g{Sd, So, Y, V, ldy, ldv, Rc, anchor};
    if (node_cov) hipLaunchKernelGGL(band_node_kernel, dim3(N), dim3(BC_T), 0, s, g, node_cov, status);
    if (pair_cov) {
        BandPairs pb;
        for (int base = 0; base < P;) {                    // a launch takes pairs until it holds BC_CB of them or BC_NF distinct far second nodes
            int cnt = 0, nf = 0;
            int64_t fnode[BC_NF];
            for (; cnt < BC_CB && base + cnt < P; ++cnt) {
                int64_t a = pairs[2 * (base + cnt)], b = pairs[2 * (base + cnt) + 1];
                int slot = -1;
                // a far pair (a, b), a > b, whose node a has its columns in `cols` too is computed as block (b, a) and stored transposed: the
                // same request the other way round reads the same columns, and the two blocks are transposes of each other to the bit
                const bool tr = far(a, b) && a > b && holds(a);
                if (tr) std::swap(a, b);
                if (far(a, b)) {
                    for (int f = 0; f < nf && slot < 0; ++f)
                        if (fnode[f] == b) slot = f;
                    if (slot < 0) {
                        if (nf == BC_NF) break;
                        slot = nf++;
                        fnode[slot] = b;
                        for (int c = 0; c < 9; ++c) {
                            const auto it = where.find(9 * b + c);
                            pb.pos[slot][c] = it == where.end() ? -1 : it->second;
                        }
                    }
                }
                pb.a[cnt] = (int)a;
                pb.b[cnt] = (int)b;
                pb.slot[cnt] = slot + (tr ? BC_TR : 0);
            }
            for (int p = cnt; p < BC_CB; ++p) pb.a[p] = pb.b[p] = 0, pb.slot[p] = -1;
            for (int f = nf; f < BC_NF; ++f)
                for (int c = 0; c < 9; ++c) pb.pos[f][c] = -1;
            hipLaunchKernelGGL(band_pair_kernel, dim3(cnt), dim3(BC_T), 0, s, g, pb, pair_cov + (size_t)base * 81);
            base += cnt;
        }
    }
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

}  // extern "C"
