// pvgo_marginals.inl -- part of the pvgo.hip translation unit (textually included there; not compiled on its own).
// Marginal covariances of a chain: the diagonal blocks and the (k, k+1) blocks of A^-1 for the block-tridiagonal
// A = (Hd, Ho), by a partitioned SELECTED INVERSION on the solver's level tree.
//
// Up-sweep, per segment (interior nodes c0 .. c0+cnt-1, separators L = c0-1, R = c0+cnt; either may be missing), left to right:
//   S_0 = A_c0c0, F_0 = A_c0,L;  node t:  [W^B | W^F | S_t^-1] = S_t^-1 [B_t | F_t | I]   (Gauss-Jordan, B_t = A_t,t+1 or A_last,R)
//   S_t+1 = A_t+1,t+1 - B_t^T W^B,  F_t+1 = -B_t^T W^F,  cL += F_t^T W^F;  last node: cR = B^T W^B, fill = -F^T W^B
// so that the separators form a block-tridiagonal chain D'_j = A_sj,sj - cR_j - cL_j+1, O'_j = fill_j+1, reduced the same way.
// Down-sweep, per segment, right to left (Takahashi; neighbours of node t when it is eliminated: N = t+1 or R, and L):
//   Sigma_t,N = -(W^B Sigma_NN + W^F Sigma_LN),  Sigma_t,L = -(W^B Sigma_NL + W^F Sigma_LL)
//   Sigma_tt  = S_t^-1 - Sigma_t,N W^B^T - Sigma_t,L W^F^T          (symmetrised)
// starting from Sigma_RR, Sigma_LR, Sigma_LL of the level above.  One wavefront per segment; the topmost level runs both sweeps
// in one workgroup (the whole call, one launch, for a chain the plan keeps on one level, such as the bilevel loop's 9-node window).
// The inputs are never written: the gauge anchor (the pose rows / columns of one node replaced by the identity) is applied on load.
namespace {

constexpr int MW = 243;              // per node and level: S^-1 | W^B | W^F, row-major 9x9 each

struct MSrc {                        // the matrix of one level
    int level0;
    const double *Hd, *Ho;           // level 0
    int anchor;                      // level 0: node whose pose DoF are replaced by the identity (-1: none)
    const double *Dsep, *cR, *cL, *fill;   // levels >= 1: the up-sweep products of the level below
    int Pprev;
};
struct MUp { double *W, *Dsep, *cR, *cL, *fill; };
struct MSig { double *D, *O; int anchor; };     // Sigma of a level: D (n,81), O (n-1,81); anchor >= 0: zero its pose rows on store

__device__ __forceinline__ double m_ldD(const MSrc& s, int k, int e) {
    if (s.level0) {
        const int r = e / 9, c = e - r * 9;
        if (k == s.anchor && (r < 6 || c < 6)) return r == c ? 1.0 : 0.0;
        return s.Hd[(size_t)k * 81 + e];
    }
    double v = s.Dsep[(size_t)k * 81 + e] - s.cR[(size_t)k * 81 + e];
    if (k + 1 < s.Pprev) v -= s.cL[(size_t)(k + 1) * 81 + e];
    return v;
}
__device__ __forceinline__ double m_ldO(const MSrc& s, int k, int e) {     // block (k, k+1)
    if (s.level0) {
        const int r = e / 9, c = e - r * 9;
        if ((k == s.anchor && r < 6) || (k + 1 == s.anchor && c < 6)) return 0.0;
        return s.Ho[(size_t)k * 81 + e];
    }
    return s.fill[(size_t)(k + 1) * 81 + e];
}
__device__ __forceinline__ void m_stD(const MSig& o, int k, int e, double v) {
    const int r = e / 9, c = e - r * 9;
    if (k == o.anchor && (r < 6 || c < 6)) v = 0.0;
    o.D[(size_t)k * 81 + e] = v;
}
__device__ __forceinline__ void m_stO(const MSig& o, int k, int e, double v) {
    const int r = e / 9, c = e - r * 9;
    if ((k == o.anchor && r < 6) || (k + 1 == o.anchor && c < 6)) v = 0.0;
    o.O[(size_t)k * 81 + e] = v;
}

struct MGeom { int c0, cnt, sR; bool has_left, has_right; };
__device__ __forceinline__ MGeom m_geom(int n, int m, int p) {
    MGeom g;
    g.c0 = p * (m + 1);
    g.cnt = min(m, n - g.c0);
    g.sR = g.c0 + m;
    g.has_left = p > 0;
    g.has_right = g.sR < n;
    return g;
}

// LDS of a sweep (doubles): up: S[2], F[2], B[2] (81 each) + W (27 columns of 9); down: Wn[2] (243) + SNN, SNL[2], SLL, XN (81)
constexpr int M_LDS_UP = 6 * 81 + 27 * 9;
constexpr int M_LDS_DOWN = 2 * MW + 5 * 81;
constexpr int M_LDS = M_LDS_UP > M_LDS_DOWN ? M_LDS_UP : M_LDS_DOWN;

__device__ void marg_up(const MSrc& src, const MUp& out, int n, int m, int p, int* flags, double* lds) {
    const int lane = threadIdx.x;
    const MGeom g = m_geom(n, m, p);
    double* S = lds;                 // [2][81] row-major
    double* F = lds + 162;           // [2][81] coupling (current node, L), row-major
    double* B = lds + 324;           // [2][81] coupling (current node, next node)
    double* W = lds + 486;           // 27 columns: W^B (0..8), W^F (9..17), S^-1 (18..26)
    auto coup = [&](int c, int e) -> double { return (c == g.c0 + g.cnt - 1 && !g.has_right) ? 0.0 : m_ldO(src, c, e); };
    for (int e = lane; e < 81; e += 64) {
        S[e] = m_ldD(src, g.c0, e);
        F[e] = g.has_left ? m_ldO(src, g.c0 - 1, (e % 9) * 9 + e / 9) : 0.0;
        B[e] = coup(g.c0, e);
        if (g.has_right) out.Dsep[(size_t)p * 81 + e] = m_ldD(src, g.sR, e);
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    __syncthreads();
    for (int t = 0; t < g.cnt; ++t) {
        const int c = g.c0 + t, cur = t & 1, nx = cur ^ 1;
        const bool more = t + 1 < g.cnt;
        const double* Sc = S + cur * 81;
        const double* Fc = F + cur * 81;
        const double* Bc = B + cur * 81;
        // the next node's blocks: requested now, needed after the elimination of this one
        double dn[2] = {0.0, 0.0}, bn[2] = {0.0, 0.0};
        if (more) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = lane + 64 * i;
                if (e < 81) { dn[i] = m_ldD(src, c + 1, e); bn[i] = coup(c + 1, e); }
            }
        }
        // Gauss-Jordan on [S | B | F | I]: lane j < 36 holds column j
        const int j = lane;
        double mc[9];
#pragma unroll
        for (int r = 0; r < 9; ++r)
            mc[r] = j < 9 ? Sc[r * 9 + j] : j < 18 ? Bc[r * 9 + j - 9] : j < 27 ? Fc[r * 9 + j - 18] : (r == j - 27 ? 1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            double a[9];
#pragma unroll
            for (int r = 0; r < 9; ++r) a[r] = bcast(mc[r], i);
            bad |= !(a[i] > 0.0);
            const double x = mc[i] * rcp_nr(a[i]);
#pragma unroll
            for (int r = 0; r < 9; ++r) mc[r] = r == i ? x : fma(-a[r], x, mc[r]);
        }
        if (j >= 9 && j < 36) {
            const int q = j - 9;
            double* wl = W + q * 9;
            const int blk = q < 9 ? 81 : q < 18 ? 162 : 0, cc = q % 9;
            double* wg = out.W + (size_t)c * MW + blk + cc;
#pragma unroll
            for (int r = 0; r < 9; ++r) { wl[r] = mc[r]; wg[r * 9] = mc[r]; }
        }
        __syncthreads();
        // S_t+1 = D_t+1 - B^T W^B | F_t+1 = -B^T W^F | cL += F^T W^F: entries lane + 64 i of the three 9x9 blocks
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            if (idx >= 243) break;
            const int which = idx / 81, e = idx - which * 81, r = e / 9, cc = e - r * 9;
            const double* L = which == 2 ? Fc : Bc;
            const double* R = W + (which == 0 ? cc : 9 + cc) * 9;
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 9; ++q) s = fma(L[q * 9 + r], R[q], s);
            if (which == 0) { if (more) S[nx * 81 + e] = dn[i] - s; }
            else if (which == 1) { if (more) F[nx * 81 + e] = -s; }
            else acc[i] += s;
        }
        if (!more && g.has_right) {
            for (int e = lane; e < 81; e += 64) {
                const int r = e / 9, cc = e - r * 9;
                double sb = 0.0, sf = 0.0;
#pragma unroll
                for (int q = 0; q < 9; ++q) { sb = fma(Bc[q * 9 + r], W[cc * 9 + q], sb); sf = fma(Fc[q * 9 + r], W[cc * 9 + q], sf); }
                out.cR[(size_t)p * 81 + e] = sb;
                if (g.has_left) out.fill[(size_t)p * 81 + e] = -sf;
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = lane + 64 * i;
                if (e < 81) B[nx * 81 + e] = bn[i];
            }
        }
        __syncthreads();
    }
    if (g.has_left) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = lane + 64 * i;
            if (idx >= 162 && idx < 243) out.cL[(size_t)p * 81 + idx - 162] = acc[i];
        }
    }
    if (bad && lane == 0) atomicOr(flags, 1);
}

// above: Sigma of the level above (separator j of this level = node j there); nullptr D: no level above (the top)
__device__ void marg_down(const double* __restrict__ Wst, const MSig& above, const MSig& out, int n, int m, int p, double* lds) {
    const int lane = threadIdx.x;
    const MGeom g = m_geom(n, m, p);
    double* Wn = lds;                // [2][243]: S^-1 | W^B | W^F of the node being processed (by step parity)
    double* SNN = lds + 2 * MW;
    double* SNL = SNN + 81;          // [2][81]
    double* SLL = SNL + 162;
    double* XN = SLL + 81;
    const bool hl = g.has_left && above.D, hr = g.has_right && above.D;
    for (int e = lane; e < 81; e += 64) {
        const int r = e / 9, cc = e - r * 9;
        SLL[e] = hl ? above.D[(size_t)(p - 1) * 81 + e] : 0.0;
        SNN[e] = hr ? above.D[(size_t)p * 81 + e] : 0.0;
        SNL[e] = (hl && hr) ? above.O[(size_t)(p - 1) * 81 + cc * 9 + r] : 0.0;     // Sigma_RL = Sigma_LR^T
        if (hr) m_stD(out, g.sR, e, SNN[e]);
    }
    const int clast = g.c0 + g.cnt - 1;
    for (int e = lane; e < MW; e += 64) Wn[e] = Wst[(size_t)clast * MW + e];
    __syncthreads();
    int pa, pb;
    pair_of(lane < 45 ? lane : 0, pa, pb);
    for (int t = g.cnt - 1, s = 0; t >= 0; --t, ++s) {
        const int c = g.c0 + t, cur = s & 1;
        const double* Wc = Wn + cur * MW;
        const double* WB = Wc + 81;
        const double* WF = Wc + 162;
        const double* SNLc = SNL + cur * 81;
        double* XL = SNL + (cur ^ 1) * 81;
        double wn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = lane + 64 * i;
            wn[i] = (t > 0 && e < MW) ? Wst[(size_t)(c - 1) * MW + e] : 0.0;
        }
        // Sigma_t,N (XN) and Sigma_t,L (XL)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = lane + 64 * i;
            if (idx >= 162) break;
            const int which = idx / 81, e = idx - which * 81, r = e / 9, cc = e - r * 9;
            double acc = 0.0;
            if (which == 0) {
#pragma unroll
                for (int q = 0; q < 9; ++q) acc = fma(WB[r * 9 + q], SNN[q * 9 + cc], acc);
#pragma unroll
                for (int q = 0; q < 9; ++q) acc = fma(WF[r * 9 + q], SNLc[cc * 9 + q], acc);     // Sigma_LN = Sigma_NL^T
                XN[e] = -acc;
                if (t < g.cnt - 1 || g.has_right) m_stO(out, c, e, -acc);
            } else {
#pragma unroll
                for (int q = 0; q < 9; ++q) acc = fma(WB[r * 9 + q], SNLc[q * 9 + cc], acc);
#pragma unroll
                for (int q = 0; q < 9; ++q) acc = fma(WF[r * 9 + q], SLL[q * 9 + cc], acc);
                XL[e] = -acc;
                if (t == 0 && g.has_left) m_stO(out, g.c0 - 1, cc * 9 + r, -acc);       // block (L, c0) = Sigma_c0,L^T
            }
        }
        __syncthreads();
        // Sigma_tt = S^-1 - XN W^B^T - XL W^F^T, the pair (a, b) and (b, a) by one lane, averaged: exactly symmetric
        if (lane < 45) {
            double vab = Wc[pa * 9 + pb], vba = Wc[pb * 9 + pa];
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                vab = fma(-XN[pa * 9 + q], WB[pb * 9 + q], vab);
                vba = fma(-XN[pb * 9 + q], WB[pa * 9 + q], vba);
            }
#pragma unroll
            for (int q = 0; q < 9; ++q) {
                vab = fma(-XL[pa * 9 + q], WF[pb * 9 + q], vab);
                vba = fma(-XL[pb * 9 + q], WF[pa * 9 + q], vba);
            }
            const double v = 0.5 * (vab + vba);
            SNN[pa * 9 + pb] = v;
            SNN[pb * 9 + pa] = v;
            m_stD(out, c, pa * 9 + pb, v);
            m_stD(out, c, pb * 9 + pa, v);
        }
        if (t > 0) {
            double* Wnx = Wn + (cur ^ 1) * MW;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = lane + 64 * i;
                if (e < MW) Wnx[e] = wn[i];
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void marg_up_kernel(MSrc src, MUp out, int n, int m, int* flags) {
    __shared__ double lds[M_LDS];
    marg_up(src, out, n, m, blockIdx.x, flags, lds);
}
__global__ __launch_bounds__(64) void marg_down_kernel(const double* __restrict__ Wst, MSig above, MSig out, int n, int m) {
    __shared__ double lds[M_LDS];
    marg_down(Wst, above, out, n, m, blockIdx.x, lds);
}
// the topmost level: one segment without separators, up-sweep and down-sweep in one workgroup.  fin (a one-level plan: this is
// the whole call): also what marg_finish_kernel does -- zeros instead of partial results, the status
__global__ __launch_bounds__(64) void marg_top_kernel(MSrc src, MUp up, MSig out, int n, int* flags, int fin, int* status) {
    __shared__ double lds[M_LDS];
    marg_up(src, up, n, n, 0, flags, lds);
    __syncthreads();
    marg_down(up.W, MSig{nullptr, nullptr, -1}, out, n, n, 0, lds);
    if (!fin) return;
    __syncthreads();
    const int f = __hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (status && threadIdx.x == 0) status[0] = f ? ISLAM_ENOTPD : ISLAM_OK;
    if (!f) return;
    for (int i = threadIdx.x; i < n * 81; i += blockDim.x) {
        out.D[i] = 0.0;
        if (i < (n - 1) * 81) out.O[i] = 0.0;
    }
}
// after the last level: a non-positive-definite matrix leaves zeros, not partial results; the status goes to `status` if given
__global__ void marg_finish_kernel(const int* flags, int* status, double* Sd, double* So, int N) {
    const int f = flags[0];
    if (status && blockIdx.x == 0 && threadIdx.x == 0) status[0] = f ? ISLAM_ENOTPD : ISLAM_OK;
    if (!f) return;
    const size_t nd = (size_t)N * 81, no = (size_t)(N - 1) * 81;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nd; i += (size_t)gridDim.x * blockDim.x) {
        Sd[i] = 0.0;
        if (i < no) So[i] = 0.0;
    }
}

// workspace: the status word, then per level (bounds as in carve: level l has at most N / 5^l nodes, N / 5^(l+1) + 2 segments)
// the per-node W records, the four per-segment products and (levels >= 1) Sigma of the level
struct MWork { int* flags; MUp up[MAXL]; MSig sig[MAXL]; size_t bytes; };
MWork mcarve(void* base, int N) {
    MWork w;
    char* p = (char*)base;
    auto take = [&](size_t nd) { double* r = (double*)p; p += align_up(nd * sizeof(double)); return r; };
    w.flags = (int*)take(4);
    size_t n = (size_t)N;
    for (int l = 0; l < MAXL; ++l) {
        const size_t segs = n / 5 + 2;
        w.up[l].W = take(n * MW);
        w.up[l].Dsep = take(segs * 81);
        w.up[l].cR = take(segs * 81);
        w.up[l].cL = take(segs * 81);
        w.up[l].fill = take(segs * 81);
        w.sig[l].D = l ? take(n * 81) : nullptr;
        w.sig[l].O = l ? take(n * 81) : nullptr;
        w.sig[l].anchor = -1;
        n = n / 5;
    }
    w.bytes = (size_t)(p - (char*)base);
    return w;
}

// the level plan of the selected inversion: the solver's planner with the one-sided cost model (every sweep here is one-sided)
static int marg_plan(int N, const int seg_len[2], SolvePlan& sp) { return plan_levels(N, seg_len, sp, false); }

static int marg_enqueue(const double* Hd, const double* Ho, int N, int anchor, const int seg_len[2], void* workspace,
                        double* Sd, double* So, int* status, hipStream_t s) {
    MWork w = mcarve((void*)align_up((size_t)workspace), N);
    SolvePlan sp;
    const int nl = marg_plan(N, seg_len, sp);
    ISLAM_HIP_CHECK(hipMemsetAsync(w.flags, 0, sizeof(int), s));
    w.sig[0].D = Sd;
    w.sig[0].O = So;
    w.sig[0].anchor = anchor;
    auto source = [&](int l) {
        MSrc src{};
        src.level0 = l == 0;
        src.Hd = Hd; src.Ho = Ho; src.anchor = anchor;
        if (l > 0) {
            src.Dsep = w.up[l - 1].Dsep; src.cR = w.up[l - 1].cR; src.cL = w.up[l - 1].cL; src.fill = w.up[l - 1].fill;
            src.Pprev = sp.lv[l - 1].P;
        }
        return src;
    };
    for (int l = 0; l + 1 < nl; ++l) {
        hipLaunchKernelGGL(marg_up_kernel, dim3(sp.lv[l].P), dim3(64), 0, s, source(l), w.up[l], sp.lv[l].n, sp.lv[l].m, w.flags);
        ISLAM_LAUNCH_CHECK();
    }
    const int T = nl - 1;
    hipLaunchKernelGGL(marg_top_kernel, dim3(1), dim3(64), 0, s, source(T), w.up[T], w.sig[T], sp.lv[T].n, w.flags, nl == 1 ? 1 : 0,
                       status);
    ISLAM_LAUNCH_CHECK();
    if (nl == 1) return ISLAM_OK;
    for (int l = nl - 2; l >= 0; --l) {
        hipLaunchKernelGGL(marg_down_kernel, dim3(sp.lv[l].P), dim3(64), 0, s, w.up[l].W, w.sig[l + 1], w.sig[l], sp.lv[l].n,
                           sp.lv[l].m);
        ISLAM_LAUNCH_CHECK();
    }
    const int nb = std::max(1, std::min(1024, (N * 81 + 255) / 256));
    hipLaunchKernelGGL(marg_finish_kernel, dim3(nb), dim3(256), 0, s, w.flags, status, Sd, So, N);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

}  // namespace

extern "C" {

size_t islam_pvgo_marginals_workspace_bytes(int N) {
    if (N < 1) return 0;
    return std::max(mcarve(nullptr, N).bytes + 256, islam_pvgo_workspace_bytes(N));
}

static int marg_check(const char* fn, int N, int anchor, size_t workspace_bytes, const double* Hd, const double* Sd) {
    if (N < 1) return fail(ISLAM_EARG, "%s: N=%d < 1", fn, N);
    if (anchor < -1 || anchor >= N) return fail(ISLAM_EARG, "%s: anchor=%d outside [-1, %d)", fn, anchor, N);
    if (workspace_bytes < islam_pvgo_marginals_workspace_bytes(N))
        return fail(ISLAM_EARG, "%s: workspace %zu < %zu bytes", fn, workspace_bytes, islam_pvgo_marginals_workspace_bytes(N));
    if (!Hd || !Sd) return fail(ISLAM_EARG, "%s: null Hd / Sd", fn);
    return ISLAM_OK;
}

int islam_pvgo_marginals(const double* Hd, const double* Ho, int N, int anchor, const int seg_len[2], void* workspace,
                         size_t workspace_bytes, double* Sd, double* So, void* stream) {
    int rc = marg_check("islam_pvgo_marginals", N, anchor, workspace_bytes, Hd, Sd);
    if (rc != ISLAM_OK) return rc;
    hipStream_t s = as_stream(stream);
    rc = marg_enqueue(Hd, Ho, N, anchor, seg_len, workspace, Sd, So, nullptr, s);
    if (rc != ISLAM_OK) return rc;
    MWork w = mcarve((void*)align_up((size_t)workspace), N);
    int flag = 0;
    ISLAM_HIP_CHECK(hipMemcpyAsync(&flag, w.flags, sizeof(int), hipMemcpyDeviceToHost, s));
    ISLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (flag) return fail(ISLAM_ENOTPD, "islam_pvgo_marginals: non-positive pivot (anchored matrix not positive definite)");
    return ISLAM_OK;
}

int islam_pvgo_marginals_enqueue(const double* Hd, const double* Ho, int N, int anchor, const int seg_len[2], void* workspace,
                                 size_t workspace_bytes, double* Sd, double* So, int* status, void* stream) {
    int rc = marg_check("islam_pvgo_marginals_enqueue", N, anchor, workspace_bytes, Hd, Sd);
    if (rc != ISLAM_OK) return rc;
    return marg_enqueue(Hd, Ho, N, anchor, seg_len, workspace, Sd, So, status, as_stream(stream));
}

int islam_pvgo_marginals_plan(int N, const int seg_len[2], int* plan9) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_marginals_plan: N=%d < 1", N);
    SolvePlan sp;
    const int nl = marg_plan(N, seg_len, sp);
    for (int l = 0; l < MAXL; ++l) {
        plan9[3 * l] = l < nl ? sp.lv[l].n : 0;
        plan9[3 * l + 1] = l < nl ? sp.lv[l].m : 0;
        plan9[3 * l + 2] = l < nl ? sp.lv[l].P : 0;
    }
    plan9[3 * MAXL] = nl - 1;
    return nl;
}

}  // extern "C"
