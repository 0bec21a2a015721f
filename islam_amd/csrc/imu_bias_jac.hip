// Bias Jacobians of the IMU pre-integration on gfx950, the first-order bias correction of pre-integrated
// increments and the closed-form gyro-bias solve from rotation residuals (Forster et al., "On-Manifold Preintegration", the quantities
// GTSAM and VINS keep on every pre-integrated factor).
//
// J = d[dphi, dv, dp] / d[b_g | b_a] (9x6) of a further bias b subtracted from every sample, at b = 0.  With A_j, Bg_j, Ba_j of
// islam_imu_preint_cov (include/islam_hip.h)
//   J_{j+1} = A_j J_j - [ Bg_j | Ba_j ],   J_0 = 0 (motion rows) or init_jac (world rows):
// an affine map on J whose linear part Phi is the covariance's, Phi = [ R 0 0 ; V I 0 ; P tI I ] (28 doubles).  The pairs (Phi, G)
// compose as (Phi2 Phi1, Phi2 G1 + G2); the (dphi, b_a) block of G is identically zero, which leaves five 3x3 blocks: 45 doubles.
// As in imu_cov.hip an element is kept LOCAL to the rotation at its own start (DR = I there); joining it behind an earlier element
// rotates its v and p ROWS by the rotation accumulated over the earlier one (R^T of that element).  The helpers are copies of
// imu_cov.hip's (that file is untouched: its results stay what they were, bit for bit); a join here is a subset of its block products.
//
// Kernels (float64 arithmetic whatever the I/O type; the levels are separate launches: no workgroup waits for another, no atomics)
//   bj_frame_reduce_kernel  one wavefront per frame: lane l folds samples [l c, (l + 1) c), c = ceil(F / 64), then a tree over the lanes;
//                           motion mode: the frame's G is the output row; world mode: the frame's element goes to the scratch
//                           (element 0 joined behind init_jac)
//   bj_scan_kernel          world mode, one wavefront per 64 elements of a level: Kogge-Stone scan in LDS, block totals = the next level
//   bj_carry_kernel         joins a level's local prefixes behind the resolved prefix of the blocks in front of them
//   bj_rows_kernel          the same for level 0, writing the 9x6 rows (row 0 = init_jac)
//   bias_correct_kernel     one lane per row: DR Exp(J_phig dbg), dv + J_vg dbg + J_va dba, dp + J_pg dbg + J_pa dba
//   gyro_bias_solve_kernel  one workgroup: per-row J^T J / J^T r terms compacted in row order, a fixed-order sum, Cholesky on one lane
// No bit-exactness contract against an oracle (the results are checked to a tolerance): FMA contraction stays on.
#include <hip/hip_runtime.h>

#include <cmath>

#include "imu_terms.h"

using namespace islam;

namespace {

constexpr int EL = 73;        // doubles per element: R (9) | V (9) | P (9) | t | G (45)
constexpr int GO = 28;        // offset of G: G_phig (9) | G_vg (9) | G_pg (9) | G_va (9) | G_pa (9), every block by rows
constexpr int WAVE = 64;

struct M3 { double m[9]; };

__device__ __forceinline__ M3 ld3(const double* p) { M3 o; for (int i = 0; i < 9; ++i) o.m[i] = p[i]; return o; }
__device__ __forceinline__ void st3(double* p, const M3& a) { for (int i = 0; i < 9; ++i) p[i] = a.m[i]; }
__device__ __forceinline__ M3 mm(const M3& a, const M3& b) {           // a b
    M3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
    return o;
}
__device__ __forceinline__ M3 mtm(const M3& a, const M3& b) {          // a^T b
    M3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.m[3 * i + j] = a.m[i] * b.m[j] + a.m[3 + i] * b.m[3 + j] + a.m[6 + i] * b.m[6 + j];
    return o;
}
__device__ __forceinline__ M3 add(const M3& a, const M3& b) { M3 o; for (int i = 0; i < 9; ++i) o.m[i] = a.m[i] + b.m[i]; return o; }
__device__ __forceinline__ M3 axpy(double s, const M3& a, const M3& b) { M3 o; for (int i = 0; i < 9; ++i) o.m[i] = s * a.m[i] + b.m[i]; return o; }

// offset inside G of entry (r, c) of the 9x6 matrix, -1 for the (dphi, b_a) block
__device__ __forceinline__ int g_index(int r, int c) {
    const int br = r / 3, bc = c / 3;
    if (bc == 0) return 9 * br + 3 * (r - 3 * br) + c;
    if (br == 0) return -1;
    return 27 + 9 * (br - 1) + 3 * (r - 3 * br) + (c - 3);
}

__device__ __forceinline__ void set_identity(double* e) {
    for (int i = 0; i < EL; ++i) e[i] = 0.0;
    e[0] = e[4] = e[8] = 1.0;
}

// x <- (element `lo` that covers the earlier samples) joined with (element `hi` that covers the later ones, local to its own start).
// With W = R_lo^T (the rotation accumulated over `lo`), Phi' = [ R_hi 0 0 ; W V_hi I 0 ; W P_hi t_hi I I ], G' = T G_hi, T = diag(I, W, W):
//   Phi = Phi' Phi_lo,  G = Phi' G_lo + G'.
// `out` may alias `lo` or `hi` (every input is read before the first store).
__device__ __forceinline__ void join(const double* lo, const double* hi, double* out) {
    const M3 R1 = ld3(lo), V1 = ld3(lo + 9), P1 = ld3(lo + 18);
    const double t1 = lo[27], t2 = hi[27];
    const M3 R2 = ld3(hi);
    const M3 V2 = mtm(R1, ld3(hi + 9)), P2 = mtm(R1, ld3(hi + 18));            // W V_hi, W P_hi
    const M3 Fg1 = ld3(lo + GO), Vg1 = ld3(lo + GO + 9), Pg1 = ld3(lo + GO + 18), Va1 = ld3(lo + GO + 27), Pa1 = ld3(lo + GO + 36);
    const M3 Fg = add(mm(R2, Fg1), ld3(hi + GO));
    const M3 Vg = add(add(mm(V2, Fg1), Vg1), mtm(R1, ld3(hi + GO + 9)));
    const M3 Pg = add(add(axpy(t2, Vg1, mm(P2, Fg1)), Pg1), mtm(R1, ld3(hi + GO + 18)));
    const M3 Va = add(Va1, mtm(R1, ld3(hi + GO + 27)));
    const M3 Pa = add(axpy(t2, Va1, Pa1), mtm(R1, ld3(hi + GO + 36)));
    st3(out, mm(R2, R1));
    st3(out + 9, add(mm(V2, R1), V1));
    st3(out + 18, add(axpy(t2, V1, mm(P2, R1)), P1));
    out[27] = t1 + t2;
    st3(out + GO, Fg); st3(out + GO + 9, Vg); st3(out + GO + 18, Pg); st3(out + GO + 27, Va); st3(out + GO + 36, Pa);
}

// Exp(w d)^T and -Jr(w d) d of one sample
__device__ __forceinline__ void sample_rot(double d, const double* w, M3& R, M3& Fg) {
    const double x = w[0] * d, y = w[1] * d, z = w[2] * d;
    const double th2 = x * x + y * y + z * z, th = sqrt(th2);
    double A, B, C;       // Exp = I + A K + B K^2,  Jr = I - B K + C K^2,  K = [theta]x
    if (th > 1e-3) {
        double s, c;
        sincos(th, &s, &c);
        const double sh = sin(0.5 * th);
        A = s / th; B = 2.0 * sh * sh / th2; C = (th - s) / (th2 * th);
    } else {
        A = 1.0 - th2 * (1.0 / 6.0) + th2 * th2 * (1.0 / 120.0);
        B = 0.5 - th2 * (1.0 / 24.0) + th2 * th2 * (1.0 / 720.0);
        C = 1.0 / 6.0 - th2 * (1.0 / 120.0) + th2 * th2 * (1.0 / 5040.0);
    }
    const M3 K{{0, -z, y, z, 0, -x, -y, x, 0}};
    const M3 K2 = mm(K, K);
    for (int i = 0; i < 9; ++i) {
        const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
        R.m[i] = id - A * K.m[i] + B * K2.m[i];
        Fg.m[i] = -d * (id - B * K.m[i] + C * K2.m[i]);
    }
}

// The element of one sample, local to the rotation in front of it: d = dt, w = gyro, a = acc.
//   Phi: R = Exp(w d)^T, V = -[a]x d, P = -[a]x d^2 / 2, t = d;   G = -[ Jr(w d) d  0 ; 0  I d ; 0  I d^2 / 2 ].
__device__ __forceinline__ void sample_element(double d, const double* w, const double* a, double* e) {
    M3 R, Fg;
    sample_rot(d, w, R, Fg);
    const double hd2 = 0.5 * d * d;
    const M3 ax{{0, -a[2], a[1], a[2], 0, -a[0], -a[1], a[0], 0}};
    for (int i = GO + 9; i < EL; ++i) e[i] = 0.0;
    st3(e, R);
    st3(e + GO, Fg);
    for (int i = 0; i < 9; ++i) { e[9 + i] = -d * ax.m[i]; e[18 + i] = -hd2 * ax.m[i]; }
    e[27] = d;
    e[GO + 27] = e[GO + 31] = e[GO + 35] = -d;
    e[GO + 36] = e[GO + 40] = e[GO + 44] = -hd2;
}

// e <- join(e, the element of the sample behind it): join() with the sample's zero blocks and P = V d / 2 written out
// (W = R_e^T; V2 = -W [a]x d, P2 = V2 d / 2; G_va' = -W d, G_pa' = -W d^2 / 2).
__device__ __forceinline__ void fold_sample(double* e, double d, const double* w, const double* a) {
    M3 R2, Fg2;
    sample_rot(d, w, R2, Fg2);
    const M3 R1 = ld3(e), V1 = ld3(e + 9), Fg1 = ld3(e + GO), Vg1 = ld3(e + GO + 9), Va1 = ld3(e + GO + 27);
    const double hd = 0.5 * d, hd2 = 0.5 * d * d;
    const M3 ax{{0, d * a[2], -d * a[1], -d * a[2], 0, d * a[0], d * a[1], -d * a[0], 0}};        // -[a]x d
    const M3 V2 = mtm(R1, ax);
    const M3 VR = mm(V2, R1), VF = mm(V2, Fg1);
    for (int i = 0; i < 9; ++i) {
        const double wt = R1.m[3 * (i % 3) + i / 3];                  // W = R1^T
        e[18 + i] = hd * VR.m[i] + d * V1.m[i] + e[18 + i];
        e[GO + 18 + i] = hd * VF.m[i] + d * Vg1.m[i] + e[GO + 18 + i];
        e[GO + 36 + i] = d * Va1.m[i] + e[GO + 36 + i] - hd2 * wt;
        e[GO + 27 + i] = Va1.m[i] - d * wt;
    }
    st3(e, mm(R2, R1));
    st3(e + 9, add(VR, V1));
    e[27] += d;
    st3(e + GO, add(mm(R2, Fg1), Fg2));
    st3(e + GO + 9, add(VF, Vg1));
}

// rows of 54 doubles from packed Gs in LDS (stride GS doubles), coalesced; the (dphi, b_a) block is written as 0.0
template <int GS>
__device__ __forceinline__ void store_rows(const double* g, int cnt, double* __restrict__ out) {
    for (int t = threadIdx.x; t < cnt * 54; t += WAVE) {
        const int row = t / 54, en = t - 54 * row;
        const int k = g_index(en / 6, en - 6 * (en / 6));
        out[t] = k < 0 ? 0.0 : g[row * GS + k];
    }
}

// init_jac (9x6 by rows) as a packed G; the (dphi, b_a) block is dropped
__device__ __forceinline__ void init_g(const double* __restrict__ init_jac, double* g) {
    for (int t = threadIdx.x; t < 54; t += WAVE) {
        const int k = g_index(t / 6, t - 6 * (t / 6));
        if (k >= 0) g[k] = init_jac[t];
    }
}

// One wavefront per frame.  elems != nullptr: the frame's element (world mode); else out rows (motion mode).
template <class T>
__global__ __launch_bounds__(WAVE) void bj_frame_reduce_kernel(const T* __restrict__ dt, const T* __restrict__ gyro, const T* __restrict__ acc,
                                                               const int64_t* __restrict__ seg, int64_t S, const double* __restrict__ init_jac,
                                                               double* __restrict__ elems, double* __restrict__ out) {
    __shared__ double lds[WAVE * EL];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int64_t s0 = min(max(seg[i], (int64_t)0), S);               // (offsets outside the slice read nothing)
    const int F = (int)(min(max(seg[i + 1], s0), S) - s0);
    const int chunk = (F + WAVE - 1) / WAVE;
    const int nact = chunk > 0 ? (F + chunk - 1) / chunk : 0;          // lanes that hold samples
    double E[EL];
    if (lane < nact) {
        const int j1 = min(F, (lane + 1) * chunk);
        for (int j = lane * chunk; j < j1; ++j) {
            const int64_t sidx = s0 + j;
            const double w[3] = {(double)gyro[3 * sidx], (double)gyro[3 * sidx + 1], (double)gyro[3 * sidx + 2]};
            const double a[3] = {(double)acc[3 * sidx], (double)acc[3 * sidx + 1], (double)acc[3 * sidx + 2]};
            if (j == lane * chunk) {
                sample_element((double)dt[sidx], w, a, E);
            } else {
                fold_sample(E, (double)dt[sidx], w, a);
            }
        }
    } else if (lane == 0) {
        set_identity(E);                                              // a frame without samples
    }
    // tree over the lanes: lane l takes in lane l + s
    for (int s = 1; s < nact; s *= 2) {
        if ((lane & (2 * s - 1)) == s && lane < nact)
            for (int k = 0; k < EL; ++k) lds[lane * EL + k] = E[k];
        __syncthreads();
        if ((lane & (2 * s - 1)) == 0 && lane + s < nact) join(E, lds + (lane + s) * EL, E);
        __syncthreads();
    }
    if (elems && init_jac && i == 0) {                                // world mode: the first element carries init_jac into the scan
        double* e0 = lds + EL;
        for (int k = lane; k < EL; k += WAVE) e0[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        __syncthreads();
        init_g(init_jac, e0 + GO);
        __syncthreads();
        if (lane == 0) join(e0, E, E);
    }
    if (lane == 0)
        for (int k = 0; k < EL; ++k) lds[k] = E[k];
    __syncthreads();
    if (elems) {
        for (int k = lane; k < EL; k += WAVE) elems[(size_t)i * EL + k] = lds[k];
    } else {
        store_rows<EL>(lds + GO, 1, out + (size_t)i * 54);
    }
}

// One wavefront per 64 elements: inclusive scan in place (local to the block's first element); totals[b] = the block's last prefix.
__global__ __launch_bounds__(WAVE) void bj_scan_kernel(double* __restrict__ elems, int n, double* __restrict__ totals) {
    __shared__ double lds[WAVE * EL];
    const int lane = threadIdx.x, base = blockIdx.x * WAVE, cnt = min(WAVE, n - base);
    double* g = elems + (size_t)base * EL;
    for (int k = lane; k < cnt * EL; k += WAVE) lds[k] = g[k];
    __syncthreads();
    double E[EL];
    if (lane < cnt)
        for (int k = 0; k < EL; ++k) E[k] = lds[lane * EL + k];
    for (int s = 1; s < cnt; s *= 2) {
        const bool on = lane >= s && lane < cnt;
        if (on) join(lds + (lane - s) * EL, E, E);
        __syncthreads();
        if (on)
            for (int k = 0; k < EL; ++k) lds[lane * EL + k] = E[k];
        __syncthreads();
    }
    for (int k = lane; k < cnt * EL; k += WAVE) g[k] = lds[k];
    if (totals)
        for (int k = lane; k < EL; k += WAVE) totals[(size_t)blockIdx.x * EL + k] = lds[(cnt - 1) * EL + k];
}

// elems[i] (local to block i / 64) <- joined behind parent[i / 64 - 1], the resolved prefix of everything in front of that block
__global__ __launch_bounds__(WAVE) void bj_carry_kernel(double* __restrict__ elems, int n, const double* __restrict__ parent) {
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (blockIdx.x == 0 || i >= n) return;
    double* e = elems + (size_t)i * EL;
    join(parent + (size_t)(blockIdx.x - 1) * EL, e, e);
}

// World rows 1 .. nframes from the level-0 prefixes (parent == nullptr: they are resolved already), row 0 = init_jac.  A frame without
// samples takes the row of the last frame in front of it that has some: the same arithmetic on the same operands, bit for bit.
__global__ __launch_bounds__(WAVE) void bj_rows_kernel(const double* __restrict__ elems, int nframes, const double* __restrict__ parent,
                                                       const int64_t* __restrict__ seg, const double* __restrict__ init_jac,
                                                       double* __restrict__ out) {
    __shared__ double g[(WAVE + 1) * 45];
    const int lane = threadIdx.x, base = blockIdx.x * WAVE, cnt = min(WAVE, nframes - base);
    double* g0 = g + WAVE * 45;                                       // init_jac, packed
    for (int k = lane; k < 45; k += WAVE) g0[k] = 0.0;
    __syncthreads();
    if (init_jac) init_g(init_jac, g0);
    __syncthreads();
    if (blockIdx.x == 0) store_rows<45>(g0, 1, out);
    if (lane < cnt) {
        int j = base + lane;
        while (j >= 0 && seg[j + 1] == seg[j]) --j;
        double* dst = g + lane * 45;
        if (j < 0) {
            for (int k = 0; k < 45; ++k) dst[k] = g0[k];
        } else {
            const double* e = elems + (size_t)j * EL;
            const int b = j / WAVE;
            if (parent && b > 0) {
                double E[EL];
                join(parent + (size_t)(b - 1) * EL, e, E);
                for (int k = 0; k < 45; ++k) dst[k] = E[GO + k];
            } else {
                for (int k = 0; k < 45; ++k) dst[k] = e[GO + k];
            }
        }
    }
    __syncthreads();
    if (cnt > 0) store_rows<45>(g, cnt, out + (size_t)(base + 1) * 54);
}

constexpr int MAX_LEVELS = 8;         // 64^8 frames

// level sizes of the scan: n, ceil(n / 64), ... down to one block
int plan_levels(int nframes, int (&cnt)[MAX_LEVELS]) {
    int L = 0;
    for (int n = nframes; L < MAX_LEVELS; n = (n + WAVE - 1) / WAVE) {
        cnt[L++] = n;
        if (n <= WAVE) break;
    }
    return L;
}

template <class T>
int run(const T* dt, const T* gyro, const T* acc, const int64_t* seg, int nframes, int64_t S, const double* init_jac, int motion_mode,
        double* out, void* scratch, hipStream_t s) {
    if (motion_mode) {
        if (nframes > 0)
            hipLaunchKernelGGL(bj_frame_reduce_kernel<T>, dim3(nframes), dim3(WAVE), 0, s, dt, gyro, acc, seg, S, (const double*)nullptr,
                               (double*)nullptr, out);
        ISLAM_LAUNCH_CHECK();
        return ISLAM_OK;
    }
    int cnt[MAX_LEVELS];
    double* lev[MAX_LEVELS];
    const int L = nframes > 0 ? plan_levels(nframes, cnt) : 0;
    double* p = reinterpret_cast<double*>(scratch);
    for (int l = 0; l < L; ++l) { lev[l] = p; p += (size_t)cnt[l] * EL; }
    if (nframes > 0)
        hipLaunchKernelGGL(bj_frame_reduce_kernel<T>, dim3(nframes), dim3(WAVE), 0, s, dt, gyro, acc, seg, S, init_jac, lev[0], (double*)nullptr);
    for (int l = 0; l < L; ++l)                                        // up: local scans, block totals feed the next level
        hipLaunchKernelGGL(bj_scan_kernel, dim3((cnt[l] + WAVE - 1) / WAVE), dim3(WAVE), 0, s, lev[l], cnt[l], l + 1 < L ? lev[l + 1] : (double*)nullptr);
    for (int l = L - 2; l >= 1; --l)                                   // down: the top level is resolved; resolve the ones below it
        hipLaunchKernelGGL(bj_carry_kernel, dim3((cnt[l] + WAVE - 1) / WAVE), dim3(WAVE), 0, s, lev[l], cnt[l], lev[l + 1]);
    hipLaunchKernelGGL(bj_rows_kernel, dim3(nframes > 0 ? (nframes + WAVE - 1) / WAVE : 1), dim3(WAVE), 0, s, L > 0 ? lev[0] : (const double*)nullptr,
                       nframes, L > 1 ? lev[1] : (const double*)nullptr, seg, init_jac, out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// ---------------------------------------------------------------------------------------------------- bias correction
struct Bias6 { double g[3], a[3]; };

template <class T>
__global__ __launch_bounds__(256) void bias_correct_kernel(const double* __restrict__ jac, const T* __restrict__ rot, const T* __restrict__ vel,
                                                           const T* __restrict__ pos, int rows, Bias6 b, T* __restrict__ out_rot,
                                                           T* __restrict__ out_vel, T* __restrict__ out_pos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const double* J = jac + (size_t)i * 54;
    double th[3], dv[3], dp[3];
    for (int r = 0; r < 3; ++r) {
        th[r] = J[6 * r] * b.g[0] + J[6 * r + 1] * b.g[1] + J[6 * r + 2] * b.g[2];
        const double* jv = J + 6 * (3 + r);
        const double* jp = J + 6 * (6 + r);
        dv[r] = jv[0] * b.g[0] + jv[1] * b.g[1] + jv[2] * b.g[2] + jv[3] * b.a[0] + jv[4] * b.a[1] + jv[5] * b.a[2];
        dp[r] = jp[0] * b.g[0] + jp[1] * b.g[1] + jp[2] * b.g[2] + jp[3] * b.a[0] + jp[4] * b.a[1] + jp[5] * b.a[2];
    }
    // Exp(th) as a quaternion xyzw
    const double t2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2], t = sqrt(t2);
    double im, re;
    if (t > 1e-4) { im = sin(0.5 * t) / t; re = cos(0.5 * t); }
    else { im = 0.5 - t2 * (1.0 / 48.0); re = 1.0 - t2 * (1.0 / 8.0); }
    const double bx = th[0] * im, by = th[1] * im, bz = th[2] * im, bw = re;
    const double ax = (double)rot[4 * (size_t)i], ay = (double)rot[4 * (size_t)i + 1], az = (double)rot[4 * (size_t)i + 2], aw = (double)rot[4 * (size_t)i + 3];
    double qx = aw * bx + ax * bw + ay * bz - az * by;
    double qy = aw * by - ax * bz + ay * bw + az * bx;
    double qz = aw * bz + ax * by - ay * bx + az * bw;
    double qw = aw * bw - ax * bx - ay * by - az * bz;
    const double n = 1.0 / sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    out_rot[4 * (size_t)i] = (T)(qx * n); out_rot[4 * (size_t)i + 1] = (T)(qy * n);
    out_rot[4 * (size_t)i + 2] = (T)(qz * n); out_rot[4 * (size_t)i + 3] = (T)(qw * n);
    for (int r = 0; r < 3; ++r) {
        out_vel[3 * (size_t)i + r] = (T)((double)vel[3 * (size_t)i + r] + dv[r]);
        out_pos[3 * (size_t)i + r] = (T)((double)pos[3 * (size_t)i + r] + dp[r]);
    }
}

// ---------------------------------------------------------------------------------------------------- gyro-bias solve
constexpr int NT = 9;                 // per-row terms: w J^T J (upper triangle by rows, 6) | w J^T r (3)
constexpr double PIVOT_REL = 1e-13;   // a Cholesky pivot below this share of its diagonal entry: H counts as singular

// One workgroup.  The rows that count (finite residual, finite non-zero weight) are compacted IN ROW ORDER into `terms`, then summed in
// a fixed order that depends on nothing but their number: a row of weight zero and a row that is not there give the same bits.
template <class T>
__global__ __launch_bounds__(256) void gyro_bias_solve_kernel(const double* __restrict__ jac, const T* __restrict__ rot_imu,
                                                              const T* __restrict__ rot_ref, const double* __restrict__ weight, int rows,
                                                              double* __restrict__ terms, int* __restrict__ status,
                                                              double* __restrict__ out_dbg, double* __restrict__ out_H) {
    __shared__ int wkeep[4], wbad[4];
    __shared__ double red[256 * NT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int fill = 0, bad = 0;
    for (int base = 0; base < rows; base += 256) {
        const int i = base + tid;
        bool keep = false, isbad = false;
        double v[NT];
        if (i < rows) {
            const double w = weight ? weight[i] : 1.0;
            const T* a = rot_imu + 4 * (size_t)i;
            const T* b = rot_ref + 4 * (size_t)i;
            // (imu_time_offset.hip's row_system copies these lines: behind one shared function some instantiation compiles differently)
            const double ax = -(double)a[0], ay = -(double)a[1], az = -(double)a[2], aw = (double)a[3];       // DR^T
            const double bx = (double)b[0], by = (double)b[1], bz = (double)b[2], bw = (double)b[3];
            double qx = aw * bx + ax * bw + ay * bz - az * by;
            double qy = aw * by - ax * bz + ay * bw + az * bx;
            double qz = aw * bz + ax * by - ay * bx + az * bw;
            double qw = aw * bw - ax * bx - ay * by - az * bz;
            if (qw < 0.0) { qx = -qx; qy = -qy; qz = -qz; qw = -qw; }
            const double vn = sqrt(qx * qx + qy * qy + qz * qz);
            const double k = vn > 1e-8 * qw ? 2.0 * atan2(vn, qw) / vn : 2.0 / qw;             // Log = k * imaginary part
            const double r[3] = {k * qx, k * qy, k * qz};
            const bool fin = isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(w);
            keep = fin && w != 0.0;
            isbad = !fin && !(w == 0.0);
            const double* J = jac + (size_t)i * 54;
            const double j0[3] = {J[0], J[6], J[12]}, j1[3] = {J[1], J[7], J[13]}, j2[3] = {J[2], J[8], J[14]};  // columns of J_phig
            auto dot = [](const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
            v[0] = w * dot(j0, j0); v[1] = w * dot(j0, j1); v[2] = w * dot(j0, j2);
            v[3] = w * dot(j1, j1); v[4] = w * dot(j1, j2); v[5] = w * dot(j2, j2);
            v[6] = w * dot(j0, r); v[7] = w * dot(j1, r); v[8] = w * dot(j2, r);
        }
        const unsigned long long mk = __ballot(keep), mb = __ballot(isbad);
        if (lane == 0) { wkeep[wv] = __popcll(mk); wbad[wv] = __popcll(mb); }
        __syncthreads();
        int off = fill;
        for (int q = 0; q < 4; ++q) {
            if (q < wv) off += wkeep[q];
            fill += wkeep[q];
            bad += wbad[q];
        }
        if (keep) {
            double* d = terms + (size_t)(off + __popcll(mk & ((1ull << lane) - 1ull))) * NT;
            for (int q = 0; q < NT; ++q) d[q] = v[q];
        }
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    double acc[NT];
    for (int q = 0; q < NT; ++q) acc[q] = 0.0;
    for (int c = tid; c < fill; c += 256)
        for (int q = 0; q < NT; ++q) acc[q] += terms[(size_t)c * NT + q];
    for (int q = 0; q < NT; ++q) red[tid * NT + q] = acc[q];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s)
            for (int q = 0; q < NT; ++q) red[tid * NT + q] += red[(tid + s) * NT + q];
        __syncthreads();
    }
    if (tid == 0) {
        const double h00 = red[0], h01 = red[1], h02 = red[2], h11 = red[3], h12 = red[4], h22 = red[5];
        double x[3] = {0.0, 0.0, 0.0};
        bool pd = false;
        // H = L L^T
        if (h00 > 0.0 && isfinite(h00)) {
            const double l00 = sqrt(h00), l10 = h01 / l00, l20 = h02 / l00;
            const double p1 = h11 - l10 * l10;
            if (p1 > PIVOT_REL * h11) {
                const double l11 = sqrt(p1), l21 = (h12 - l20 * l10) / l11;
                const double p2 = h22 - l20 * l20 - l21 * l21;
                if (p2 > PIVOT_REL * h22 && isfinite(p2)) {
                    const double l22 = sqrt(p2);
                    const double y0 = red[6] / l00, y1 = (red[7] - l10 * y0) / l11, y2 = (red[8] - l20 * y0 - l21 * y1) / l22;
                    x[2] = y2 / l22;
                    x[1] = (y1 - l21 * x[2]) / l11;
                    x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
                    pd = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
                    if (!pd) x[0] = x[1] = x[2] = 0.0;
                }
            }
        }
        out_dbg[0] = x[0]; out_dbg[1] = x[1]; out_dbg[2] = x[2];
        if (out_H) {
            out_H[0] = h00; out_H[1] = h01; out_H[2] = h02;
            out_H[3] = h01; out_H[4] = h11; out_H[5] = h12;
            out_H[6] = h02; out_H[7] = h12; out_H[8] = h22;
        }
        status[0] = pd ? 0 : 1;
        status[1] = bad;
    }
}

}  // namespace

extern "C" {

size_t islam_imu_preint_bias_jac_scratch_bytes(int64_t S, int nframes) {
    if (nframes <= 0 || S < 0) return 0;
    int cnt[MAX_LEVELS];
    const int L = plan_levels(nframes, cnt);
    size_t n = 0;
    for (int l = 0; l < L; ++l) n += (size_t)cnt[l];
    return sizeof(double) * EL * n + 256;
}

int islam_imu_preint_bias_jac(const void* dt, const void* gyro, const void* acc, const int64_t* seg, int nframes, int64_t S,
                              int max_frame_samples, const double* init_jac, int motion_mode, double* out_jac, void* scratch, int dtype,
                              void* stream) {
    if (nframes < 0 || S < 0) return fail(ISLAM_EARG, "islam_imu_preint_bias_jac: nframes=%d S=%lld", nframes, (long long)S);
    if (max_frame_samples < 0 || max_frame_samples > S)
        return fail(ISLAM_EARG, "islam_imu_preint_bias_jac: max frame samples %d out of range (S=%lld)", max_frame_samples, (long long)S);
    if (dtype != ISLAM_F64 && dtype != ISLAM_F32) return fail(ISLAM_EARG, "islam_imu_preint_bias_jac: dtype %d", dtype);
    const bool motion = motion_mode != 0;
    if (!out_jac && (!motion || nframes > 0)) return fail(ISLAM_EARG, "islam_imu_preint_bias_jac: out_jac is NULL");
    if (nframes > 0 && !seg) return fail(ISLAM_EARG, "islam_imu_preint_bias_jac: seg is NULL (nframes=%d)", nframes);
    if (nframes > 0 && S > 0 && (!dt || !gyro || !acc)) return fail(ISLAM_EARG, "islam_imu_preint_bias_jac: dt / gyro / acc is NULL (S=%lld)", (long long)S);
    if (nframes > 0 && !motion && !scratch)
        return fail(ISLAM_EARG, "islam_imu_preint_bias_jac: world mode needs islam_imu_preint_bias_jac_scratch_bytes() of scratch");
    hipStream_t s = as_stream(stream);
    if (dtype == ISLAM_F64)
        return run<double>((const double*)dt, (const double*)gyro, (const double*)acc, seg, nframes, S, init_jac, motion ? 1 : 0, out_jac, scratch, s);
    return run<float>((const float*)dt, (const float*)gyro, (const float*)acc, seg, nframes, S, init_jac, motion ? 1 : 0, out_jac, scratch, s);
}

int islam_imu_bias_correct(const double* jac, const void* rot, const void* vel, const void* pos, int rows, const double dbg[3],
                           const double dba[3], void* out_rot, void* out_vel, void* out_pos, int dtype, void* stream) {
    if (const int rc = tsum::check_entry("islam_imu_bias_correct", rows, dtype)) return rc;
    if (!dbg || !dba) return fail(ISLAM_EARG, "islam_imu_bias_correct: dbg / dba are required (three values each, host memory)");
    if (rows > 0 && (!jac || !rot || !vel || !pos || !out_rot || !out_vel || !out_pos))
        return fail(ISLAM_EARG, "islam_imu_bias_correct: jac / rot / vel / pos / out_rot / out_vel / out_pos is NULL (rows=%d)", rows);
    if (rows == 0) return ISLAM_OK;
    const Bias6 b{{dbg[0], dbg[1], dbg[2]}, {dba[0], dba[1], dba[2]}};
    hipStream_t s = as_stream(stream);
    const dim3 grid((rows + 255) / 256);
    if (dtype == ISLAM_F64)
        hipLaunchKernelGGL(bias_correct_kernel<double>, grid, dim3(256), 0, s, jac, (const double*)rot, (const double*)vel, (const double*)pos, rows, b,
                           (double*)out_rot, (double*)out_vel, (double*)out_pos);
    else
        hipLaunchKernelGGL(bias_correct_kernel<float>, grid, dim3(256), 0, s, jac, (const float*)rot, (const float*)vel, (const float*)pos, rows, b,
                           (float*)out_rot, (float*)out_vel, (float*)out_pos);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

size_t islam_imu_gyro_bias_solve_scratch_bytes(int rows) { return sizeof(double) * (tsum::HEAD + (size_t)NT * (rows > 0 ? rows : 0)); }

int islam_imu_gyro_bias_solve(const double* jac, const void* rot_imu, const void* rot_ref, const double* weight, int rows, double* out_dbg,
                              double* out_H, void* scratch, int dtype, void* stream) {
    if (const int rc = tsum::check_entry("islam_imu_gyro_bias_solve", rows, dtype)) return rc;
    if (!out_dbg || !scratch) return fail(ISLAM_EARG, "islam_imu_gyro_bias_solve: out_dbg / scratch is NULL");
    if (rows > 0 && (!jac || !rot_imu || !rot_ref)) return fail(ISLAM_EARG, "islam_imu_gyro_bias_solve: jac / rot_imu / rot_ref is NULL (rows=%d)", rows);
    hipStream_t s = as_stream(stream);
    int* status = reinterpret_cast<int*>(scratch);
    double* terms = reinterpret_cast<double*>(scratch) + tsum::HEAD;
    if (dtype == ISLAM_F64)
        hipLaunchKernelGGL(gyro_bias_solve_kernel<double>, dim3(1), dim3(256), 0, s, jac, (const double*)rot_imu, (const double*)rot_ref, weight, rows,
                           terms, status, out_dbg, out_H);
    else
        hipLaunchKernelGGL(gyro_bias_solve_kernel<float>, dim3(1), dim3(256), 0, s, jac, (const float*)rot_imu, (const float*)rot_ref, weight, rows,
                           terms, status, out_dbg, out_H);
    int host[2];
    if (const int rc = tsum::read_status(status, s, host)) return rc;
    if (host[0] != 0)
        return fail(ISLAM_ENOTPD, "islam_imu_gyro_bias_solve: the 3x3 normal matrix of %d rows (%d excluded) is not positive definite", rows, host[1]);
    return host[1];
}

}  // extern "C"
