// Covariance of the IMU pre-integration on gfx950: what pp.module.IMUPreintegrator(prop_cov=True) adds
// to the pre-integrated factors (PyPose, external: the match is unpinned; include/islam_hip.h states the definition).
//
// Error state [dphi, dv, dp] (Forster's ordering), dphi the right perturbation of the pre-integrated rotation.  Per sample
//   Sigma <- A Sigma A^T + Bg diag(sg2) Bg^T + Ba diag(sa2) Ba^T,
//   A = [ dr^T 0 0 ; -DR [a]x d  I 0 ; -DR [a]x d^2/2  I d  I ],  Bg = [ Jr(w d) d ; 0 ; 0 ],  Ba = [ 0 ; DR d ; DR d^2/2 ].
// The recurrence is an affine map on Sigma, and the pairs (Phi, Q) compose associatively.  Phi keeps the sparsity of A --
//   Phi = [ R 0 0 ; V I 0 ; P tI I ]   (three 3x3 blocks and the accumulated time) -- and Q is symmetric: 28 + 45 doubles.
// An element is kept LOCAL to the rotation at its own start (DR = I there); joining it behind an earlier element rotates its v and p
// rows by the rotation accumulated over the earlier one, which is R^T of that element: the operator needs nothing but its operands.
//
// Kernels (float64 arithmetic whatever the I/O type; no workgroup waits for another one: the levels are separate launches)
//   frame_reduce_kernel  one wavefront per frame: lane l folds samples [l c, (l + 1) c), c = ceil(F / 64), then a tree over the lanes;
//                        motion mode: the frame's Q is the output row; world mode: the frame's element goes to the scratch
//                        (element 0 joined behind init_cov)
//   scan_kernel          world mode, one wavefront per 64 elements of a level: Kogge-Stone scan in LDS, block totals = the next level
//   carry_kernel         joins a level's local prefixes behind the resolved prefix of the blocks in front of them
//   rows_kernel          the same for level 0, writing the symmetrised 9x9 rows (row 0 = init_cov)
// This translation unit carries no bit-exactness contract (the results are checked to a tolerance): FMA contraction stays on.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

using namespace islam;

namespace {

constexpr int EL = 73;        // doubles per element: R (9) | V (9) | P (9) | t | Q packed (45)
constexpr int QO = 28;        // offset of Q: a = Q_phiphi (6, upper triangle by rows) | b = Q_vphi (9) | c = Q_pphi (9) | d = Q_vv (6) | e = Q_pv (9) | f = Q_pp (6)
constexpr int WAVE = 64;

struct M3 { double m[9]; };

__device__ __forceinline__ M3 ld3(const double* p) { M3 o; for (int i = 0; i < 9; ++i) o.m[i] = p[i]; return o; }
__device__ __forceinline__ void st3(double* p, const M3& a) { for (int i = 0; i < 9; ++i) p[i] = a.m[i]; }
__device__ __forceinline__ M3 ldsym(const double* p) { return {{p[0], p[1], p[2], p[1], p[3], p[4], p[2], p[4], p[5]}}; }
// the symmetric part of a block that is symmetric up to rounding
__device__ __forceinline__ void stsym(double* p, const M3& a) {
    p[0] = a.m[0]; p[1] = 0.5 * (a.m[1] + a.m[3]); p[2] = 0.5 * (a.m[2] + a.m[6]);
    p[3] = a.m[4]; p[4] = 0.5 * (a.m[5] + a.m[7]); p[5] = a.m[8];
}
__device__ __forceinline__ M3 mm(const M3& a, const M3& b) {           // a b
    M3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
    return o;
}
__device__ __forceinline__ M3 mmt(const M3& a, const M3& b) {          // a b^T
    M3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.m[3 * i + j] = a.m[3 * i] * b.m[3 * j] + a.m[3 * i + 1] * b.m[3 * j + 1] + a.m[3 * i + 2] * b.m[3 * j + 2];
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
__device__ __forceinline__ M3 tr(const M3& a) { return {{a.m[0], a.m[3], a.m[6], a.m[1], a.m[4], a.m[7], a.m[2], a.m[5], a.m[8]}}; }
__device__ __forceinline__ M3 add(const M3& a, const M3& b) { M3 o; for (int i = 0; i < 9; ++i) o.m[i] = a.m[i] + b.m[i]; return o; }
__device__ __forceinline__ M3 axpy(double s, const M3& a, const M3& b) { M3 o; for (int i = 0; i < 9; ++i) o.m[i] = s * a.m[i] + b.m[i]; return o; }

// index of entry (r, c) of the 9x9 matrix inside the packed Q
__device__ __forceinline__ int q_index(int r, int c) {
    if (r < c) { const int t = r; r = c; c = t; }
    const int br = r / 3, bc = c / 3, ir = r - 3 * br, ic = c - 3 * bc;
    if (br == bc) {
        const int lo = ic < ir ? ic : ir, hi = ic < ir ? ir : ic;
        const int off = br == 0 ? 0 : (br == 1 ? 24 : 39);
        return off + (lo == 0 ? hi : (lo == 1 ? 2 + hi : 5));
    }
    return (br == 1 ? 6 : (bc == 0 ? 15 : 30)) + 3 * ir + ic;
}

__device__ __forceinline__ void set_identity(double* e) {
    for (int i = 0; i < EL; ++i) e[i] = 0.0;
    e[0] = e[4] = e[8] = 1.0;
}

// x <- (element `lo` that covers the earlier samples) joined with (element `hi` that covers the later ones, local to its own start).
// With W = R_lo^T (the rotation accumulated over `lo`), Phi' = [ R_hi 0 0 ; W V_hi I 0 ; W P_hi t_hi I I ], Q' = T Q_hi T^T, T = diag(I, W, W):
//   Phi = Phi' Phi_lo,  Q = Phi' Q_lo Phi'^T + Q'.
// `out` may alias `lo` or `hi` (every input is read before the first store).
__device__ __forceinline__ void join(const double* lo, const double* hi, double* out) {
    const M3 R1 = ld3(lo), V1 = ld3(lo + 9), P1 = ld3(lo + 18);
    const double t1 = lo[27], t2 = hi[27];
    const M3 R2 = ld3(hi);
    const M3 V2 = mtm(R1, ld3(hi + 9)), P2 = mtm(R1, ld3(hi + 18));            // W V_hi, W P_hi
    const M3 a1 = ldsym(lo + QO), b1 = ld3(lo + QO + 6), c1 = ld3(lo + QO + 15), d1 = ldsym(lo + QO + 24), e1 = ld3(lo + QO + 30),
             f1 = ldsym(lo + QO + 39);
    // Q' = T Q_hi T^T
    const M3 a2 = ldsym(hi + QO);
    const M3 b2 = mtm(R1, ld3(hi + QO + 6)), c2 = mtm(R1, ld3(hi + QO + 15));
    const M3 d2 = mm(mtm(R1, ldsym(hi + QO + 24)), R1), e2 = mm(mtm(R1, ld3(hi + QO + 30)), R1), f2 = mm(mtm(R1, ldsym(hi + QO + 39)), R1);
    // M = Phi' Q_lo, the blocks the lower triangle of M Phi'^T needs
    const M3 Mvf = add(mm(V2, a1), b1);
    const M3 Mvv = add(mmt(V2, b1), d1);
    const M3 Mpf = add(axpy(t2, b1, mm(P2, a1)), c1);
    const M3 Mpv = add(axpy(t2, d1, mmt(P2, b1)), e1);
    const M3 Mpp = add(axpy(t2, tr(e1), mmt(P2, c1)), f1);
    const M3 a = add(mmt(mm(R2, a1), R2), a2);
    const M3 b = add(mmt(Mvf, R2), b2);
    const M3 c = add(mmt(Mpf, R2), c2);
    const M3 d = add(add(mmt(Mvf, V2), Mvv), d2);
    const M3 e = add(add(mmt(Mpf, V2), Mpv), e2);
    const M3 f = add(add(axpy(t2, Mpv, mmt(Mpf, P2)), Mpp), f2);
    st3(out, mm(R2, R1));
    st3(out + 9, add(mm(V2, R1), V1));
    st3(out + 18, add(axpy(t2, V1, mm(P2, R1)), P1));
    out[27] = t1 + t2;
    stsym(out + QO, a); st3(out + QO + 6, b); st3(out + QO + 15, c);
    stsym(out + QO + 24, d); st3(out + QO + 30, e); stsym(out + QO + 39, f);
}

// The element of one sample, local to the rotation in front of it: d = dt, w = gyro, a = acc, sg / sa = the variances.
__device__ __forceinline__ void sample_element(double d, const double* w, const double* a, const double* sg, const double* sa, double* e) {
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
    M3 R, J;              // R = Exp^T = I - A K + B K^2
    for (int i = 0; i < 9; ++i) {
        const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
        R.m[i] = id - A * K.m[i] + B * K2.m[i];
        J.m[i] = id - B * K.m[i] + C * K2.m[i];
    }
    st3(e, R);
    const double hd2 = 0.5 * d * d;
    const M3 ax{{0, -a[2], a[1], a[2], 0, -a[0], -a[1], a[0], 0}};
    for (int i = 0; i < 9; ++i) { e[9 + i] = -d * ax.m[i]; e[18 + i] = -hd2 * ax.m[i]; }
    e[27] = d;
    for (int i = QO; i < EL; ++i) e[i] = 0.0;
    // Q_phiphi = d^2 Jr diag(sg) Jr^T
    M3 Js = J;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Js.m[3 * i + j] *= sg[j] * d * d;
    stsym(e + QO, mmt(Js, J));
    // [Q_vv Q_vp ; Q_pv Q_pp] = [ d ; d^2 / 2 ] diag(sa) [ d ; d^2 / 2 ]^T
    const int dg[3] = {0, 3, 5}, fg[3] = {0, 4, 8};
    for (int i = 0; i < 3; ++i) {
        e[QO + 24 + dg[i]] = d * d * sa[i];
        e[QO + 30 + fg[i]] = hd2 * d * sa[i];
        e[QO + 39 + dg[i]] = hd2 * hd2 * sa[i];
    }
}

// 64 rows of 81 doubles from 64 packed Qs in LDS (stride QS doubles), coalesced
template <int QS>
__device__ __forceinline__ void store_rows(const double* q, int cnt, double* __restrict__ out) {
    for (int t = threadIdx.x; t < cnt * 81; t += WAVE) {
        const int row = t / 81, en = t - 81 * row;
        out[t] = q[row * QS + q_index(en / 9, en - 9 * (en / 9))];
    }
}

// The element that carries init_cov into the scan: Phi = I, Q = the symmetric part of init_cov.
__device__ __forceinline__ void init_element(const double* __restrict__ init_cov, double* e) {
    for (int k = threadIdx.x; k < QO; k += WAVE) e[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    for (int t = threadIdx.x; t < 81; t += WAVE) {
        const int r = t / 9, c = t - 9 * r;
        if (r >= c) e[QO + q_index(r, c)] = 0.5 * (init_cov[9 * r + c] + init_cov[9 * c + r]);
    }
}

// One wavefront per frame.  elems != nullptr: the frame's element (world mode); else out rows (motion mode).
template <class T>
__global__ __launch_bounds__(WAVE) void frame_reduce_kernel(const T* __restrict__ dt, const T* __restrict__ gyro, const T* __restrict__ acc,
                                                            const int64_t* __restrict__ seg, double sgx, double sgy, double sgz, double sax,
                                                            double say, double saz, const T* __restrict__ sg_s, const T* __restrict__ sa_s,
                                                            int64_t S, const double* __restrict__ init_cov, double* __restrict__ elems,
                                                            double* __restrict__ out) {
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
            double sg[3] = {sgx, sgy, sgz}, sa[3] = {sax, say, saz};
            if (sg_s) { sg[0] = (double)sg_s[3 * sidx]; sg[1] = (double)sg_s[3 * sidx + 1]; sg[2] = (double)sg_s[3 * sidx + 2]; }
            if (sa_s) { sa[0] = (double)sa_s[3 * sidx]; sa[1] = (double)sa_s[3 * sidx + 1]; sa[2] = (double)sa_s[3 * sidx + 2]; }
            if (j == lane * chunk) {
                sample_element((double)dt[sidx], w, a, sg, sa, E);
            } else {
                double X[EL];
                sample_element((double)dt[sidx], w, a, sg, sa, X);
                join(E, X, E);
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
    if (elems && init_cov && i == 0) {                                // world mode: the first element carries init_cov into the scan
        init_element(init_cov, lds + EL);
        __syncthreads();
        if (lane == 0) join(lds + EL, E, E);
    }
    if (lane == 0)
        for (int k = 0; k < EL; ++k) lds[k] = E[k];
    __syncthreads();
    if (elems) {
        for (int k = lane; k < EL; k += WAVE) elems[(size_t)i * EL + k] = lds[k];
    } else {
        store_rows<EL>(lds + QO, 1, out + (size_t)i * 81);
    }
}

// One wavefront per 64 elements: inclusive scan in place (local to the block's first element); totals[b] = the block's last prefix.
__global__ __launch_bounds__(WAVE) void scan_kernel(double* __restrict__ elems, int n, double* __restrict__ totals) {
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
__global__ __launch_bounds__(WAVE) void carry_kernel(double* __restrict__ elems, int n, const double* __restrict__ parent) {
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (blockIdx.x == 0 || i >= n) return;
    double* e = elems + (size_t)i * EL;
    join(parent + (size_t)(blockIdx.x - 1) * EL, e, e);
}

// World rows 1 .. nframes from the level-0 prefixes (parent == nullptr: they are resolved already), row 0 = init_cov.  A frame without
// samples takes the row of the last frame in front of it that has some: the same arithmetic on the same operands, bit for bit.
__global__ __launch_bounds__(WAVE) void rows_kernel(const double* __restrict__ elems, int nframes, const double* __restrict__ parent,
                                                    const int64_t* __restrict__ seg, const double* __restrict__ init_cov,
                                                    double* __restrict__ out) {
    __shared__ double q[WAVE * 45];
    const int lane = threadIdx.x, base = blockIdx.x * WAVE, cnt = min(WAVE, nframes - base);
    if (blockIdx.x == 0)
        for (int t = lane; t < 81; t += WAVE) {
            const int r = t / 9, c = t - 9 * r;
            out[t] = init_cov ? 0.5 * (init_cov[9 * r + c] + init_cov[9 * c + r]) : 0.0;
        }
    if (lane < cnt) {
        int j = base + lane;
        while (j >= 0 && seg[j + 1] == seg[j]) --j;
        double* dst = q + lane * 45;
        if (j < 0) {
            for (int r = 0; r < 9; ++r)
                for (int c = 0; c <= r; ++c) dst[q_index(r, c)] = init_cov ? 0.5 * (init_cov[9 * r + c] + init_cov[9 * c + r]) : 0.0;
        } else {
            const double* e = elems + (size_t)j * EL;
            const int b = j / WAVE;
            if (parent && b > 0) {
                double E[EL];
                join(parent + (size_t)(b - 1) * EL, e, E);
                for (int k = 0; k < 45; ++k) dst[k] = E[QO + k];
            } else {
                for (int k = 0; k < 45; ++k) dst[k] = e[QO + k];
            }
        }
    }
    __syncthreads();
    store_rows<45>(q, cnt, out + (size_t)(base + 1) * 81);
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
int run(const T* dt, const T* gyro, const T* acc, const int64_t* seg, int nframes, int64_t S, const double* gc, const double* ac, const T* gcs,
        const T* acs, const double* init_cov, int motion_mode, double* out, void* scratch, hipStream_t s) {
    if (motion_mode) {
        if (nframes > 0)
            hipLaunchKernelGGL(frame_reduce_kernel<T>, dim3(nframes), dim3(WAVE), 0, s, dt, gyro, acc, seg, gc[0], gc[1], gc[2], ac[0], ac[1],
                               ac[2], gcs, acs, S, (const double*)nullptr, (double*)nullptr, out);
        ISLAM_LAUNCH_CHECK();
        return ISLAM_OK;
    }
    int cnt[MAX_LEVELS];
    double* lev[MAX_LEVELS];
    const int L = nframes > 0 ? plan_levels(nframes, cnt) : 0;
    double* p = reinterpret_cast<double*>(scratch);
    for (int l = 0; l < L; ++l) { lev[l] = p; p += (size_t)cnt[l] * EL; }
    if (nframes > 0)
        hipLaunchKernelGGL(frame_reduce_kernel<T>, dim3(nframes), dim3(WAVE), 0, s, dt, gyro, acc, seg, gc[0], gc[1], gc[2], ac[0], ac[1], ac[2],
                           gcs, acs, S, init_cov, lev[0], (double*)nullptr);
    for (int l = 0; l < L; ++l)                                        // up: local scans, block totals feed the next level
        hipLaunchKernelGGL(scan_kernel, dim3((cnt[l] + WAVE - 1) / WAVE), dim3(WAVE), 0, s, lev[l], cnt[l], l + 1 < L ? lev[l + 1] : (double*)nullptr);
    for (int l = L - 2; l >= 1; --l)                                   // down: the top level is resolved; resolve the ones below it
        hipLaunchKernelGGL(carry_kernel, dim3((cnt[l] + WAVE - 1) / WAVE), dim3(WAVE), 0, s, lev[l], cnt[l], lev[l + 1]);
    hipLaunchKernelGGL(rows_kernel, dim3(nframes > 0 ? (nframes + WAVE - 1) / WAVE : 1), dim3(WAVE), 0, s, L > 0 ? lev[0] : (const double*)nullptr,
                       nframes, L > 1 ? lev[1] : (const double*)nullptr, seg, init_cov, out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

bool bad_variance(const double* v) {
    for (int i = 0; i < 3; ++i)
        if (!(v[i] >= 0.0) || std::isinf(v[i])) return true;
    return false;
}

}  // namespace

extern "C" {

size_t islam_imu_preint_cov_scratch_bytes(int64_t S, int nframes) {
    if (nframes <= 0 || S < 0) return 0;
    int cnt[MAX_LEVELS];
    const int L = plan_levels(nframes, cnt);
    size_t n = 0;
    for (int l = 0; l < L; ++l) n += (size_t)cnt[l];
    return sizeof(double) * EL * n + 256;
}

int islam_imu_preint_cov(const void* dt, const void* gyro, const void* acc, const int64_t* seg, int nframes, int64_t S, int max_frame_samples,
                         const double gyro_cov[3], const double acc_cov[3], const void* gyro_cov_s, const void* acc_cov_s, const double* init_cov,
                         int motion_mode, double* out_cov, void* scratch, int dtype, void* stream) {
    if (nframes < 0 || S < 0) return fail(ISLAM_EARG, "islam_imu_preint_cov: nframes=%d S=%lld", nframes, (long long)S);
    if (max_frame_samples < 0 || max_frame_samples > S)
        return fail(ISLAM_EARG, "islam_imu_preint_cov: max frame samples %d out of range (S=%lld)", max_frame_samples, (long long)S);
    if (dtype != ISLAM_F64 && dtype != ISLAM_F32) return fail(ISLAM_EARG, "islam_imu_preint_cov: dtype %d", dtype);
    if (!gyro_cov || !acc_cov) return fail(ISLAM_EARG, "islam_imu_preint_cov: gyro_cov / acc_cov are required (three variances each)");
    if (bad_variance(gyro_cov) || bad_variance(acc_cov)) return fail(ISLAM_EARG, "islam_imu_preint_cov: a variance is negative or not finite");
    const bool motion = motion_mode != 0;
    if (!out_cov && (!motion || nframes > 0)) return fail(ISLAM_EARG, "islam_imu_preint_cov: out_cov is NULL");
    if (nframes > 0 && !seg) return fail(ISLAM_EARG, "islam_imu_preint_cov: seg is NULL (nframes=%d)", nframes);
    if (nframes > 0 && S > 0 && (!dt || !gyro || !acc)) return fail(ISLAM_EARG, "islam_imu_preint_cov: dt / gyro / acc is NULL (S=%lld)", (long long)S);
    if (nframes > 0 && !motion && !scratch) return fail(ISLAM_EARG, "islam_imu_preint_cov: world mode needs islam_imu_preint_cov_scratch_bytes() of scratch");
    hipStream_t s = as_stream(stream);
    if (dtype == ISLAM_F64)
        return run<double>((const double*)dt, (const double*)gyro, (const double*)acc, seg, nframes, S, gyro_cov, acc_cov, (const double*)gyro_cov_s,
                           (const double*)acc_cov_s, init_cov, motion ? 1 : 0, out_cov, scratch, s);
    return run<float>((const float*)dt, (const float*)gyro, (const float*)acc, seg, nframes, S, gyro_cov, acc_cov, (const float*)gyro_cov_s,
                      (const float*)acc_cov_s, init_cov, motion ? 1 : 0, out_cov, scratch, s);
}

}  // extern "C"
