// Joint two-view dense bundle adjustment on gfx950: the pose of a link and one inverse depth per pixel, the stereo depth as a
// Gaussian prior, the depths eliminated pixel by pixel (definitions: include/islam_hip.h, "dense reprojection"; DESIGN.md section
// 3.25).  It stands beside dense_reproj.hip and shares its per-pixel front (reproj_pixel), reduction epilogue, final-kernel body,
// Cholesky step, sum layout and host-side argument checks (dense_reproj_dev.h).
//
// Per pixel of link b at inverse depth rho, all in fp64:  P = (1/rho) ray,  Q = T^-1 P,  r, valid, s, c, J_cam as in section 3.23,
//   jd = dr/drho = dr/dQ R ray (-1/rho^2),   h_pd = c J_cam^T jd,   h_dd = c jd.jd + w,   g_d = c jd.r + w (rho - rho0),
// and the camera-frame sums are the per-pixel Schur complements: sum c J^T J - h_pd h_pd^T / h_dd, sum c J^T r - h_pd g_d / h_dd,
// cost = sum rho_rob(s) + w (rho - rho0)^2.  No atomics, one row of 30 per workgroup by plain stores, so repeats give the same bits.
// Under refinement evaluation k >= 1 is still one launch of the partial kernel, in two sweeps of the workgroup's pixels: the first
// forms every pixel's trial rho from the state the previous final kernel left (current pose, current rho, pose step) and writes it
// to the link's other buffer, the second evaluates the sums at (trial pose, trial rho), each thread reading back its own writes.
// (One sweep with both halves per pixel needs 446 VGPRs, one wave per SIMD, and spills at 256; two sweeps need no more than the
// pose-only kernel)  Both sweeps call ba_pixel for the per-pixel terms, and the second sweep is the only
// code that forms sums, so islam_dense_ba_normal at the returned state runs the same instructions on the same bits.
// Further down: the gradient of the joint refinement in depth and flow (joint_adj_partial_kernel, joint_adj_solve_kernel,
// joint_adj_vjp_kernel).
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "dense_reproj_dev.h"
#include "lie_dev.h"

using namespace islam;

namespace {

// where the partial kernel finds and leaves the inverse depths
struct RhoState {
    const double* given;       // eval < 0 (normal equations at a given state): (B,H,W) or nullptr = the prior
    double *buf0, *buf1;       // eval >= 0: the two (B,H,W) buffers of the refinement
    const int* select;         // (B) which buffer is current (read for eval >= 1)
    const int* status;         // (B) a link whose status is set stands still
    const double* cur_pose;    // (B,7) the current pose (eval >= 1)
    const double* delta;       // (B,6) the pose step that led to the trial pose (eval >= 1)
    int eval;
};

// everything of one pixel at (T^-1 = (R, t), rho) that the sums and the back-substitution need: the shared front at z = 1 / rho and
// jd = dr/drho = dr/dQ R ray (-1/rho^2)
struct BaPixel {
    Pixel p;
    double jdu, jdv;
};

ISLAM_DEV BaPixel ba_pixel(const M3<double>& R, const V3<double>& t, double rho, double xh, double yh, double tu, double tv, bool m,
                           const Intr& in, int kind, double delta, double d2) {
    BaPixel b;
    const double zi = 1.0 / rho;
    b.p = reproj_pixel(R, t, zi, xh, yh, tu, tv, m, in, kind, delta, d2);
    const V3<double> dR = R * V3<double>{xh, yh, 1.0};      // dQ/d(1/rho)
    const double k = -(zi * zi);
    b.jdu = (b.p.a * dR.x + b.p.bq * dR.z) * k;
    b.jdv = (b.p.cq * dR.y + b.p.dq * dR.z) * k;
    return b;
}

ISLAM_DEV void pose_to_lds(const SE3<double>& Ti, double* dst) {
    m3_store(qmat(Ti.q), dst);
    dst[9] = Ti.t.x;
    dst[10] = Ti.t.y;
    dst[11] = Ti.t.z;
}

__global__ __launch_bounds__(256) void dense_ba_partial_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                                const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                                const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                                const double* __restrict__ prior_weight, double* __restrict__ partial,
                                                                int H, int W, int kind, double delta, RhoState rs) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const Intr in = intr_load(intr4 + 4 * b);
    const double w = prior_weight[b];
    const bool wok = w > 0.0;
    const double d2 = delta * delta;
    // the back-substitution sweep runs at the current pose (Tp[0]), the sums at the pose under evaluation (Tp[1])
    const bool backsub = rs.eval >= 1 && rs.status[b] == ISLAM_DENSE_REPROJ_OK;
    __shared__ double Tp[2][12], dcam[6];
    if (threadIdx.x == 0) {
        pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp[1]);
        if (backsub) {
            pose_to_lds(camera_inverse(rs.cur_pose + 7 * b, rgb2imu), Tp[0]);
            const double* dl = rs.delta + 6 * b;
            V3<double> dr{dl[0], dl[1], dl[2]}, df{dl[3], dl[4], dl[5]};
            adjoint_apply(rgb2imu, dr, df);      // delta_cam = Ad(C^-1) delta
            dcam[0] = dr.x; dcam[1] = dr.y; dcam[2] = dr.z; dcam[3] = df.x; dcam[4] = df.y; dcam[5] = df.z;
        }
    }
    __syncthreads();

    const size_t off = (size_t)b * HW;
    const float* zp = depth + off;
    const float* fup = flow + 2 * off;
    const float* fvp = fup + HW;
    const uint8_t* mp = mask ? mask + off : nullptr;
    const double* rcur = nullptr;      // the inverse depths this evaluation starts from (nullptr: the prior)
    double* rnext = nullptr;           // where the state is initialised (evaluation 0) or the trial goes
    if (rs.eval == 0) {
        rnext = rs.buf0 + off;
    } else if (rs.eval >= 1) {
        const int sel = rs.select[b];
        rcur = (sel ? rs.buf1 : rs.buf0) + off;
        rnext = backsub ? (sel ? rs.buf0 : rs.buf1) + off : nullptr;
    } else if (rs.given) {
        rcur = rs.given + off;
    }

    // First sweep (evaluation k >= 1 of a link that is still being refined): every pixel's trial rho from the current pose, the
    // current rho and the pose step.  A pixel invalid at the current state goes back to its prior; one without a prior stays at 0.
    if (backsub) {
        const M3<double> R = m3_load(Tp[0]);
        const V3<double> t{Tp[0][9], Tp[0][10], Tp[0][11]};
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
            const int v = i / W, u = i - v * W;
            const double ud = (double)u, vd = (double)v;
            const double z = (double)zp[i];
            const bool prior = isfinite(z) && z > 0.0;
            const double rho0 = prior ? 1.0 / z : 0.0;
            const double rho = rcur[i];
            double trial = rho0;
            if (prior && rho > 0.0) {
                const BaPixel p = ba_pixel(R, t, rho, (ud - in.cx) / in.fx, (vd - in.cy) / in.fy, (double)fup[i] + ud, (double)fvp[i] + vd,
                                           mp ? mp[i] != 0 : true, in, kind, delta, d2);
                if (p.p.valid) {
                    const double eu = p.p.c * p.jdu, ev = p.p.c * p.jdv;
                    const double hdd = eu * p.jdu + ev * p.jdv + w;
                    const double gd = eu * p.p.ru + ev * p.p.rv + w * (rho - rho0);
                    double du = 0.0, dv = 0.0;      // J_cam delta_cam
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        du += p.p.ju[q] * dcam[q];
                        dv += p.p.jv[q] * dcam[q];
                    }
                    trial = rho - (gd + (eu * du + ev * dv)) / hdd;
                    if (!(isfinite(trial) && trial > 0.0)) trial = rho;
                }
            }
            rnext[i] = trial;
        }
    }

    // Second sweep: the sums at the pose under evaluation and at the trial rho (each thread reads back what it wrote itself), or at
    // the state as given.  This is the only code that forms the sums, so islam_dense_ba_normal repeats a refinement's bits.
    double acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0.0;
    const double* rsrc = backsub ? rnext : rcur;
    const M3<double> R = m3_load(Tp[1]);
    const V3<double> t{Tp[1][9], Tp[1][10], Tp[1][11]};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const int v = i / W, u = i - v * W;
        const double ud = (double)u, vd = (double)v;
        const double z = (double)zp[i];
        const bool prior = isfinite(z) && z > 0.0;
        const double rho0 = prior ? 1.0 / z : 0.0;
        const double rho = rsrc ? rsrc[i] : rho0;
        if (rs.eval == 0) rnext[i] = rho0;
        if (!(prior && wok && isfinite(rho) && rho > 0.0)) continue;      // outside the valid set at every state
        const BaPixel p = ba_pixel(R, t, rho, (ud - in.cx) / in.fx, (vd - in.cy) / in.fy, (double)fup[i] + ud, (double)fvp[i] + vd,
                                   mp ? mp[i] != 0 : true, in, kind, delta, d2);
        if (!p.p.valid) continue;
        const double c = p.p.c, ru = p.p.ru, rv = p.p.rv;
        // with e = c jd:  h_pd = J_cam^T e,  h_dd = e.jd + w,  g_d = e.r + w (rho - rho0).  The pixel's Schur term takes the shape of
        // section 3.23's: c J^T J - h_pd h_pd^T / h_dd = J^T M J with the 2x2 M = c I - e e^T / h_dd, and
        // c J^T r - h_pd g_d / h_dd = J^T (c r - e g_d / h_dd)
        const double eu = c * p.jdu, ev = c * p.jdv;
        const double dprior = rho - rho0;
        const double hdd = eu * p.jdu + ev * p.jdv + w;
        const double gd = eu * ru + ev * rv + w * dprior;
        const double ih = 1.0 / hdd;
        const double fu = eu * ih, fv = ev * ih;
        const double m00 = c - fu * eu, m01 = -(fu * ev), m11 = c - fv * ev;
        const double su = c * ru - fu * gd, sv = c * rv - fv * gd;
        int k = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double wu = m00 * p.p.ju[q] + m01 * p.p.jv[q], wv = m01 * p.p.ju[q] + m11 * p.p.jv[q];
#pragma unroll
            for (int l = q; l < 6; ++l) acc[k++] += wu * p.p.ju[l] + wv * p.p.jv[l];
            acc[S_G + q] += p.p.ju[q] * su + p.p.jv[q] * sv;
        }
        acc[S_COST] += p.p.rob + w * dprior * dprior;
        acc[S_L1] += fabs(ru) + fabs(rv);
        acc[S_COUNT] += 1.0;
    }
    // a link without a usable prior weight has no sums: NaN, which the final kernel reports
    reduce_and_store_row(acc, partial + ((size_t)b * NBLK + blockIdx.x) * NS, wok);
}

__global__ __launch_bounds__(64) void dense_ba_final_kernel(const double* __restrict__ partial, const double* __restrict__ rgb2imu,
                                                             const double* __restrict__ pose_eval, Outputs out, Refine rf, Joint jt, int B) {
    final_body<true>(partial, rgb2imu, pose_eval, out, rf, jt, B);
}

// the refined inverse depths out of whichever buffer the link's selector names
__global__ __launch_bounds__(256) void dense_ba_gather_kernel(const double* __restrict__ buf0, const double* __restrict__ buf1,
                                                               const int* __restrict__ select, double* __restrict__ out, int HW) {
    const int b = blockIdx.y;
    const double* src = (select[b] ? buf1 : buf0) + (size_t)b * HW;
    double* dst = out + (size_t)b * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) dst[i] = src[i];
}

}  // namespace

extern "C" size_t islam_dense_ba_scratch_bytes(int B, int H, int W, int iters_or_0) {
    if (B < 1 || H < 1 || W < 1) return 0;
    size_t n = partial_bytes(B);
    if (iters_or_0 > 0)      // trial pose, pose step, selector, two inverse-depth buffers
        n += align_up((size_t)B * 7 * sizeof(double)) + align_up((size_t)B * 6 * sizeof(double)) + align_up((size_t)B * sizeof(int)) +
             2 * align_up((size_t)B * H * W * sizeof(double));
    return n;
}

extern "C" int islam_dense_ba_normal(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                     const double* rgb2imu, const double* intr4, const double* prior_weight,
                                     const double* inv_depth_or_null, int robust_kind, double robust_delta, double* out_S, double* out_g,
                                     double* out_cost, double* out_l1, double* out_count, double* out_sums, void* scratch, int B, int H,
                                     int W, void* stream) {
    const Outputs o{out_S, out_g, out_cost, out_l1, out_count, out_sums};
    if (int rc = check_common("islam_dense_ba_normal", depth, flow, motion, intr4, robust_kind, robust_delta, o, scratch, B, H, W,
                              prior_weight != nullptr))
        return rc;
    hipStream_t s = as_stream(stream);
    double* partial = static_cast<double*>(scratch);
    RhoState rs{};
    rs.given = inv_depth_or_null;
    rs.eval = -1;
    hipLaunchKernelGGL(dense_ba_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu, intr4, prior_weight,
                       partial, H, W, robust_kind, robust_delta, rs);
    hipLaunchKernelGGL(dense_ba_final_kernel, dim3(B), dim3(64), 0, s, partial, rgb2imu, motion, o, Refine{}, Joint{}, B);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" int islam_dense_ba_refine(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                     const double* rgb2imu, const double* intr4, const double* prior_weight, int robust_kind,
                                     double robust_delta, int iters, double damping, double min_count, double* out_motion,
                                     double* out_inv_depth, double* out_S, double* out_g, double* out_cost, double* out_l1,
                                     double* out_count, double* out_sums, double* out_lambda, int* out_accepted, int* out_rejected,
                                     int* out_status, double* trace, int trace_cap, void* scratch, int B, int H, int W, void* stream) {
    const char* who = "islam_dense_ba_refine";
    const Outputs o{out_S, out_g, out_cost, out_l1, out_count, out_sums};
    if (int rc = check_common(who, depth, flow, motion, intr4, robust_kind, robust_delta, o, scratch, B, H, W, prior_weight != nullptr))
        return rc;
    Refine rf{out_motion, nullptr, out_lambda, out_accepted, out_rejected, out_status, trace_cap > 0 ? trace : nullptr, trace_cap, 0, 0,
              min_count, damping};
    if (int rc = check_refine(who, iters, rf, trace)) return rc;
    if (!out_inv_depth) return fail(ISLAM_EARG, "%s: NULL out_inv_depth", who);
    hipStream_t s = as_stream(stream);
    char* base = static_cast<char*>(scratch);
    double* partial = reinterpret_cast<double*>(base);
    base += partial_bytes(B);
    double* trial = reinterpret_cast<double*>(base);
    base += align_up((size_t)B * 7 * sizeof(double));
    double* step = reinterpret_cast<double*>(base);
    base += align_up((size_t)B * 6 * sizeof(double));
    int* select = reinterpret_cast<int*>(base);
    base += align_up((size_t)B * sizeof(int));
    const size_t HW = (size_t)H * W;
    double* buf0 = reinterpret_cast<double*>(base);
    double* buf1 = reinterpret_cast<double*>(base + align_up((size_t)B * HW * sizeof(double)));
    rf.trial = trial;
    const Joint jt{prior_weight, step, select};
    RhoState rs{nullptr, buf0, buf1, select, out_status, out_motion, step, 0};
    for (int k = 0; k < iters; ++k) {
        const double* pose = k == 0 ? motion : trial;
        rf.eval = rs.eval = k;
        rf.last = k == iters - 1;
        hipLaunchKernelGGL(dense_ba_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, pose, rgb2imu, intr4, prior_weight,
                           partial, H, W, robust_kind, robust_delta, rs);
        hipLaunchKernelGGL(dense_ba_final_kernel, dim3(B), dim3(64), 0, s, partial, rgb2imu, pose, o, rf, jt, B);
    }
    hipLaunchKernelGGL(dense_ba_gather_kernel, dim3(NBLK, B), dim3(256), 0, s, buf0, buf1, select, out_inv_depth, (int)HW);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// ------------------------------------------------------------------ the gradient of the joint refinement in depth and flow
//   At the state (T*, rho*) a refinement returned the joint gradient G = [g_p; g_d] vanishes, so a loss L on
// the outputs has dL = lambda^T dG with H_full lambda = -v, v = [v_p; v_d] the loss's gradient in the pose tangent and in every rho*.
// The depths are eliminated pixel by pixel as in the forward pass:
//   u_cam = sum_valid h_pd v_d / h_dd,   S lambda_p = -(v_p - A^T u_cam),   lambda_cam = A lambda_p,
//   lambda_d = -(v_d + h_pd^T lambda_cam) / h_dd   (an invalid pixel with a prior: c = 0, lambda_d = -v_d / w),
// and with Phi = lambda_p^T g_p + sum lambda_d g_d at fixed state, lambda and valid set, q = J_cam lambda_cam + jd lambda_d:
//   dPhi/dflow = -(c q + 2 c' (q.r) r),   dPhi/ddepth = w lambda_d / depth^2.
// joint_adj_partial_kernel reduces u_cam (one row of 6 per workgroup, plain stores), joint_adj_solve_kernel makes lambda_p,
// joint_adj_vjp_kernel streams the two gradients out.  (The three names keep clear of the four substrings by which
// tests/test_dense_reproj_cpu.py counts the family's seven older kernels.)
namespace {

__global__ __launch_bounds__(256) void joint_adj_partial_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                                 const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                                 const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                                 const double* __restrict__ prior_weight, const double* __restrict__ inv_depth,
                                                                 const double* __restrict__ grad_rho, const int* __restrict__ status,
                                                                 double* __restrict__ partial6, int H, int W, int kind, double delta) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const double w = prior_weight[b];
    // a marked link (or one without a usable prior weight) stores rows of zeros without reading its pixels
    const bool live = w > 0.0 && !(status && status[b] != ISLAM_DENSE_REPROJ_OK);
    double acc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = 0.0;
    if (live) {
        const Intr in = intr_load(intr4 + 4 * b);
        const double d2 = delta * delta;
        __shared__ double Tp[12];
        if (threadIdx.x == 0) pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
        __syncthreads();
        const M3<double> R = m3_load(Tp);
        const V3<double> t{Tp[9], Tp[10], Tp[11]};
        const size_t off = (size_t)b * HW;
        const float* zp = depth + off;
        const float* fup = flow + 2 * off;
        const float* fvp = fup + HW;
        const uint8_t* mp = mask ? mask + off : nullptr;
        const double* rp = inv_depth + off;
        const double* vp = grad_rho + off;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
            const int v = i / W, u = i - v * W;
            const double ud = (double)u, vd = (double)v;
            const double z = (double)zp[i];
            const double rho = rp[i];
            if (!(isfinite(z) && z > 0.0 && isfinite(rho) && rho > 0.0)) continue;
            const BaPixel p = ba_pixel(R, t, rho, (ud - in.cx) / in.fx, (vd - in.cy) / in.fy, (double)fup[i] + ud, (double)fvp[i] + vd,
                                       mp ? mp[i] != 0 : true, in, kind, delta, d2);
            if (!p.p.valid) continue;
            const double eu = p.p.c * p.jdu, ev = p.p.c * p.jdv;
            const double k = vp[i] / (eu * p.jdu + ev * p.jdv + w);      // v_d / h_dd
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += (eu * p.p.ju[q] + ev * p.p.jv[q]) * k;
        }
    }
    reduce_and_store_row6(acc, partial6 + ((size_t)b * NBLK + blockIdx.x) * 6, live);
}

// lambda_p per link.  v_p from the gradient on [t, q xyzw] as reproj_ift_kernel forms it; u_cam = the NBLK rows in fixed order (0 when
// the reduction did not run); A^T u = [R^T u_rho; R^T (u_phi - t x u_rho)] with C^-1 = (R, t).  A link that comes with a status, whose
// prior weight is not > 0, or whose S has a non-positive pivot gets lambda_p = 0.
__global__ __launch_bounds__(64) void joint_adj_solve_kernel(const double* __restrict__ Sm, const double* __restrict__ motion,
                                                              const double* __restrict__ grad_motion, const double* __restrict__ rgb2imu,
                                                              const double* __restrict__ prior_weight, const int* __restrict__ status_in,
                                                              const double* __restrict__ partial6, double* __restrict__ lambda_p,
                                                              int* __restrict__ status_out) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ double Hn[36], un[6], vn[6], L[6][6], x[6];
    __shared__ int st;
    if (i < 36) Hn[i] = Sm[(size_t)b * 36 + i];
    if (i >= 36 && i < 42) {
        double v = 0.0;
        if (partial6)
            for (int k = 0; k < NBLK; ++k) v += partial6[((size_t)b * NBLK + k) * 6 + (i - 36)];
        un[i - 36] = v;
    }
    __syncthreads();
    if (i == 0) {
        const SE3<double> X = se3_load(motion + (size_t)b * 7);
        const double* gm = grad_motion + (size_t)b * 7;
        V3<double> vr = tmul(qmat(X.q), v3(gm[0], gm[1], gm[2]));
        const V3<double> qv{X.q.x, X.q.y, X.q.z}, gq{gm[3], gm[4], gm[5]};
        V3<double> vf = 0.5 * (X.q.w * gq - cross(qv, gq) - gm[6] * qv);
        V3<double> ur{un[0], un[1], un[2]}, uf{un[3], un[4], un[5]};
        if (rgb2imu) {
            const SE3<double> Ci = se3_inv(se3_load(rgb2imu));
            const M3<double> Rc = qmat(Ci.q);
            uf = tmul(Rc, uf - cross(Ci.t, ur));
            ur = tmul(Rc, ur);
        }
        vr = vr - ur;
        vf = vf - uf;
        vn[0] = vr.x; vn[1] = vr.y; vn[2] = vr.z; vn[3] = vf.x; vn[4] = vf.y; vn[5] = vf.z;
        int s = status_in ? status_in[b] : ISLAM_DENSE_REPROJ_OK;
        if (s == ISLAM_DENSE_REPROJ_OK && !(prior_weight[b] > 0.0)) s = ISLAM_DENSE_REPROJ_BADPRIOR;
        if (s == ISLAM_DENSE_REPROJ_OK && !lm_step(Hn, vn, 0.0, L, x)) s = ISLAM_DENSE_REPROJ_NOTPD;
        st = s;
        status_out[b] = s;
    }
    __syncthreads();
    if (i < 6) lambda_p[(size_t)b * 6 + i] = st == ISLAM_DENSE_REPROJ_OK ? x[i] : 0.0;
}

__global__ __launch_bounds__(256) void joint_adj_vjp_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                             const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                             const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                             const double* __restrict__ prior_weight, const double* __restrict__ inv_depth,
                                                             const double* __restrict__ lambda_p, const double* __restrict__ grad_rho,
                                                             const int* __restrict__ status, float* __restrict__ grad_depth,
                                                             float* __restrict__ grad_flow, int H, int W, int kind, double delta) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const size_t off = (size_t)b * HW;
    float* gzp = grad_depth + off;
    float* gup = grad_flow + 2 * off;
    float* gvp = gup + HW;
    const double w = prior_weight[b];
    if (!(w > 0.0) || (status && status[b] != ISLAM_DENSE_REPROJ_OK)) {      // a link without a gradient: zeros, whatever its pixels hold
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) gzp[i] = gup[i] = gvp[i] = 0.0f;
        return;
    }
    const Intr in = intr_load(intr4 + 4 * b);
    const double d2 = delta * delta;
    __shared__ double Tp[12], lcam[6];
    if (threadIdx.x == 0) {
        pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
        const double* lp = lambda_p + 6 * b;
        V3<double> lr{lp[0], lp[1], lp[2]}, lf{lp[3], lp[4], lp[5]};
        adjoint_apply(rgb2imu, lr, lf);      // lambda_cam = Ad(C^-1) lambda_p
        lcam[0] = lr.x; lcam[1] = lr.y; lcam[2] = lr.z; lcam[3] = lf.x; lcam[4] = lf.y; lcam[5] = lf.z;
    }
    __syncthreads();
    const M3<double> R = m3_load(Tp);
    const V3<double> t{Tp[9], Tp[10], Tp[11]};
    const float* zp = depth + off;
    const float* fup = flow + 2 * off;
    const float* fvp = fup + HW;
    const uint8_t* mp = mask ? mask + off : nullptr;
    const double* rp = inv_depth + off;
    const double* vp = grad_rho ? grad_rho + off : nullptr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const int v = i / W, u = i - v * W;
        const double ud = (double)u, vd = (double)v;
        const double z = (double)zp[i];
        double gz = 0.0, gu = 0.0, gv = 0.0;
        if (isfinite(z) && z > 0.0) {      // the pixel has a prior
            const double rho = rp[i];
            const double vdi = vp ? vp[i] : 0.0;
            double ld = -vdi / w;          // c = 0: an invalid pixel follows its prior
            if (isfinite(rho) && rho > 0.0) {
                const BaPixel p = ba_pixel(R, t, rho, (ud - in.cx) / in.fx, (vd - in.cy) / in.fy, (double)fup[i] + ud, (double)fvp[i] + vd,
                                           mp ? mp[i] != 0 : true, in, kind, delta, d2);
                if (p.p.valid) {
                    const double c = p.p.c, ru = p.p.ru, rv = p.p.rv;
                    const double eu = c * p.jdu, ev = c * p.jdv;
                    double du = 0.0, dv = 0.0;      // J_cam lambda_cam
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        du += p.p.ju[q] * lcam[q];
                        dv += p.p.jv[q] * lcam[q];
                    }
                    ld = -(vdi + (eu * du + ev * dv)) / (eu * p.jdu + ev * p.jdv + w);
                    const double qu = du + p.jdu * ld, qv = dv + p.jdv * ld;
                    const double k2 = 2.0 * p.p.cp * (qu * ru + qv * rv);
                    gu = -(c * qu + k2 * ru);
                    gv = -(c * qv + k2 * rv);
                }
            }
            gz = w * ld / (z * z);
        }
        gzp[i] = (float)gz;
        gup[i] = (float)gu;
        gvp[i] = (float)gv;
    }
}

}  // namespace

extern "C" size_t islam_dense_ba_adjoint_scratch_bytes(int B) {
    if (B < 1) return 0;
    return align_up((size_t)B * NBLK * 6 * sizeof(double));
}

extern "C" int islam_dense_ba_ift_weights(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                          const double* rgb2imu, const double* intr4, const double* prior_weight, const double* inv_depth,
                                          int robust_kind, double robust_delta, const double* S, const double* grad_motion,
                                          const double* grad_inv_depth_or_null, const int* status_in_or_null, void* scratch, int B, int H,
                                          int W, double* lambda_p, int* status_out, void* stream) {
    const char* who = "islam_dense_ba_ift_weights";
    if (int rc = check_shape_kind(who, B, H, W, robust_kind, robust_delta)) return rc;
    if (!depth || !flow || !motion || !intr4 || !scratch)
        return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 / scratch pointer", who);
    if (!prior_weight) return fail(ISLAM_EARG, "%s: NULL prior_weight", who);
    if (!inv_depth || !S || !grad_motion || !lambda_p || !status_out)
        return fail(ISLAM_EARG, "%s: NULL inv_depth / S / grad_motion / lambda_p / status_out pointer", who);
    hipStream_t s = as_stream(stream);
    double* partial6 = static_cast<double*>(scratch);
    if (grad_inv_depth_or_null)
        hipLaunchKernelGGL(joint_adj_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu, intr4, prior_weight,
                           inv_depth, grad_inv_depth_or_null, status_in_or_null, partial6, H, W, robust_kind, robust_delta);
    hipLaunchKernelGGL(joint_adj_solve_kernel, dim3(B), dim3(64), 0, s, S, motion, grad_motion, rgb2imu, prior_weight, status_in_or_null,
                       grad_inv_depth_or_null ? partial6 : nullptr, lambda_p, status_out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" int islam_dense_ba_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion, const double* rgb2imu,
                                  const double* intr4, const double* prior_weight, const double* inv_depth, int robust_kind,
                                  double robust_delta, const double* lambda_p, const double* grad_inv_depth_or_null,
                                  const int* status_or_null, float* grad_depth, float* grad_flow, int B, int H, int W, void* stream) {
    const char* who = "islam_dense_ba_vjp";
    if (int rc = check_shape_kind(who, B, H, W, robust_kind, robust_delta)) return rc;
    if (!depth || !flow || !motion || !intr4) return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 pointer", who);
    if (!prior_weight) return fail(ISLAM_EARG, "%s: NULL prior_weight", who);
    if (!inv_depth || !lambda_p || !grad_depth || !grad_flow)
        return fail(ISLAM_EARG, "%s: NULL inv_depth / lambda_p / grad_depth / grad_flow pointer", who);
    hipLaunchKernelGGL(joint_adj_vjp_kernel, dim3(NBLK, B), dim3(256), 0, as_stream(stream), depth, flow, mask, motion, rgb2imu, intr4,
                       prior_weight, inv_depth, lambda_p, grad_inv_depth_or_null, status_or_null, grad_depth, grad_flow, H, W, robust_kind,
                       robust_delta);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}
