// Joint two-view dense bundle adjustment on gfx950: the pose of a link and one inverse depth per pixel, the stereo depth as a
// Gaussian prior, the depths eliminated pixel by pixel (definitions: include/islam_hip.h, "dense reprojection"; DESIGN.md section
// 3.25).  It stands beside dense_reproj.hip and shares its pixel loop head (pixel_in), per-pixel front (reproj_pixel), reduction
// epilogue, final-kernel body, Cholesky step, sum layout and host-side argument checks (dense_reproj_dev.h).
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
// joint_adj_vjp_kernel), and per-pixel prior weights with the posterior variance of the inverse depths
// (ba_wmap_partial_kernel beside the partial kernel; depth_var_factor_kernel, depth_var_pixel_kernel; section 3.27).  At the end: the
// same gradient with the exact (Newton) Hessian and per-pixel prior weights (ba_newton_partial_kernel, ba_newton_solve_kernel,
// ba_newton_vjp_kernel; section 3.30).  Between the two: the gradient of the posterior variance in the state (depth_var_adj_partial_kernel,
// depth_var_vjp_kernel, depth_var_pose_kernel; section 3.32).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "common.h"
#include "dense_reproj_dev.h"
#include "lie_dev.h"
#include "lie_vjp_dev.h"

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

// everything of one pixel at (T^-1 = (R, t), rho) that the sums and the back-substitution need: the shared front at z = 1 / rho,
// jd = dr/drho = dr/dQ R ray (-1/rho^2), and the depth row e = c jd, h_dd = e.jd + w
struct BaPixel {
    Pixel p;
    double jdu, jdv, eu, ev, hdd;
};

ISLAM_DEV BaPixel ba_pixel(const M3<double>& R, const V3<double>& t, double rho, const PixelIn& px, const LinkPixels& lp, double w) {
    BaPixel b;
    const double zi = 1.0 / rho;
    b.p = reproj_pixel(R, t, zi, px, lp);
    const V3<double> dR = R * V3<double>{px.xh, px.yh, 1.0};      // dQ/d(1/rho)
    const double k = -(zi * zi);
    b.jdu = (b.p.a * dR.x + b.p.bq * dR.z) * k;
    b.jdv = (b.p.cq * dR.y + b.p.dq * dR.z) * k;
    b.eu = b.p.c * b.jdu;
    b.ev = b.p.c * b.jdv;
    b.hdd = b.eu * b.jdu + b.ev * b.jdv + w;
    return b;
}

ISLAM_DEV void pose_to_lds(const SE3<double>& Ti, double* dst) {
    m3_store(qmat(Ti.q), dst);
    dst[9] = Ti.t.x;
    dst[10] = Ti.t.y;
    dst[11] = Ti.t.z;
}

// a pixel's prior under a weight map (section 3.27): usable iff the depth is AND m_i is finite and > 0, w_i = w_b (double)m_i, one rounding
ISLAM_DEV bool map_prior(const float* __restrict__ scale, int i, double wb, bool prior, double& w) {
    const double m = (double)scale[i];
    w = wb * m;
    return prior && isfinite(m) && m > 0.0;
}

// The body of the two partial kernels.  MAP = false is dense_ba_partial_kernel as section 3.25 describes it, one prior weight per link;
// MAP = true (ba_wmap_partial_kernel, section 3.27) reads prior_scale (B,H,W) float32 beside the depth, and the pixel's w_i = w_b m_i
// stands wherever w does.  A pixel whose m_i is not finite or is <= 0 has no usable prior, like one whose depth is <= 0.
template <bool MAP>
ISLAM_DEV void ba_partial_body(const float* __restrict__ depth, const float* __restrict__ flow, const uint8_t* __restrict__ mask,
                               const double* __restrict__ pose7, const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                               const double* __restrict__ prior_weight, const float* __restrict__ prior_scale,
                               double* __restrict__ partial, int H, int W, int kind, double delta, const RhoState& rs) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const double wb = prior_weight[b];
    const bool wok = wb > 0.0;
    // the back-substitution sweep runs at the current pose (Tp[0]), the sums at the pose under evaluation (Tp[1])
    const bool backsub = rs.eval >= 1 && rs.status[b] == ISLAM_DENSE_REPROJ_OK;
    __shared__ double Tp[2][12], dcam[6];
    if (threadIdx.x == 0) {
        pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp[1]);
        if (backsub) {
            pose_to_lds(camera_inverse(rs.cur_pose + 7 * b, rgb2imu), Tp[0]);
            adjoint_to_camera(rgb2imu, rs.delta + 6 * b, dcam);      // delta_cam = Ad(C^-1) delta
        }
    }
    __syncthreads();

    const size_t off = (size_t)b * HW;
    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    const float* ms = MAP ? prior_scale + off : nullptr;
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
            const PixelIn px = pixel_in(lp, i);
            bool prior = isfinite(px.z) && px.z > 0.0;
            double w = wb;
            if constexpr (MAP) prior = map_prior(ms, i, wb, prior, w);
            const double rho0 = prior ? 1.0 / px.z : 0.0;
            const double rho = rcur[i];
            double trial = rho0;
            if (prior && rho > 0.0) {
                const BaPixel p = ba_pixel(R, t, rho, px, lp, w);
                if (p.p.valid) {
                    const double gd = p.eu * p.p.ru + p.ev * p.p.rv + w * (rho - rho0);
                    // J_cam delta_cam, here and not in a function shared with joint_adj_vjp_kernel: behind one the compiler swaps the two
                    // products of e.(J_cam delta_cam) before it fuses one of them, and the trial rho moves in its last bit
                    double du = 0.0, dv = 0.0;
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        du += p.p.ju[q] * dcam[q];
                        dv += p.p.jv[q] * dcam[q];
                    }
                    trial = rho - (gd + (p.eu * du + p.ev * dv)) / p.hdd;
                    if (!(isfinite(trial) && trial > 0.0)) trial = rho;
                }
            }
            rnext[i] = trial;
        }
    }

    // Second sweep: the sums at the pose under evaluation and at the trial rho (each thread reads back what it wrote itself), or at
    // the state as given.  This is the only code that forms the sums, so islam_dense_ba_normal repeats a refinement's bits.
    double acc[NS] = {};
    const double* rsrc = backsub ? rnext : rcur;
    const M3<double> R = m3_load(Tp[1]);
    const V3<double> t{Tp[1][9], Tp[1][10], Tp[1][11]};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const PixelIn px = pixel_in(lp, i);
        bool prior = isfinite(px.z) && px.z > 0.0;
        double w = wb;
        if constexpr (MAP) prior = map_prior(ms, i, wb, prior, w);
        const double rho0 = prior ? 1.0 / px.z : 0.0;
        const double rho = rsrc ? rsrc[i] : rho0;
        if (rs.eval == 0) rnext[i] = rho0;
        if (!(prior && wok && isfinite(rho) && rho > 0.0)) continue;      // outside the valid set at every state
        const BaPixel p = ba_pixel(R, t, rho, px, lp, w);
        if (!p.p.valid) continue;
        const double c = p.p.c, ru = p.p.ru, rv = p.p.rv;
        // with e = c jd:  h_pd = J_cam^T e,  h_dd = e.jd + w,  g_d = e.r + w (rho - rho0).  The pixel's Schur term takes the shape of
        // section 3.23's: c J^T J - h_pd h_pd^T / h_dd = J^T M J with the 2x2 M = c I - e e^T / h_dd, and
        // c J^T r - h_pd g_d / h_dd = J^T (c r - e g_d / h_dd)
        const double eu = p.eu, ev = p.ev;
        const double dprior = rho - rho0;
        const double gd = eu * ru + ev * rv + w * dprior;
        const double ih = 1.0 / p.hdd;
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
    reduce_and_store_row<NS>(acc, partial + ((size_t)b * NBLK + blockIdx.x) * NS, wok, NAN);
}

__global__ __launch_bounds__(256) void dense_ba_partial_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                                const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                                const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                                const double* __restrict__ prior_weight, double* __restrict__ partial,
                                                                int H, int W, int kind, double delta, RhoState rs) {
    ba_partial_body<false>(depth, flow, mask, pose7, rgb2imu, intr4, prior_weight, nullptr, partial, H, W, kind, delta, rs);
}

__global__ __launch_bounds__(256) void ba_wmap_partial_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                               const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                               const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                               const double* __restrict__ prior_weight,
                                                               const float* __restrict__ prior_scale, double* __restrict__ partial, int H,
                                                               int W, int kind, double delta, RhoState rs) {
    ba_partial_body<true>(depth, flow, mask, pose7, rgb2imu, intr4, prior_weight, prior_scale, partial, H, W, kind, delta, rs);
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


// The scratch of the joint entry points, in one place: the partial sums, and for a refinement the trial pose, the pose step, the
// selector and the two inverse-depth buffers.  bytes: where the layout ends; base == nullptr serves to size it.
struct JointScratch {
    double *partial, *trial, *step;
    int* select;
    double *buf0, *buf1;
    size_t bytes;
};

JointScratch joint_scratch(void* base, int B, int H, int W, bool refine) {
    JointScratch js{};
    auto carve = [&](auto*& p, size_t count) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(base) + js.bytes);
        js.bytes += align_up(count * sizeof(*p));
    };
    carve(js.partial, (size_t)B * NBLK * NS);
    if (refine) {
        carve(js.trial, (size_t)B * 7);
        carve(js.step, (size_t)B * 6);
        carve(js.select, (size_t)B);
        carve(js.buf0, (size_t)B * H * W);
        carve(js.buf1, (size_t)B * H * W);
    }
    return js;
}

// one launch of the partial kernel: with a weight map the map kernel, else the kernel of section 3.25
void launch_partial(hipStream_t s, const float* depth, const float* flow, const uint8_t* mask, const double* pose, const double* rgb2imu,
                    const double* intr4, const double* prior_weight, const float* prior_scale, double* partial, int B, int H, int W, int kind,
                    double delta, const RhoState& rs) {
    if (prior_scale)
        hipLaunchKernelGGL(ba_wmap_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, pose, rgb2imu, intr4, prior_weight,
                           prior_scale, partial, H, W, kind, delta, rs);
    else
        hipLaunchKernelGGL(dense_ba_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, pose, rgb2imu, intr4, prior_weight,
                           partial, H, W, kind, delta, rs);
}

// islam_dense_ba_normal and islam_dense_ba_normal_map (map: the entry point takes a weight map, and a NULL one is an error)
int normal_entry(const char* who, bool map, const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                 const double* rgb2imu, const double* intr4, const double* prior_weight, const float* prior_scale,
                 const double* inv_depth_or_null, int robust_kind, double robust_delta, const Outputs& o, void* scratch, int B, int H, int W,
                 void* stream) {
    if (int rc = check_common(who, depth, flow, motion, intr4, robust_kind, robust_delta, o, scratch, B, H, W, prior_weight != nullptr))
        return rc;
    if (map && !prior_scale) return fail(ISLAM_EARG, "%s: NULL prior_scale", who);
    hipStream_t s = as_stream(stream);
    const JointScratch js = joint_scratch(scratch, B, H, W, false);
    RhoState rs{};
    rs.given = inv_depth_or_null;
    rs.eval = -1;
    launch_partial(s, depth, flow, mask, motion, rgb2imu, intr4, prior_weight, prior_scale, js.partial, B, H, W, robust_kind, robust_delta, rs);
    hipLaunchKernelGGL(dense_ba_final_kernel, dim3(B), dim3(64), 0, s, js.partial, rgb2imu, motion, o, Refine{}, Joint{}, B);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// islam_dense_ba_refine and islam_dense_ba_refine_map; rf as the entry point filled it
int refine_entry(const char* who, bool map, const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                 const double* rgb2imu, const double* intr4, const double* prior_weight, const float* prior_scale, int robust_kind,
                 double robust_delta, int iters, Refine rf, const double* trace, double* out_inv_depth, const Outputs& o, void* scratch, int B,
                 int H, int W, void* stream) {
    if (int rc = check_common(who, depth, flow, motion, intr4, robust_kind, robust_delta, o, scratch, B, H, W, prior_weight != nullptr))
        return rc;
    if (int rc = check_refine(who, iters, rf, trace)) return rc;
    if (!out_inv_depth) return fail(ISLAM_EARG, "%s: NULL out_inv_depth", who);
    if (map && !prior_scale) return fail(ISLAM_EARG, "%s: NULL prior_scale", who);
    hipStream_t s = as_stream(stream);
    const JointScratch js = joint_scratch(scratch, B, H, W, true);
    rf.trial = js.trial;
    const Joint jt{prior_weight, js.step, js.select};
    RhoState rs{nullptr, js.buf0, js.buf1, js.select, rf.status, rf.motion, js.step, 0};
    for (int k = 0; k < iters; ++k) {
        const double* pose = k == 0 ? motion : js.trial;
        rf.eval = rs.eval = k;
        rf.last = k == iters - 1;
        launch_partial(s, depth, flow, mask, pose, rgb2imu, intr4, prior_weight, prior_scale, js.partial, B, H, W, robust_kind, robust_delta, rs);
        hipLaunchKernelGGL(dense_ba_final_kernel, dim3(B), dim3(64), 0, s, js.partial, rgb2imu, pose, o, rf, jt, B);
    }
    hipLaunchKernelGGL(dense_ba_gather_kernel, dim3(NBLK, B), dim3(256), 0, s, js.buf0, js.buf1, js.select, out_inv_depth, H * W);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

}  // namespace

extern "C" size_t islam_dense_ba_scratch_bytes(int B, int H, int W, int iters_or_0) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return joint_scratch(nullptr, B, H, W, iters_or_0 > 0).bytes;
}

extern "C" int islam_dense_ba_normal(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                     const double* rgb2imu, const double* intr4, const double* prior_weight,
                                     const double* inv_depth_or_null, int robust_kind, double robust_delta, double* out_S, double* out_g,
                                     double* out_cost, double* out_l1, double* out_count, double* out_sums, void* scratch, int B, int H,
                                     int W, void* stream) {
    return normal_entry("islam_dense_ba_normal", false, depth, flow, mask, motion, rgb2imu, intr4, prior_weight, nullptr, inv_depth_or_null,
                        robust_kind, robust_delta, Outputs{out_S, out_g, out_cost, out_l1, out_count, out_sums}, scratch, B, H, W, stream);
}

extern "C" int islam_dense_ba_normal_map(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                         const double* rgb2imu, const double* intr4, const double* prior_weight, const float* prior_scale,
                                         const double* inv_depth_or_null, int robust_kind, double robust_delta, double* out_S,
                                         double* out_g, double* out_cost, double* out_l1, double* out_count, double* out_sums, void* scratch,
                                         int B, int H, int W, void* stream) {
    return normal_entry("islam_dense_ba_normal_map", true, depth, flow, mask, motion, rgb2imu, intr4, prior_weight, prior_scale,
                        inv_depth_or_null, robust_kind, robust_delta, Outputs{out_S, out_g, out_cost, out_l1, out_count, out_sums}, scratch, B,
                        H, W, stream);
}

extern "C" int islam_dense_ba_refine(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                     const double* rgb2imu, const double* intr4, const double* prior_weight, int robust_kind,
                                     double robust_delta, int iters, double damping, double min_count, double* out_motion,
                                     double* out_inv_depth, double* out_S, double* out_g, double* out_cost, double* out_l1,
                                     double* out_count, double* out_sums, double* out_lambda, int* out_accepted, int* out_rejected,
                                     int* out_status, double* trace, int trace_cap, void* scratch, int B, int H, int W, void* stream) {
    const Refine rf{out_motion, nullptr, out_lambda, out_accepted, out_rejected, out_status, trace_cap > 0 ? trace : nullptr, trace_cap, 0, 0,
                    min_count, damping};
    return refine_entry("islam_dense_ba_refine", false, depth, flow, mask, motion, rgb2imu, intr4, prior_weight, nullptr, robust_kind,
                        robust_delta, iters, rf, trace, out_inv_depth, Outputs{out_S, out_g, out_cost, out_l1, out_count, out_sums}, scratch, B,
                        H, W, stream);
}

extern "C" int islam_dense_ba_refine_map(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                         const double* rgb2imu, const double* intr4, const double* prior_weight, const float* prior_scale,
                                         int robust_kind, double robust_delta, int iters, double damping, double min_count,
                                         double* out_motion, double* out_inv_depth, double* out_S, double* out_g, double* out_cost,
                                         double* out_l1, double* out_count, double* out_sums, double* out_lambda, int* out_accepted,
                                         int* out_rejected, int* out_status, double* trace, int trace_cap, void* scratch, int B, int H, int W,
                                         void* stream) {
    const Refine rf{out_motion, nullptr, out_lambda, out_accepted, out_rejected, out_status, trace_cap > 0 ? trace : nullptr, trace_cap, 0, 0,
                    min_count, damping};
    return refine_entry("islam_dense_ba_refine_map", true, depth, flow, mask, motion, rgb2imu, intr4, prior_weight, prior_scale, robust_kind,
                        robust_delta, iters, rf, trace, out_inv_depth, Outputs{out_S, out_g, out_cost, out_l1, out_count, out_sums}, scratch, B,
                        H, W, stream);
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
// joint_adj_vjp_kernel streams the two gradients out.  (tests/test_dense_reproj_cpu.py pins the family's ten kernel names.)
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
    double acc[6] = {};
    if (live) {
        __shared__ double Tp[12];
        if (threadIdx.x == 0) pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
        __syncthreads();
        const M3<double> R = m3_load(Tp);
        const V3<double> t{Tp[9], Tp[10], Tp[11]};
        const size_t off = (size_t)b * HW;
        const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
        const double* rp = inv_depth + off;
        const double* vp = grad_rho + off;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
            const PixelIn px = pixel_in(lp, i);
            const double rho = rp[i];
            if (!(isfinite(px.z) && px.z > 0.0 && isfinite(rho) && rho > 0.0)) continue;
            const BaPixel p = ba_pixel(R, t, rho, px, lp, w);
            if (!p.p.valid) continue;
            const double k = vp[i] / p.hdd;      // v_d / h_dd
#pragma unroll
            for (int l = 0; l < 6; ++l) acc[l] += (p.eu * p.p.ju[l] + p.ev * p.p.jv[l]) * k;
        }
    }
    reduce_and_store_row<6>(acc, partial6 + ((size_t)b * NBLK + blockIdx.x) * 6, live, 0.0);
}

// lambda_p per link.  v_p from the gradient on [t, q xyzw] as reproj_ift_kernel forms it (tangent_gradient); u_cam = the NBLK rows in
// fixed order (0 when the reduction did not run); A^T u by adjoint_apply<true>.  A link that comes with a status, whose prior weight is
// not > 0, or whose S has a non-positive pivot gets lambda_p = 0 (adjoint_solve_tail).
__global__ __launch_bounds__(64) void joint_adj_solve_kernel(const double* __restrict__ Sm, const double* __restrict__ motion,
                                                              const double* __restrict__ grad_motion, const double* __restrict__ rgb2imu,
                                                              const double* __restrict__ prior_weight, const int* __restrict__ status_in,
                                                              const double* __restrict__ partial6, double* __restrict__ lambda_p,
                                                              int* __restrict__ status_out) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ double Hn[36], un[6], vn[6], L[6][6], x[6];
    if (i < 36) Hn[i] = Sm[(size_t)b * 36 + i];
    if (i >= 36 && i < 42) {
        double v = 0.0;
        if (partial6)
            for (int k = 0; k < NBLK; ++k) v += partial6[((size_t)b * NBLK + k) * 6 + (i - 36)];
        un[i - 36] = v;
    }
    __syncthreads();
    if (i == 0) {
        V3<double> vr, vf;
        tangent_gradient(motion + (size_t)b * 7, grad_motion + (size_t)b * 7, vr, vf);
        V3<double> ur{un[0], un[1], un[2]}, uf{un[3], un[4], un[5]};
        adjoint_apply<true>(rgb2imu, ur, uf);      // A^T u_cam
        vr = vr - ur;      // into registers first: through vn the compiler splits the FMAs of v_phi - u_phi, and lambda_p's last bits move
        vf = vf - uf;
        vn[0] = vr.x; vn[1] = vr.y; vn[2] = vr.z; vn[3] = vf.x; vn[4] = vf.y; vn[5] = vf.z;
    }
    int s = status_in ? status_in[b] : ISLAM_DENSE_REPROJ_OK;
    if (s == ISLAM_DENSE_REPROJ_OK && !(prior_weight[b] > 0.0)) s = ISLAM_DENSE_REPROJ_BADPRIOR;
    adjoint_solve_tail(s, Hn, vn, L, x, status_out + b, lambda_p + (size_t)b * 6);
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
    const LinkGrads out = link_grads(grad_depth, grad_flow, b, HW);
    const double w = prior_weight[b];
    if (!(w > 0.0) || (status && status[b] != ISLAM_DENSE_REPROJ_OK)) return grad_zero_link(out, HW);      // a link without a gradient
    __shared__ double Tp[12], lcam[6];
    if (threadIdx.x == 0) {
        pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
        adjoint_to_camera(rgb2imu, lambda_p + 6 * b, lcam);      // lambda_cam = Ad(C^-1) lambda_p
    }
    __syncthreads();
    const M3<double> R = m3_load(Tp);
    const V3<double> t{Tp[9], Tp[10], Tp[11]};
    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    const double* rp = inv_depth + off;
    const double* vp = grad_rho ? grad_rho + off : nullptr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const PixelIn px = pixel_in(lp, i);
        const double z = px.z;
        double gz = 0.0, gu = 0.0, gv = 0.0;
        if (isfinite(z) && z > 0.0) {      // the pixel has a prior
            const double rho = rp[i];
            const double vdi = vp ? vp[i] : 0.0;
            double ld = -vdi / w;          // c = 0: an invalid pixel follows its prior
            if (isfinite(rho) && rho > 0.0) {
                const BaPixel p = ba_pixel(R, t, rho, px, lp, w);
                if (p.p.valid) {
                    const double c = p.p.c, ru = p.p.ru, rv = p.p.rv;
                    double du = 0.0, dv = 0.0;      // J_cam lambda_cam
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        du += p.p.ju[q] * lcam[q];
                        dv += p.p.jv[q] * lcam[q];
                    }
                    ld = -(vdi + (p.eu * du + p.ev * dv)) / p.hdd;
                    const double qu = du + p.jdu * ld, qv = dv + p.jdv * ld;
                    const double k2 = 2.0 * p.p.cp * (qu * ru + qv * rv);
                    gu = -(c * qu + k2 * ru);
                    gv = -(c * qv + k2 * rv);
                }
            }
            gz = w * ld / (z * z);
        }
        grad_store(out, i, gz, gu, gv);
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
    if (int rc = check_joint_adjoint(who, depth, flow, motion, intr4, prior_weight, inv_depth, lambda_p, robust_kind, robust_delta, B, H, W))
        return rc;
    if (!S || !grad_motion || !status_out || !scratch) return fail(ISLAM_EARG, "%s: NULL S / grad_motion / status_out / scratch pointer", who);
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
    if (int rc = check_joint_adjoint(who, depth, flow, motion, intr4, prior_weight, inv_depth, lambda_p, robust_kind, robust_delta, B, H, W))
        return rc;
    if (!grad_depth || !grad_flow) return fail(ISLAM_EARG, "%s: NULL grad_depth / grad_flow pointer", who);
    hipLaunchKernelGGL(joint_adj_vjp_kernel, dim3(NBLK, B), dim3(256), 0, as_stream(stream), depth, flow, mask, motion, rgb2imu, intr4,
                       prior_weight, inv_depth, lambda_p, grad_inv_depth_or_null, status_or_null, grad_depth, grad_flow, H, W, robust_kind,
                       robust_delta);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// ------------------------------------------------------------------ the posterior variance of the inverse depths
//   At a state (pose, rho), in units of sigma_px^2 and in the Gauss-Newton approximation with the robust
// weight c, with h_cam = J_cam^T e (= h_pd), h_dd = e.jd + w_i as ba_pixel forms them and S_cam the first 21 sums of the same state:
//   marginal over the pose:   v_i = 1 / h_dd + h_cam^T S_cam^-1 h_cam / h_dd^2        conditional on the pose:   v_i = 1 / h_dd
//   a pixel with a prior that is invalid at the state (c = 0):  v_i = 1 / w_i;   no usable prior, or rho not finite or <= 0:  NaN.
// depth_var_factor_kernel inverts S_cam per link and forms the link's status, depth_var_pixel_kernel streams the map out: one 8-byte
// store per pixel, no reduction, no atomics.  (Their names stay clear of the family's ten, which tests/test_dense_reproj_cpu.py pins.)
namespace {

// One 64-lane workgroup per link.  status: the incoming one if set, BADPRIOR for a prior weight that is not > 0, NOTPD for a sum that
// is not finite or (marginal mode) a non-positive pivot, else OK.  Marginal mode: lane k solves S_cam x = e_k by the header's Cholesky
// (six factorisations side by side, everything runtime-indexed in LDS) and the upper triangle of S_cam^-1 goes to sinv (B,21).
__global__ __launch_bounds__(64) void depth_var_factor_kernel(const double* __restrict__ sums, const double* __restrict__ prior_weight,
                                                               const int* __restrict__ status_in, int marginal,
                                                               double* __restrict__ sinv, int* __restrict__ status_out) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ double Hn[36], gn[6][6], L[6][6][6], x[6][6];
    __shared__ int bad;
    if (i == 0) bad = 0;
    if (i < 36) {
        const int r = i / 6, c = i - 6 * r;
        Hn[i] = sums[(size_t)b * NS + tri(min(r, c), max(r, c))];
        gn[r][c] = r == c ? -1.0 : 0.0;      // lm_step solves H x = -g
    }
    __syncthreads();
    int s = status_in ? status_in[b] : ISLAM_DENSE_REPROJ_OK;
    if (s == ISLAM_DENSE_REPROJ_OK && !(prior_weight[b] > 0.0)) s = ISLAM_DENSE_REPROJ_BADPRIOR;
    if (i < 36 && !isfinite(Hn[i])) bad = 1;
    if (marginal && s == ISLAM_DENSE_REPROJ_OK && i < 6 && !lm_step(Hn, gn[i], 0.0, L[i], x[i])) bad = 1;
    __syncthreads();
    if (s == ISLAM_DENSE_REPROJ_OK && bad) s = ISLAM_DENSE_REPROJ_NOTPD;
    if (i == 0) status_out[b] = s;
    if (marginal && i < 36) {
        const int r = i / 6, c = i - 6 * r;
        if (r <= c) sinv[(size_t)b * 21 + tri(r, c)] = s == ISLAM_DENSE_REPROJ_OK ? x[c][r] : NAN;
    }
}

// grid (NBLK, B) x 256, grid-stride.  A link whose status is set gets NaN at every pixel.
__global__ __launch_bounds__(256) void depth_var_pixel_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                               const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                               const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                               const double* __restrict__ prior_weight,
                                                               const float* __restrict__ prior_scale, const double* __restrict__ inv_depth,
                                                               const double* __restrict__ sinv, const int* __restrict__ status,
                                                               double* __restrict__ out_var, int H, int W, int kind, double delta,
                                                               int marginal) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const size_t off = (size_t)b * HW;
    double* out = out_var + off;
    if (status[b] != ISLAM_DENSE_REPROJ_OK) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) out[i] = NAN;
        return;
    }
    __shared__ double Tp[12], Si[21];
    if (threadIdx.x == 0) pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
    if (marginal && threadIdx.x >= 64 && threadIdx.x < 64 + 21) Si[threadIdx.x - 64] = sinv[(size_t)b * 21 + threadIdx.x - 64];
    __syncthreads();
    const M3<double> R = m3_load(Tp);
    const V3<double> t{Tp[9], Tp[10], Tp[11]};
    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    const double wb = prior_weight[b];
    const float* ms = prior_scale ? prior_scale + off : nullptr;
    const double* rp = inv_depth ? inv_depth + off : nullptr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const PixelIn px = pixel_in(lp, i);
        bool prior = isfinite(px.z) && px.z > 0.0;
        double w = wb;
        if (ms) prior = map_prior(ms, i, wb, prior, w);
        const double rho = rp ? rp[i] : (prior ? 1.0 / px.z : 0.0);
        double v = NAN;
        if (prior && isfinite(rho) && rho > 0.0) {
            v = 1.0 / w;      // c = 0: only the prior speaks
            const BaPixel p = ba_pixel(R, t, rho, px, lp, w);
            if (p.p.valid) {
                const double ih = 1.0 / p.hdd;
                v = ih;
                if (marginal) {
                    double h[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) h[q] = p.eu * p.p.ju[q] + p.ev * p.p.jv[q];
                    double quad = 0.0;      // h^T S_cam^-1 h over the stored upper triangle
                    int k = 0;
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        double row = 0.0;
#pragma unroll
                        for (int l = q; l < 6; ++l) row += Si[k++] * (l == q ? h[l] : 2.0 * h[l]);
                        quad += h[q] * row;
                    }
                    v = ih + quad * ih * ih;
                }
            }
        }
        out[i] = v;
    }
}

}  // namespace

extern "C" size_t islam_dense_ba_depth_var_scratch_bytes(int B) {
    if (B < 1) return 0;
    return align_up((size_t)B * 21 * sizeof(double));
}

extern "C" int islam_dense_ba_depth_var(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                        const double* rgb2imu, const double* intr4, const double* prior_weight,
                                        const float* prior_scale_or_null, const double* inv_depth_or_null, const double* sums,
                                        const int* status_or_null, int robust_kind, double robust_delta, int mode, double* out_var,
                                        int* out_status, void* scratch, int B, int H, int W, void* stream) {
    const char* who = "islam_dense_ba_depth_var";
    if (int rc = check_shape_kind(who, B, H, W, robust_kind, robust_delta)) return rc;
    if (mode != 0 && mode != 1) return fail(ISLAM_EARG, "%s: mode must be 0 (marginal) or 1 (conditional), got %d", who, mode);
    if (!depth || !flow || !motion || !intr4) return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 pointer", who);
    if (!prior_weight) return fail(ISLAM_EARG, "%s: NULL prior_weight", who);
    if (!sums || !out_var || !out_status || !scratch) return fail(ISLAM_EARG, "%s: NULL sums / out_var / out_status / scratch pointer", who);
    hipStream_t s = as_stream(stream);
    double* sinv = static_cast<double*>(scratch);
    const int marginal = mode == 0;
    hipLaunchKernelGGL(depth_var_factor_kernel, dim3(B), dim3(64), 0, s, sums, prior_weight, status_or_null, marginal, sinv, out_status);
    hipLaunchKernelGGL(depth_var_pixel_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu, intr4, prior_weight,
                       prior_scale_or_null, inv_depth_or_null, sinv, out_status, out_var, H, W, robust_kind, robust_delta, marginal);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// ------------------------------------------------------------------ the gradient of the posterior variance
// (the formulas: include/islam_hip.h, islam_dense_ba_depth_var_vjp.)  The total derivative of v in the state
// (rho, motion, flow), S_cam being a function of the same state: with g_i the cotangent of v_i, a = J^T jd (h_cam = c a), k = |jd|^2,
// q = a^T S^-1 a, G = -sum g_i y_i y_i^T / h_dd^2 (y = c S^-1 a) the cotangent of S_cam, n = a^T G a and tau = <G, J^T J>, everything is
// the gradient of one scalar per valid pixel, phi = g (1 / h_dd + c^2 q / h_dd^2) + c tau - c^2 n / h_dd at fixed S^-1 and G.  The valid
// set and the branch of the Huber kernel are the forward pass's.  depth_var_adj_partial_kernel reduces the 21 sums of G (marginal mode
// only; one row per workgroup, plain stores), depth_var_vjp_kernel streams the gradients in rho and flow out and reduces the 12 sums of
// the cotangent of (R, t) = T^-1, depth_var_pose_kernel chains those to the plain components of motion.
namespace {

// y = S x for a symmetric 6x6 held as its row-major upper triangle (in LDS: every lane reads the same address)
ISLAM_DEV void symv6(const double* S, const double* x, double* y) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double v = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) v += S[r < c ? tri(r, c) : tri(c, r)] * x[c];
        y[r] = v;
    }
}

ISLAM_DEV double dot6(const double* x, const double* y) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) v += x[q] * y[q];
    return v;
}

// The pixel as depth_var_pixel_kernel takes it.  true: v_i is the valid row of the table (it depends on the state) and p holds its terms;
// false: v_i is 1 / w_i or NaN, a constant of the state.
ISLAM_DEV bool var_pixel(const M3<double>& R, const V3<double>& t, const LinkPixels& lp, const float* ms, const double* rp, double wb, int i,
                         PixelIn& px, double& rho, BaPixel& p) {
    px = pixel_in(lp, i);
    bool prior = isfinite(px.z) && px.z > 0.0;
    double w = wb;
    if (ms) prior = map_prior(ms, i, wb, prior, w);
    rho = rp[i];
    if (!(prior && isfinite(rho) && rho > 0.0)) return false;
    p = ba_pixel(R, t, rho, px, lp, w);
    return p.p.valid;
}

// grid (NBLK, B) x 256, grid-stride (marginal mode).  partial (B, NBLK, 21): the workgroup's sums of -g y y^T / h_dd^2 over its valid
// pixels, upper triangle.  A link whose status is set writes nothing: nobody reads its rows.
__global__ __launch_bounds__(256) void depth_var_adj_partial_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                                     const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                                     const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                                     const double* __restrict__ prior_weight,
                                                                     const float* __restrict__ prior_scale,
                                                                     const double* __restrict__ inv_depth, const double* __restrict__ sinv,
                                                                     const int* __restrict__ status, const double* __restrict__ grad_var,
                                                                     double* __restrict__ partial, int H, int W, int kind, double delta) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const size_t off = (size_t)b * HW;
    if (status[b] != ISLAM_DENSE_REPROJ_OK) return;
    __shared__ double Tp[12], Si[21];
    if (threadIdx.x == 0) pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + 21) Si[threadIdx.x - 64] = sinv[(size_t)b * 21 + threadIdx.x - 64];
    __syncthreads();
    const M3<double> R = m3_load(Tp);
    const V3<double> t{Tp[9], Tp[10], Tp[11]};
    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    const double wb = prior_weight[b];
    const float* ms = prior_scale ? prior_scale + off : nullptr;
    const double* rp = inv_depth + off;
    const double* gv = grad_var + off;
    double acc[21] = {};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        PixelIn px;
        BaPixel p;
        double rho;
        if (!var_pixel(R, t, lp, ms, rp, wb, i, px, rho, p)) continue;      // the cotangent is read at a valid pixel only: elsewhere it may be NaN
        double a[6], y[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) a[q] = p.p.ju[q] * p.jdu + p.p.jv[q] * p.jdv;
        symv6(Si, a, y);
        const double ih = 1.0 / p.hdd;
        const double coef = -(gv[i] * (p.p.c * ih) * (p.p.c * ih));
        int k = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double yq = coef * y[q];
#pragma unroll
            for (int l = q; l < 6; ++l) acc[k++] += yq * y[l];
        }
    }
    reduce_and_store_row<21>(acc, partial + ((size_t)b * NBLK + blockIdx.x) * 21, true, 0.0);
}

// grid (NBLK, B) x 256, grid-stride.  Per pixel: grad_inv_depth (one 8-byte store), grad_flow (two float stores); per workgroup one row
// of 12 in partial (B, NBLK, 12): the sums of the cotangent of R (row-major, m ray^T with m the cotangent of R ray) and of t.  gpart: the
// rows depth_var_adj_partial_kernel wrote, summed here in index order (marginal mode; conditional: G = 0 and S^-1 is not read).  A link
// whose status is set gets zeros at every pixel and writes no row.
__global__ __launch_bounds__(256) void depth_var_vjp_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                             const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                             const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                             const double* __restrict__ prior_weight, const float* __restrict__ prior_scale,
                                                             const double* __restrict__ inv_depth, const double* __restrict__ sinv,
                                                             const double* __restrict__ gpart, const int* __restrict__ status,
                                                             const double* __restrict__ grad_var, double* __restrict__ grad_inv_depth,
                                                             float* __restrict__ grad_flow, double* __restrict__ partial, int H, int W,
                                                             int kind, double delta, int marginal) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const size_t off = (size_t)b * HW;
    double* grho = grad_inv_depth + off;
    float* gfu = grad_flow + 2 * off;
    float* gfv = gfu + HW;
    if (status[b] != ISLAM_DENSE_REPROJ_OK) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
            grho[i] = 0.0;
            gfu[i] = gfv[i] = 0.0f;
        }
        return;
    }
    __shared__ double Tp[12], Si[21], Gb[21];
    if (threadIdx.x == 0) pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
    if (marginal && threadIdx.x >= 64 && threadIdx.x < 64 + 21) Si[threadIdx.x - 64] = sinv[(size_t)b * 21 + threadIdx.x - 64];
    if (marginal && threadIdx.x >= 128 && threadIdx.x < 128 + 21) {
        double v = 0.0;
        for (int k = 0; k < NBLK; ++k) v += gpart[((size_t)b * NBLK + k) * 21 + threadIdx.x - 128];
        Gb[threadIdx.x - 128] = v;
    }
    __syncthreads();
    const M3<double> R = m3_load(Tp);
    const V3<double> t{Tp[9], Tp[10], Tp[11]};
    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    const double wb = prior_weight[b];
    const float* ms = prior_scale ? prior_scale + off : nullptr;
    const double* rp = inv_depth + off;
    const double* gv = grad_var + off;
    double acc[12] = {};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        PixelIn px;
        BaPixel p;
        double rho;
        double g_rho = 0.0, g_fu = 0.0, g_fv = 0.0;      // exact zeros where v is a constant of the state or NaN
        if (var_pixel(R, t, lp, ms, rp, wb, i, px, rho, p)) {
            const double g = gv[i];
            const double* ju = p.p.ju;
            const double* jv = p.p.jv;
            const double c = p.p.c, jdu = p.jdu, jdv = p.jdv;
            const double ih = 1.0 / p.hdd, ih2 = ih * ih, c2 = c * c;
            const double kk = jdu * jdu + jdv * jdv;
            // phi and its partials; in conditional mode q = n = tau = 0 and the cotangent of a vanishes
            double ab[6] = {}, Gu[6] = {}, Gv[6] = {};
            double qq = 0.0, n = 0.0, tau = 0.0;
            if (marginal) {
                double a[6], Sa[6], Ga[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) a[q] = ju[q] * jdu + jv[q] * jdv;
                symv6(Si, a, Sa);
                symv6(Gb, ju, Gu);
                symv6(Gb, jv, Gv);
#pragma unroll
                for (int q = 0; q < 6; ++q) Ga[q] = jdu * Gu[q] + jdv * Gv[q];
                qq = dot6(a, Sa);
                n = dot6(a, Ga);
                tau = dot6(ju, Gu) + dot6(jv, Gv);
                const double pq = g * c2 * ih2, pn = -(c2 * ih);
#pragma unroll
                for (int q = 0; q < 6; ++q) ab[q] = 2.0 * (pq * Sa[q] + pn * Ga[q]);
            }
            const double ph = c2 * n * ih2 - g * ih2 - 2.0 * g * c2 * qq * (ih2 * ih);
            const double pc = 2.0 * g * c * qq * ih2 + tau - 2.0 * c * n * ih + kk * ph;
            const double pk = c * ph;
            // the cotangents of the rows of J_cam and of jd
            double Ju[6], Jv[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                Ju[q] = jdu * ab[q] + 2.0 * c * Gu[q];
                Jv[q] = jdv * ab[q] + 2.0 * c * Gv[q];
            }
            const double bju = dot6(ju, ab) + 2.0 * pk * jdu, bjv = dot6(jv, ab) + 2.0 * pk * jdv;
            // through J = J_q [-I, [Q]x], jd = J_q d and c(s) to the cotangents of J_q = [[a, 0, bq], [0, cq, dq]], Q, d and r
            const V3<double> m = R * V3<double>{px.xh, px.yh, 1.0};      // dQ/d(1/rho); d = -m / rho^2
            const double zi = 1.0 / rho, k2 = -(zi * zi);
            const V3<double> d{m.x * k2, m.y * k2, m.z * k2};
            const V3<double> Q = p.p.Q;
            const double fa = p.p.a, fb = p.p.bq, fc = p.p.cq, fd = p.p.dq, iz = p.p.iz;
            const double ba = bju * d.x - Ju[0] - Ju[4] * Q.z + Ju[5] * Q.y;
            const double bb = bju * d.z - Ju[2] - Ju[3] * Q.y + Ju[4] * Q.x;
            const double bc = bjv * d.y - Jv[1] + Jv[3] * Q.z - Jv[5] * Q.x;
            const double bd = bjv * d.z - Jv[2] - Jv[3] * Q.y + Jv[4] * Q.x;
            const double bru = 2.0 * p.p.cp * pc * p.p.ru, brv = 2.0 * p.p.cp * pc * p.p.rv;
            const V3<double> bQ{Ju[4] * fb + Jv[4] * fd - Jv[5] * fc + fa * bru - fa * iz * bb,
                                Ju[5] * fa - Ju[3] * fb - Jv[3] * fd + fc * brv - fc * iz * bd,
                                Jv[3] * fc - Ju[4] * fa + fb * bru + fd * brv - iz * (fa * ba + 2.0 * fb * bb + fc * bc + 2.0 * fd * bd)};
            const V3<double> bd3{bju * fa, bjv * fc, bju * fb + bjv * fd};
            // Q = m / rho + t, d = -m / rho^2
            const V3<double> bm{zi * bQ.x + k2 * bd3.x, zi * bQ.y + k2 * bd3.y, zi * bQ.z + k2 * bd3.z};
            g_rho = k2 * dot(bQ, m) + 2.0 * (zi * zi * zi) * dot(bd3, m);
            g_fu = -bru;
            g_fv = -brv;
            acc[0] += bm.x * px.xh; acc[1] += bm.x * px.yh; acc[2] += bm.x;
            acc[3] += bm.y * px.xh; acc[4] += bm.y * px.yh; acc[5] += bm.y;
            acc[6] += bm.z * px.xh; acc[7] += bm.z * px.yh; acc[8] += bm.z;
            acc[9] += bQ.x; acc[10] += bQ.y; acc[11] += bQ.z;
        }
        grho[i] = g_rho;
        gfu[i] = (float)g_fu;
        gfv[i] = (float)g_fv;
    }
    reduce_and_store_row<12>(acc, partial + ((size_t)b * NBLK + blockIdx.x) * 12, true, 0.0);
}

// grid (B) x 64.  The NBLK rows of a link are summed in index order; lane 0 chains the cotangent of (R, t) = T^-1 back through qmat, the
// inverse and the mount conjugation of camera_inverse to the plain components [t, q xyzw] of motion[b] (no unit-norm assumption, the
// convention of section 3.31).  A link with a status gets seven zeros.
__global__ __launch_bounds__(64) void depth_var_pose_kernel(const double* __restrict__ partial, const double* __restrict__ motion,
                                                             const double* __restrict__ rgb2imu, const int* __restrict__ status,
                                                             double* __restrict__ grad_motion) {
    const int b = blockIdx.x, i = threadIdx.x;
    const bool live = status[b] == ISLAM_DENSE_REPROJ_OK;
    __shared__ double s[12];
    if (live && i < 12) {
        double v = 0.0;
        for (int k = 0; k < NBLK; ++k) v += partial[((size_t)b * NBLK + k) * 12 + i];
        s[i] = v;
    }
    __syncthreads();
    if (i != 0) return;
    double* gm = grad_motion + (size_t)b * 7;
    if (!live) {
        for (int k = 0; k < 7; ++k) gm[k] = 0.0;
        return;
    }
    camera_inverse_vjp(motion + 7 * b, rgb2imu, s, v3(s[9], s[10], s[11]), gm);
}

// the scratch of islam_dense_ba_depth_var_vjp: S_cam^-1 (B,21), the rows of G (B,NBLK,21), the rows of the pose sums (B,NBLK,12)
struct VarGradScratch {
    double *sinv, *gpart, *ppart;
    size_t bytes;
};

VarGradScratch var_grad_scratch(void* base, int B) {
    VarGradScratch vs{};
    auto carve = [&](double*& p, size_t count) {
        p = reinterpret_cast<double*>(reinterpret_cast<uintptr_t>(base) + vs.bytes);
        vs.bytes += align_up(count * sizeof(double));
    };
    carve(vs.sinv, (size_t)B * 21);
    carve(vs.gpart, (size_t)B * NBLK * 21);
    carve(vs.ppart, (size_t)B * NBLK * 12);
    return vs;
}

}  // namespace

extern "C" size_t islam_dense_ba_depth_var_vjp_scratch_bytes(int B) {
    if (B < 1) return 0;
    return var_grad_scratch(nullptr, B).bytes;
}

extern "C" int islam_dense_ba_depth_var_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                            const double* rgb2imu_or_null, const double* intr4, const double* prior_weight,
                                            const float* prior_scale_or_null, const double* inv_depth, const double* sums,
                                            const int* status_or_null, int robust_kind, double robust_delta, int mode, const double* grad_var,
                                            double* grad_inv_depth, float* grad_flow, double* grad_motion, int* out_status, void* scratch, int B,
                                            int H, int W, void* stream) {
    const char* who = "islam_dense_ba_depth_var_vjp";
    if (int rc = check_shape_kind(who, B, H, W, robust_kind, robust_delta)) return rc;
    if (mode != 0 && mode != 1) return fail(ISLAM_EARG, "%s: mode must be 0 (marginal) or 1 (conditional), got %d", who, mode);
    if (!depth || !flow || !motion || !intr4) return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 pointer", who);
    if (!prior_weight) return fail(ISLAM_EARG, "%s: NULL prior_weight", who);
    if (!inv_depth || !sums || !grad_var) return fail(ISLAM_EARG, "%s: NULL inv_depth / sums / grad_var pointer", who);
    if (!grad_inv_depth || !grad_flow || !grad_motion || !out_status || !scratch)
        return fail(ISLAM_EARG, "%s: NULL grad_inv_depth / grad_flow / grad_motion / out_status / scratch pointer", who);
    hipStream_t s = as_stream(stream);
    const VarGradScratch vs = var_grad_scratch(scratch, B);
    const int marginal = mode == 0;
    // the forward call's first launch on the same sums: the same S_cam^-1 and status, bit for bit, so nothing has to be saved
    hipLaunchKernelGGL(depth_var_factor_kernel, dim3(B), dim3(64), 0, s, sums, prior_weight, status_or_null, marginal, vs.sinv, out_status);
    if (marginal)
        hipLaunchKernelGGL(depth_var_adj_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu_or_null, intr4,
                           prior_weight, prior_scale_or_null, inv_depth, vs.sinv, out_status, grad_var, vs.gpart, H, W, robust_kind,
                           robust_delta);
    hipLaunchKernelGGL(depth_var_vjp_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu_or_null, intr4, prior_weight,
                       prior_scale_or_null, inv_depth, vs.sinv, vs.gpart, out_status, grad_var, grad_inv_depth, grad_flow, vs.ppart, H, W,
                       robust_kind, robust_delta, marginal);
    hipLaunchKernelGGL(depth_var_pose_kernel, dim3(B), dim3(64), 0, s, vs.ppart, motion, rgb2imu_or_null, out_status, grad_motion);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// ------------------------------------------------------------------ the gradient of the joint refinement with the exact Hessian
// (the formulas: include/islam_hip.h, islam_dense_ba_newton_weights.)  Section 3.26's adjoint system with
// the Gauss-Newton blocks c J_cam^T J_cam, h_pd, h_dd replaced by one half of the Hessian of the cost, in the same per-pixel
// elimination.  With J_q = dr/dQ, D_p = [-I, [Q]x], d = dQ/drho = -R ray / rho^2, M = c I + 2 c' r r^T, n = J_q^T c r and
// K = J_q^T M J_q - (n e_z^T + e_z n^T) / Q_z:
//   n_pp = D_p^T K D_p + C,   n_pd = D_p^T K d + [0; n x d],   n_dd = d^T K d - (2 / rho) n.d + w_i,
// C the second-order term of Exp: C_rho,phi = [n]x / 2, C_phi,phi = (n Q^T + Q n^T) / 2 - (n.Q) I.  A valid pixel whose n_dd is not
// > 0 takes its three Gauss-Newton blocks (K -> c J_q^T J_q, n -> 0) and is counted.  ba_newton_partial_kernel reduces the 21 sums of
// S_N,cam = sum n_pp - n_pd n_pd^T / n_dd, the 6 of u_cam = sum n_pd v_d / n_dd and the count (one row of 28 per workgroup, plain
// stores), ba_newton_solve_kernel makes S_N = A^T S_N,cam A and lambda_p, ba_newton_vjp_kernel streams section 3.26's data gradient out
// with lambda_d from the exact n_pd, n_dd.  MAP: the pixel's prior weight is w_b m_i (map_prior), as in section 3.27.
namespace {

constexpr int NN = 28, N_U = 21, N_FB = 27;      // the row of the reduction: 21 of S_N,cam, 6 of u_cam, the fallback count

// the pose-depth column and the depth-depth entry of one valid pixel, with what the pose-pose block is formed from: K (xx, xy, xz, yy,
// yz, zz), n, and K d
struct NewtonPixel {
    double K[6];
    V3<double> n, Kd, d;
    double npd[6], ndd;
    bool fallback;
};

// K and n from the 2x2 M = [[m00, m01], [m01, m11]] and y = c r; then d-dependent terms.  exact = false: the Gauss-Newton blocks
ISLAM_DEV void newton_terms(const Pixel& p, const V3<double>& d, double zi, double w, bool exact, NewtonPixel& o) {
    const double c = p.c, ru = p.ru, rv = p.rv;
    const double k2 = exact ? 2.0 * p.cp : 0.0;
    const double m00 = c + k2 * ru * ru, m01 = k2 * ru * rv, m11 = c + k2 * rv * rv;
    const double a = p.a, bq = p.bq, cq = p.cq, dq = p.dq;
    // n = J_q^T y
    const double yu = exact ? c * ru : 0.0, yv = exact ? c * rv : 0.0;
    o.n = {a * yu, cq * yv, bq * yu + dq * yv};
    // J_q^T M J_q with J_q = [[a, 0, bq], [0, cq, dq]], and B = -iz (n e_z^T + e_z n^T)
    const double tu = m00 * bq + m01 * dq, tv = m01 * bq + m11 * dq;      // M (bq, dq)
    o.K[0] = a * a * m00;
    o.K[1] = a * cq * m01;
    o.K[2] = a * tu - p.iz * o.n.x;
    o.K[3] = cq * cq * m11;
    o.K[4] = cq * tv - p.iz * o.n.y;
    o.K[5] = bq * tu + dq * tv - 2.0 * p.iz * o.n.z;
    o.Kd = {o.K[0] * d.x + o.K[1] * d.y + o.K[2] * d.z, o.K[1] * d.x + o.K[3] * d.y + o.K[4] * d.z, o.K[2] * d.x + o.K[4] * d.y + o.K[5] * d.z};
    o.ndd = dot(d, o.Kd) - 2.0 * zi * dot(o.n, d) + w;
}

// everything of one VALID pixel; p the front at 1 / rho, dR = R ray
ISLAM_DEV NewtonPixel newton_pixel(const Pixel& p, const V3<double>& dR, double rho, double w) {
    NewtonPixel o;
    const double zi = 1.0 / rho;
    const double k = -(zi * zi);
    o.d = {dR.x * k, dR.y * k, dR.z * k};
    newton_terms(p, o.d, zi, w, true, o);
    o.fallback = !(o.ndd > 0.0);
    if (o.fallback) newton_terms(p, o.d, zi, w, false, o);
    // n_pd = D_p^T K d + [0; n x d] = [-K d; K d x Q + n x d]
    const V3<double> f = cross(o.Kd, p.Q) + cross(o.n, o.d);
    o.npd[0] = -o.Kd.x; o.npd[1] = -o.Kd.y; o.npd[2] = -o.Kd.z;
    o.npd[3] = f.x; o.npd[4] = f.y; o.npd[5] = f.z;
    return o;
}

template <bool MAP>
__global__ __launch_bounds__(256) void ba_newton_partial_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                                 const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                                 const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                                 const double* __restrict__ prior_weight,
                                                                 const float* __restrict__ prior_scale, const double* __restrict__ inv_depth,
                                                                 const double* __restrict__ grad_rho, const int* __restrict__ status,
                                                                 double* __restrict__ partial, int H, int W, int kind, double delta) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const double wb = prior_weight[b];
    // a marked link (or one without a usable prior weight) stores rows of zeros without reading its pixels
    const bool live = wb > 0.0 && !(status && status[b] != ISLAM_DENSE_REPROJ_OK);
    double acc[NN] = {};
    if (live) {
        __shared__ double Tp[12];
        if (threadIdx.x == 0) pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
        __syncthreads();
        const M3<double> R = m3_load(Tp);
        const V3<double> t{Tp[9], Tp[10], Tp[11]};
        const size_t off = (size_t)b * HW;
        const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
        const float* ms = MAP ? prior_scale + off : nullptr;
        const double* rp = inv_depth + off;
        const double* vp = grad_rho ? grad_rho + off : nullptr;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
            const PixelIn px = pixel_in(lp, i);
            bool prior = isfinite(px.z) && px.z > 0.0;
            double w = wb;
            if constexpr (MAP) prior = map_prior(ms, i, wb, prior, w);
            const double rho = rp[i];
            if (!(prior && isfinite(rho) && rho > 0.0)) continue;
            const Pixel p = reproj_pixel(R, t, 1.0 / rho, px, lp);
            if (!p.valid) continue;
            const NewtonPixel o = newton_pixel(p, R * V3<double>{px.xh, px.yh, 1.0}, rho, w);
            const double ih = 1.0 / o.ndd;
            // the columns of D_p = [-I, [Q]x]: -e_x, -e_y, -e_z, Q x e_x, Q x e_y, Q x e_z, and K times each
            const V3<double> Q = p.Q;
            const V3<double> col[6] = {{-1.0, 0.0, 0.0}, {0.0, -1.0, 0.0}, {0.0, 0.0, -1.0}, {0.0, Q.z, -Q.y}, {-Q.z, 0.0, Q.x}, {Q.y, -Q.x, 0.0}};
            const double* K = o.K;
            V3<double> Kc[6];
#pragma unroll
            for (int l = 0; l < 6; ++l)
                Kc[l] = {K[0] * col[l].x + K[1] * col[l].y + K[2] * col[l].z, K[1] * col[l].x + K[3] * col[l].y + K[4] * col[l].z,
                         K[2] * col[l].x + K[4] * col[l].y + K[5] * col[l].z};
            // C: the second-order term of Exp.  rho-phi block [n]x / 2, phi-phi block (n Q^T + Q n^T) / 2 - (n.Q) I
            const V3<double> n = o.n;
            const double nq = dot(n, Q);
            const double hx = 0.5 * n.x, hy = 0.5 * n.y, hz = 0.5 * n.z;
            double C[21] = {};
            C[tri(0, 4)] = -hz; C[tri(0, 5)] = hy; C[tri(1, 3)] = hz; C[tri(1, 5)] = -hx; C[tri(2, 3)] = -hy; C[tri(2, 4)] = hx;
            C[tri(3, 3)] = n.x * Q.x - nq; C[tri(4, 4)] = n.y * Q.y - nq; C[tri(5, 5)] = n.z * Q.z - nq;
            C[tri(3, 4)] = hx * Q.y + hy * Q.x; C[tri(3, 5)] = hx * Q.z + hz * Q.x; C[tri(4, 5)] = hy * Q.z + hz * Q.y;
            int k = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const double fq = o.npd[q] * ih;
#pragma unroll
                for (int l = q; l < 6; ++l, ++k) acc[k] += (dot(col[q], Kc[l]) + C[k]) - fq * o.npd[l];
            }
            if (vp) {
                const double kv = vp[i] * ih;      // v_d / n_dd
#pragma unroll
                for (int l = 0; l < 6; ++l) acc[N_U + l] += o.npd[l] * kv;
            }
            acc[N_FB] += o.fallback ? 1.0 : 0.0;
        }
    }
    reduce_and_store_row<NN>(acc, partial + ((size_t)b * NBLK + blockIdx.x) * NN, live, 0.0);
}

// S_N and lambda_p per link, one 64-lane workgroup: the NBLK rows in fixed order, S_N = A^T S_N,cam A as the final kernel forms its H
// ((r, c) and (c, r) run the same operations: symmetric to the bit), v_p from the gradient on [t, q xyzw] (tangent_gradient), A^T u_cam
// by adjoint_apply<true>.  A link that comes with a status, whose prior weight is not > 0 (BADPRIOR), or whose S_N is not finite or
// has a non-positive pivot (NOTPD) gets lambda_p = 0 (adjoint_solve_tail).
__global__ __launch_bounds__(64) void ba_newton_solve_kernel(const double* __restrict__ partial, const double* __restrict__ motion,
                                                              const double* __restrict__ grad_motion, const double* __restrict__ rgb2imu,
                                                              const double* __restrict__ prior_weight, const int* __restrict__ status_in,
                                                              double* __restrict__ lambda_p, double* __restrict__ S_out,
                                                              int* __restrict__ fallback_count, int* __restrict__ status_out) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ double s[NN], Rm[9], Sm[9], A[36], Hn[36], vn[6], L[6][6], x[6];
    __shared__ int bad;
    if (i < NN) {
        double v = 0.0;
        for (int k = 0; k < NBLK; ++k) v += partial[((size_t)b * NBLK + k) * NN + i];
        s[i] = v;
    }
    if (i == 0) {      // C^-1 = (R, t)
        bad = 0;
        M3<double> Rc = m3_identity<double>(), Sc{0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (rgb2imu) {
            const SE3<double> Ci = se3_inv(se3_load(rgb2imu));
            Rc = qmat(Ci.q);
            Sc = skew(Ci.t) * Rc;
        }
        m3_store(Rc, Rm);
        m3_store(Sc, Sm);
    }
    __syncthreads();
    if (i < 36) {      // A = Ad(C^-1) = [[R, [t]x R], [0, R]]
        const int r = i / 6, c = i - 6 * r;
        A[i] = r < 3 ? (c < 3 ? Rm[3 * r + c] : Sm[3 * r + c - 3]) : (c < 3 ? 0.0 : Rm[3 * (r - 3) + c - 3]);
    }
    __syncthreads();
    if (i < 36) {
        const int r0 = i / 6, c0 = i - 6 * r0;
        const int r = min(r0, c0), c = max(r0, c0);
        double v = 0.0;
        for (int k = 0; k < 6; ++k) {
            double w = 0.0;
            for (int l = 0; l < 6; ++l) w += s[tri(min(k, l), max(k, l))] * A[l * 6 + c];
            v += A[k * 6 + r] * w;
        }
        Hn[i] = v;
        if (!isfinite(v)) bad = 1;
        if (S_out) S_out[(size_t)b * 36 + i] = v;
    }
    if (i == 0) {
        fallback_count[b] = (int)s[N_FB];
        V3<double> vr, vf;
        tangent_gradient(motion + (size_t)b * 7, grad_motion + (size_t)b * 7, vr, vf);
        V3<double> ur{s[N_U], s[N_U + 1], s[N_U + 2]}, uf{s[N_U + 3], s[N_U + 4], s[N_U + 5]};
        adjoint_apply<true>(rgb2imu, ur, uf);      // A^T u_cam
        vr = vr - ur;
        vf = vf - uf;
        vn[0] = vr.x; vn[1] = vr.y; vn[2] = vr.z; vn[3] = vf.x; vn[4] = vf.y; vn[5] = vf.z;
    }
    __syncthreads();
    int st = status_in ? status_in[b] : ISLAM_DENSE_REPROJ_OK;
    if (st == ISLAM_DENSE_REPROJ_OK && !(prior_weight[b] > 0.0)) st = ISLAM_DENSE_REPROJ_BADPRIOR;
    if (st == ISLAM_DENSE_REPROJ_OK && bad) st = ISLAM_DENSE_REPROJ_NOTPD;
    adjoint_solve_tail(st, Hn, vn, L, x, status_out + b, lambda_p + (size_t)b * 6);
}

template <bool MAP>
__global__ __launch_bounds__(256) void ba_newton_vjp_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                             const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                             const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                             const double* __restrict__ prior_weight, const float* __restrict__ prior_scale,
                                                             const double* __restrict__ inv_depth, const double* __restrict__ lambda_p,
                                                             const double* __restrict__ grad_rho, const int* __restrict__ status,
                                                             float* __restrict__ grad_depth, float* __restrict__ grad_flow, int H, int W,
                                                             int kind, double delta) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const size_t off = (size_t)b * HW;
    const LinkGrads out = link_grads(grad_depth, grad_flow, b, HW);
    const double wb = prior_weight[b];
    if (!(wb > 0.0) || (status && status[b] != ISLAM_DENSE_REPROJ_OK)) return grad_zero_link(out, HW);      // a link without a gradient
    __shared__ double Tp[12], lcam[6];
    if (threadIdx.x == 0) {
        pose_to_lds(camera_inverse(pose7 + 7 * b, rgb2imu), Tp);
        adjoint_to_camera(rgb2imu, lambda_p + 6 * b, lcam);      // lambda_cam = Ad(C^-1) lambda_p
    }
    __syncthreads();
    const M3<double> R = m3_load(Tp);
    const V3<double> t{Tp[9], Tp[10], Tp[11]};
    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    const float* ms = MAP ? prior_scale + off : nullptr;
    const double* rp = inv_depth + off;
    const double* vp = grad_rho ? grad_rho + off : nullptr;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const PixelIn px = pixel_in(lp, i);
        const double z = px.z;
        bool prior = isfinite(z) && z > 0.0;
        double w = wb;
        if constexpr (MAP) prior = map_prior(ms, i, wb, prior, w);
        double gz = 0.0, gu = 0.0, gv = 0.0;
        if (prior) {
            const double rho = rp[i];
            const double vdi = vp ? vp[i] : 0.0;
            double ld = -vdi / w;          // an invalid pixel follows its prior
            if (isfinite(rho) && rho > 0.0) {
                const Pixel p = reproj_pixel(R, t, 1.0 / rho, px, lp);
                if (p.valid) {
                    const NewtonPixel o = newton_pixel(p, R * V3<double>{px.xh, px.yh, 1.0}, rho, w);
                    const double c = p.c, ru = p.ru, rv = p.rv;
                    double du = 0.0, dv = 0.0, nl = 0.0;      // J_cam lambda_cam, n_pd . lambda_cam
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        du += p.ju[q] * lcam[q];
                        dv += p.jv[q] * lcam[q];
                        nl += o.npd[q] * lcam[q];
                    }
                    ld = -(vdi + nl) / o.ndd;
                    // jd = J_q d
                    const double jdu = p.a * o.d.x + p.bq * o.d.z, jdv = p.cq * o.d.y + p.dq * o.d.z;
                    const double qu = du + jdu * ld, qv = dv + jdv * ld;
                    const double k2 = 2.0 * p.cp * (qu * ru + qv * rv);
                    gu = -(c * qu + k2 * ru);
                    gv = -(c * qv + k2 * rv);
                }
            }
            gz = w * ld / (z * z);
        }
        grad_store(out, i, gz, gu, gv);
    }
}

}  // namespace

extern "C" size_t islam_dense_ba_newton_scratch_bytes(int B) {
    if (B < 1) return 0;
    return align_up((size_t)B * NBLK * NN * sizeof(double));
}

extern "C" int islam_dense_ba_newton_weights(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                             const double* rgb2imu, const double* intr4, const double* prior_weight,
                                             const float* prior_scale_or_null, const double* inv_depth, int robust_kind, double robust_delta,
                                             const double* grad_motion, const double* grad_inv_depth_or_null, const int* status_in_or_null,
                                             void* scratch, int B, int H, int W, double* lambda_p, double* S_newton_or_null,
                                             int* fallback_count, int* status_out, void* stream) {
    const char* who = "islam_dense_ba_newton_weights";
    if (int rc = check_joint_adjoint(who, depth, flow, motion, intr4, prior_weight, inv_depth, lambda_p, robust_kind, robust_delta, B, H, W))
        return rc;
    if (!grad_motion || !fallback_count || !status_out || !scratch)
        return fail(ISLAM_EARG, "%s: NULL grad_motion / fallback_count / status_out / scratch pointer", who);
    hipStream_t s = as_stream(stream);
    double* partial = static_cast<double*>(scratch);
    if (prior_scale_or_null)
        hipLaunchKernelGGL(ba_newton_partial_kernel<true>, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu, intr4,
                           prior_weight, prior_scale_or_null, inv_depth, grad_inv_depth_or_null, status_in_or_null, partial, H, W, robust_kind,
                           robust_delta);
    else
        hipLaunchKernelGGL(ba_newton_partial_kernel<false>, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu, intr4,
                           prior_weight, nullptr, inv_depth, grad_inv_depth_or_null, status_in_or_null, partial, H, W, robust_kind, robust_delta);
    hipLaunchKernelGGL(ba_newton_solve_kernel, dim3(B), dim3(64), 0, s, partial, motion, grad_motion, rgb2imu, prior_weight, status_in_or_null,
                       lambda_p, S_newton_or_null, fallback_count, status_out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" int islam_dense_ba_newton_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                         const double* rgb2imu, const double* intr4, const double* prior_weight,
                                         const float* prior_scale_or_null, const double* inv_depth, int robust_kind, double robust_delta,
                                         const double* lambda_p, const double* grad_inv_depth_or_null, const int* status_or_null,
                                         float* grad_depth, float* grad_flow, int B, int H, int W, void* stream) {
    const char* who = "islam_dense_ba_newton_vjp";
    if (int rc = check_joint_adjoint(who, depth, flow, motion, intr4, prior_weight, inv_depth, lambda_p, robust_kind, robust_delta, B, H, W))
        return rc;
    if (!grad_depth || !grad_flow) return fail(ISLAM_EARG, "%s: NULL grad_depth / grad_flow pointer", who);
    if (prior_scale_or_null)
        hipLaunchKernelGGL(ba_newton_vjp_kernel<true>, dim3(NBLK, B), dim3(256), 0, as_stream(stream), depth, flow, mask, motion, rgb2imu, intr4,
                           prior_weight, prior_scale_or_null, inv_depth, lambda_p, grad_inv_depth_or_null, status_or_null, grad_depth, grad_flow,
                           H, W, robust_kind, robust_delta);
    else
        hipLaunchKernelGGL(ba_newton_vjp_kernel<false>, dim3(NBLK, B), dim3(256), 0, as_stream(stream), depth, flow, mask, motion, rgb2imu, intr4,
                           prior_weight, nullptr, inv_depth, lambda_p, grad_inv_depth_or_null, status_or_null, grad_depth, grad_flow, H, W,
                           robust_kind, robust_delta);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}
