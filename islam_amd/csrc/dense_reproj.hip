// Dense reprojection residual on gfx950: Gauss-Newton normal equations per link from one pass over the image, and a device-side
// Levenberg-Marquardt on them (definitions: include/islam_hip.h, "dense reprojection").
//
// Per pixel (u, v) of link b, all in fp64:  P = z ((u-cx)/fx, (v-cy)/fy, 1),  Q = T^-1 P with T = C^-1 motion C,
//   valid = mask & Q_z > 0.1 & |Q_x/Q_z| <= 1 & |Q_y/Q_z| <= 1,   r = (fx Q_x/Q_z + cx - (flow_u + u), fy Q_y/Q_z + cy - (flow_v + v)),
//   J_cam = dr/dQ [-I, [Q]x]  (right perturbation T Exp(xi_cam)),  s = |r|^2,  c = rho'(s).
// The partial kernel accumulates, in the CAMERA frame, sums[0..20] = the upper triangle of sum c J^T J in row-major order of the
// triangle, sums[21..26] = sum c J^T r, sums[27] = sum rho(s), sums[28] = sum |r_u| + |r_v|, sums[29] = number of valid pixels.
// HBM-bound: 13 bytes per pixel (depth, two flow floats, one mask byte) for ~150 flops.  The final kernel sums the NBLK rows of a
// link in fixed order and applies A = Ad(C^-1) once: H = A^T H_cam A, g = A^T g_cam.  No atomics anywhere: a second call gives
// the same bits.  Under refinement the final kernel's lane 0 also runs the LM bookkeeping of its link (accept test, damping,
// 6x6 Cholesky in LDS, next trial pose), so an evaluation is two launches and the host never waits between them.
// The head of the pixel loop (pixel_in), everything of a pixel ahead of the accumulators (reproj_pixel), the reduction epilogue, the
// final kernel's body, the Cholesky step, the pose decode, the stores of the VJP kernel, the head and tail of the solve kernel and
// the host-side argument checks are shared with dense_ba.hip through dense_reproj_dev.h.
// Further down: the gradient of the refined pose in depth and flow (reproj_vjp_kernel, reproj_ift_kernel).
#include <hip/hip_runtime.h>

#include "common.h"
#include "dense_reproj_dev.h"
#include "lie_dev.h"

using namespace islam;

namespace {

__global__ __launch_bounds__(256) void dense_reproj_partial_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                                    const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                                    const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                                    double* __restrict__ partial, int H, int W, int kind, double delta) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const SE3<double> Ti = camera_inverse(pose7 + 7 * b, rgb2imu);
    const M3<double> R = qmat(Ti.q);
    const V3<double> t = Ti.t;

    double acc[NS] = {};
    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const PixelIn pin = pixel_in(lp, i);
        const Pixel px = reproj_pixel(R, t, pin.z, pin, lp);
        if (!px.valid) continue;
        const double *ju = px.ju, *jv = px.jv;
        int k = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const double wu = px.c * ju[p], wv = px.c * jv[p];
#pragma unroll
            for (int q = p; q < 6; ++q) acc[k++] += wu * ju[q] + wv * jv[q];
            acc[S_G + p] += wu * px.ru + wv * px.rv;
        }
        acc[S_COST] += px.rob;
        acc[S_L1] += fabs(px.ru) + fabs(px.rv);
        acc[S_COUNT] += 1.0;
    }
    reduce_and_store_row<NS>(acc, partial + ((size_t)b * NBLK + blockIdx.x) * NS, true, NAN);
}

__global__ __launch_bounds__(64) void dense_reproj_final_kernel(const double* __restrict__ partial, const double* __restrict__ rgb2imu,
                                                                 const double* __restrict__ pose_eval, Outputs out, Refine rf, int B) {
    final_body<false>(partial, rgb2imu, pose_eval, out, rf, Joint{}, B);
}

// ------------------------------------------------------------------ the gradient of the refined pose in depth and flow
//   Phi = w^T g = sum_valid c(s) q.r with q = dr/dQ m, m = [-I, [Q]x] A w, at a fixed pose and a fixed
// valid set.  reproj_vjp_kernel writes dPhi/dz and dPhi/dflow of every pixel: the partial kernel's pass without its reduction, 13
// bytes read and 12 written per pixel, no LDS, no atomics.  reproj_ift_kernel makes the w for which that is the gradient of a loss
// on the refined pose: w = -H^-1 v, v the loss's gradient in the right tangent of the pose.
// (The two names leave "dense_reproj" to the two kernels above: tests/test_dense_reproj_cpu.py pins the family's kernel names.)
__global__ __launch_bounds__(256) void reproj_vjp_kernel(const float* __restrict__ depth, const float* __restrict__ flow,
                                                          const uint8_t* __restrict__ mask, const double* __restrict__ pose7,
                                                          const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                          const double* __restrict__ w6, const int* __restrict__ status,
                                                          float* __restrict__ grad_depth, float* __restrict__ grad_flow, int H, int W,
                                                          int kind, double delta) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const LinkGrads out = link_grads(grad_depth, grad_flow, b, HW);
    if (status && status[b] != ISLAM_DENSE_REPROJ_OK) return grad_zero_link(out, HW);      // a link without a gradient
    const SE3<double> Ti = camera_inverse(pose7 + 7 * b, rgb2imu);
    const M3<double> R = qmat(Ti.q);
    const V3<double> t = Ti.t;
    V3<double> wr{w6[6 * b], w6[6 * b + 1], w6[6 * b + 2]}, wf{w6[6 * b + 3], w6[6 * b + 4], w6[6 * b + 5]};
    adjoint_apply(rgb2imu, wr, wf);      // w_cam = Ad(C^-1) w

    const LinkPixels lp = link_pixels(depth, flow, mask, intr4, b, HW, W, kind, delta);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const PixelIn pin = pixel_in(lp, i);
        const Pixel p = reproj_pixel(R, t, pin.z, pin, lp);
        double gz = 0.0, gu = 0.0, gv = 0.0;
        if (p.valid) {
            const V3<double>& Q = p.Q;
            const double ru = p.ru, rv = p.rv, c = p.c, cp = p.cp, a = p.a, bq = p.bq, cq = p.cq, dq = p.dq, iz = p.iz;
            const V3<double> mm = cross(Q, wf) - wr;                            // [-I, [Q]x] w_cam
            const double qu = a * mm.x + bq * mm.z, qv = cq * mm.y + dq * mm.z;  // q = dr/dQ m
            const double k2 = 2.0 * cp * (qu * ru + qv * rv);
            const double eu = c * qu + k2 * ru, ev = c * qv + k2 * rv;           // e = d(c q.r)/dr
            const V3<double> dQ = R * V3<double>{pin.xh, pin.yh, 1.0};           // dQ/dz
            const double da = -a * iz * dQ.z, dbq = -a * iz * dQ.x - 2.0 * bq * iz * dQ.z;      // d(dr/dQ) along dQ
            const double dcq = -cq * iz * dQ.z, ddq = -cq * iz * dQ.y - 2.0 * dq * iz * dQ.z;
            const V3<double> n = cross(dQ, wf);                                 // dm along dQ
            const double tu = da * mm.x + dbq * mm.z + a * n.x + bq * n.z, tv = dcq * mm.y + ddq * mm.z + cq * n.y + dq * n.z;
            gz = eu * (a * dQ.x + bq * dQ.z) + ev * (cq * dQ.y + dq * dQ.z) + c * (ru * tu + rv * tv);
            gu = -eu;
            gv = -ev;
        }
        grad_store(out, i, gz, gu, gv);
    }
}

// w = -H^-1 v per link, v = dL/dxi on motion Exp(xi) from the gradient on [t, q xyzw] (tangent_gradient).  A link that comes with a
// status, or whose H has a non-positive pivot, gets w = 0.
__global__ __launch_bounds__(64) void reproj_ift_kernel(const double* __restrict__ Hm, const double* __restrict__ motion,
                                                         const double* __restrict__ grad_motion, const int* __restrict__ status_in,
                                                         double* __restrict__ w, int* __restrict__ status_out) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ double Hn[36], vn[6], L[6][6], x[6];
    if (i < 36) Hn[i] = Hm[(size_t)b * 36 + i];
    if (i == 0) {
        V3<double> vr, vf;
        tangent_gradient(motion + (size_t)b * 7, grad_motion + (size_t)b * 7, vr, vf);
        vn[0] = vr.x; vn[1] = vr.y; vn[2] = vr.z; vn[3] = vf.x; vn[4] = vf.y; vn[5] = vf.z;
    }
    __syncthreads();
    adjoint_solve_tail(status_in ? status_in[b] : ISLAM_DENSE_REPROJ_OK, Hn, vn, L, x, status_out + b, w + (size_t)b * 6);
}

}  // namespace

extern "C" size_t islam_dense_reproj_scratch_bytes(int B, int iters_or_0) {
    if (B < 1) return 0;
    size_t n = partial_bytes(B);
    if (iters_or_0 > 0) n += align_up((size_t)B * 7 * sizeof(double));
    return n;
}

extern "C" int islam_dense_reproj_normal(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                         const double* rgb2imu, const double* intr4, int robust_kind, double robust_delta,
                                         double* out_H, double* out_g, double* out_cost, double* out_l1, double* out_count,
                                         double* out_sums, void* scratch, int B, int H, int W, void* stream) {
    const Outputs o{out_H, out_g, out_cost, out_l1, out_count, out_sums};
    if (int rc = check_common("islam_dense_reproj_normal", depth, flow, motion, intr4, robust_kind, robust_delta, o, scratch, B, H, W))
        return rc;
    hipStream_t s = as_stream(stream);
    double* partial = static_cast<double*>(scratch);
    hipLaunchKernelGGL(dense_reproj_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, motion, rgb2imu, intr4, partial,
                       H, W, robust_kind, robust_delta);
    hipLaunchKernelGGL(dense_reproj_final_kernel, dim3(B), dim3(64), 0, s, partial, rgb2imu, motion, o, Refine{}, B);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" int islam_dense_reproj_refine(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                         const double* rgb2imu, const double* intr4, int robust_kind, double robust_delta, int iters,
                                         double damping, double min_count, double* out_motion, double* out_H, double* out_g,
                                         double* out_cost, double* out_l1, double* out_count, double* out_sums, double* out_lambda,
                                         int* out_accepted, int* out_rejected, int* out_status, double* trace, int trace_cap,
                                         void* scratch, int B, int H, int W, void* stream) {
    const char* who = "islam_dense_reproj_refine";
    const Outputs o{out_H, out_g, out_cost, out_l1, out_count, out_sums};
    if (int rc = check_common(who, depth, flow, motion, intr4, robust_kind, robust_delta, o, scratch, B, H, W)) return rc;
    double* partial = static_cast<double*>(scratch);
    double* trial = reinterpret_cast<double*>(static_cast<char*>(scratch) + partial_bytes(B));
    Refine rf{out_motion, trial, out_lambda, out_accepted, out_rejected, out_status, trace_cap > 0 ? trace : nullptr, trace_cap, 0, 0,
              min_count, damping};
    if (int rc = check_refine(who, iters, rf, trace)) return rc;
    hipStream_t s = as_stream(stream);
    for (int k = 0; k < iters; ++k) {
        const double* pose = k == 0 ? motion : trial;
        rf.eval = k;
        rf.last = k == iters - 1;
        hipLaunchKernelGGL(dense_reproj_partial_kernel, dim3(NBLK, B), dim3(256), 0, s, depth, flow, mask, pose, rgb2imu, intr4, partial,
                           H, W, robust_kind, robust_delta);
        hipLaunchKernelGGL(dense_reproj_final_kernel, dim3(B), dim3(64), 0, s, partial, rgb2imu, pose, o, rf, B);
    }
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" int islam_dense_reproj_vjp(const float* depth, const float* flow, const uint8_t* mask, const double* motion,
                                      const double* rgb2imu, const double* intr4, int B, int H, int W, int robust_kind,
                                      double robust_delta, const double* w, const int* status_or_null, float* grad_depth,
                                      float* grad_flow, void* stream) {
    const char* who = "islam_dense_reproj_vjp";
    if (int rc = check_shape_kind(who, B, H, W, robust_kind, robust_delta)) return rc;
    if (!depth || !flow || !motion || !intr4 || !w || !grad_depth || !grad_flow)
        return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 / w / grad_depth / grad_flow pointer", who);
    hipLaunchKernelGGL(reproj_vjp_kernel, dim3(NBLK, B), dim3(256), 0, as_stream(stream), depth, flow, mask, motion, rgb2imu, intr4, w,
                       status_or_null, grad_depth, grad_flow, H, W, robust_kind, robust_delta);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" int islam_dense_reproj_ift_weights(const double* H, const double* motion, const double* grad_motion,
                                              const int* status_in_or_null, int B, double* w, int* status_out, void* stream) {
    const char* who = "islam_dense_reproj_ift_weights";
    if (B < 1) return fail(ISLAM_EARG, "%s: bad shape (%d)", who, B);
    if (!H || !motion || !grad_motion || !w || !status_out)
        return fail(ISLAM_EARG, "%s: NULL H / motion / grad_motion / w / status_out pointer", who);
    hipLaunchKernelGGL(reproj_ift_kernel, dim3(B), dim3(64), 0, as_stream(stream), H, motion, grad_motion, status_in_or_null, w, status_out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}
