// Joint two-view dense bundle adjustment on gfx950: the pose of a link and one inverse depth per pixel, the stereo depth as a
// Gaussian prior, the depths eliminated pixel by pixel (definitions: include/islam_hip.h, "dense reprojection"; DESIGN.md section
// 3.25).  It stands beside dense_reproj.hip and shares its final-kernel body, Cholesky step and sum layout (dense_reproj_dev.h).
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

// everything of one pixel at (T^-1 = (R, t), rho) that the sums and the back-substitution need
struct Pixel {
    bool valid;
    double ru, rv, c, rob, ju[6], jv[6], jdu, jdv;
};

ISLAM_DEV Pixel ba_pixel(const M3<double>& R, const V3<double>& t, double rho, double xh, double yh, double tu, double tv, bool m,
                         double fx, double fy, double cx, double cy, int kind, double delta, double d2) {
    Pixel p;
    const double zi = 1.0 / rho;
    const V3<double> P{zi * xh, zi * yh, zi};
    const V3<double> Q = R * P + t;
    p.valid = m && Q.z > 0.1;
    const double px = Q.x / Q.z, py = Q.y / Q.z;
    p.valid = p.valid && fabs(px) <= 1.0 && fabs(py) <= 1.0;
    p.ru = fx * px + cx - tu;
    p.rv = fy * py + cy - tv;
    const double s = p.ru * p.ru + p.rv * p.rv;
    p.rob = s;
    p.c = 1.0;
    if (kind == ISLAM_ROBUST_HUBER) {
        if (s > d2) {
            const double rs = sqrt(s);
            p.rob = 2.0 * delta * rs - d2;
            p.c = delta / rs;
        }
    } else if (kind == ISLAM_ROBUST_CAUCHY) {
        p.rob = d2 * log1p(s / d2);
        p.c = 1.0 / (1.0 + s / d2);
    }
    // dr/dQ = [[a, 0, bq], [0, cq, dq]];  rows of dr/dQ [-I, [Q]x]
    const double iz = 1.0 / Q.z;
    const double a = fx * iz, bq = -(a * px), cq = fy * iz, dq = -(cq * py);
    p.ju[0] = -a; p.ju[1] = 0.0; p.ju[2] = -bq; p.ju[3] = -bq * Q.y; p.ju[4] = bq * Q.x - a * Q.z; p.ju[5] = a * Q.y;
    p.jv[0] = 0.0; p.jv[1] = -cq; p.jv[2] = -dq; p.jv[3] = cq * Q.z - dq * Q.y; p.jv[4] = dq * Q.x; p.jv[5] = -cq * Q.x;
    const V3<double> dR = R * V3<double>{xh, yh, 1.0};      // dQ/d(1/rho)
    const double k = -(zi * zi);
    p.jdu = (a * dR.x + bq * dR.z) * k;
    p.jdv = (cq * dR.y + dq * dR.z) * k;
    return p;
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
    const double fx = intr4[4 * b], fy = intr4[4 * b + 1], cx = intr4[4 * b + 2], cy = intr4[4 * b + 3];
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
            // delta_cam = Ad(C^-1) delta = [R_c d_rho + t_c x (R_c d_phi), R_c d_phi]
            const double* dl = rs.delta + 6 * b;
            V3<double> dr{dl[0], dl[1], dl[2]}, df{dl[3], dl[4], dl[5]};
            if (rgb2imu) {
                const SE3<double> Ci = se3_inv(se3_load(rgb2imu));
                const M3<double> Rc = qmat(Ci.q);
                df = Rc * df;
                dr = Rc * dr + cross(Ci.t, df);
            }
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
                const Pixel p = ba_pixel(R, t, rho, (ud - cx) / fx, (vd - cy) / fy, (double)fup[i] + ud, (double)fvp[i] + vd,
                                         mp ? mp[i] != 0 : true, fx, fy, cx, cy, kind, delta, d2);
                if (p.valid) {
                    const double eu = p.c * p.jdu, ev = p.c * p.jdv;
                    const double hdd = eu * p.jdu + ev * p.jdv + w;
                    const double gd = eu * p.ru + ev * p.rv + w * (rho - rho0);
                    double du = 0.0, dv = 0.0;      // J_cam delta_cam
#pragma unroll
                    for (int q = 0; q < 6; ++q) {
                        du += p.ju[q] * dcam[q];
                        dv += p.jv[q] * dcam[q];
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
        const Pixel p = ba_pixel(R, t, rho, (ud - cx) / fx, (vd - cy) / fy, (double)fup[i] + ud, (double)fvp[i] + vd,
                                 mp ? mp[i] != 0 : true, fx, fy, cx, cy, kind, delta, d2);
        if (!p.valid) continue;
        // with e = c jd:  h_pd = J_cam^T e,  h_dd = e.jd + w,  g_d = e.r + w (rho - rho0).  The pixel's Schur term takes the shape of
        // section 3.23's: c J^T J - h_pd h_pd^T / h_dd = J^T M J with the 2x2 M = c I - e e^T / h_dd, and
        // c J^T r - h_pd g_d / h_dd = J^T (c r - e g_d / h_dd)
        const double eu = p.c * p.jdu, ev = p.c * p.jdv;
        const double dprior = rho - rho0;
        const double hdd = eu * p.jdu + ev * p.jdv + w;
        const double gd = eu * p.ru + ev * p.rv + w * dprior;
        const double ih = 1.0 / hdd;
        const double fu = eu * ih, fv = ev * ih;
        const double m00 = p.c - fu * eu, m01 = -(fu * ev), m11 = p.c - fv * ev;
        const double su = p.c * p.ru - fu * gd, sv = p.c * p.rv - fv * gd;
        int k = 0;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double wu = m00 * p.ju[q] + m01 * p.jv[q], wv = m01 * p.ju[q] + m11 * p.jv[q];
#pragma unroll
            for (int l = q; l < 6; ++l) acc[k++] += wu * p.ju[l] + wv * p.jv[l];
            acc[S_G + q] += p.ju[q] * su + p.jv[q] * sv;
        }
        acc[S_COST] += p.rob + w * dprior * dprior;
        acc[S_L1] += fabs(p.ru) + fabs(p.rv);
        acc[S_COUNT] += 1.0;
    }
    __shared__ double red[4][NS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double x = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) red[wv][i] = x;
    }
    __syncthreads();
    if (threadIdx.x < NS)      // a link without a usable prior weight has no sums: NaN, which the final kernel reports
        partial[((size_t)b * NBLK + blockIdx.x) * NS + threadIdx.x] =
            wok ? red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] : NAN;
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

int check_common(const char* who, const float* depth, const float* flow, const double* motion, const double* intr4, const double* prior_weight,
                 int kind, double delta, const Outputs& o, const void* scratch, int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 30)) return fail(ISLAM_EARG, "%s: bad shape (%d,%d,%d)", who, B, H, W);
    if (kind != ISLAM_ROBUST_NONE && kind != ISLAM_ROBUST_HUBER && kind != ISLAM_ROBUST_CAUCHY)
        return fail(ISLAM_EARG, "%s: unknown robust kind %d", who, kind);
    if (!(delta > 0.0)) return fail(ISLAM_EARG, "%s: robust delta must be positive (got %g)", who, delta);
    if (!depth || !flow || !motion || !intr4 || !o.H || !o.g || !o.cost || !o.l1 || !o.count || !o.sums || !scratch)
        return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 / output / scratch pointer", who);
    if (!prior_weight) return fail(ISLAM_EARG, "%s: NULL prior_weight", who);
    return ISLAM_OK;
}

size_t partial_bytes(int B) { return align_up((size_t)B * NBLK * NS * sizeof(double)); }

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
    if (int rc = check_common("islam_dense_ba_normal", depth, flow, motion, intr4, prior_weight, robust_kind, robust_delta, o, scratch, B, H, W))
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
    if (int rc = check_common(who, depth, flow, motion, intr4, prior_weight, robust_kind, robust_delta, o, scratch, B, H, W)) return rc;
    if (iters < 1) return fail(ISLAM_EARG, "%s: iters must be at least 1 (got %d)", who, iters);
    if (!(damping >= 0.0) || !(min_count >= 0.0)) return fail(ISLAM_EARG, "%s: damping and min_count must be non-negative", who);
    if (!out_motion || !out_lambda || !out_accepted || !out_rejected || !out_status)
        return fail(ISLAM_EARG, "%s: NULL out_motion / out_lambda / out_accepted / out_rejected / out_status", who);
    if (!out_inv_depth) return fail(ISLAM_EARG, "%s: NULL out_inv_depth", who);
    if (trace_cap < 0 || (trace_cap > 0 && !trace)) return fail(ISLAM_EARG, "%s: trace_cap %d without a trace buffer", who, trace_cap);
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
    Refine rf{out_motion, trial, out_lambda, out_accepted, out_rejected, out_status, trace_cap > 0 ? trace : nullptr, trace_cap, 0, 0,
              min_count, damping};
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
