// Depth propagation on gfx950: the inverse depths one joint refinement returned for frame k, and their variances, carried into the pixel
// grid of frame k+1 and fused there with that frame's own stereo measurement (definitions: include/islam_hip.h, "depth propagation";
// DESIGN.md section 3.28).  It stands beside dense_ba.hip and takes the camera-frame pose of a link (camera_inverse), the intrinsics
// (Intr) and the shape check from dense_reproj_dev.h.
//
// Per source pixel i of link b at (rho, s), all in fp64, with (R, t) = T^-1:
//   a = R[2,:].ray,  Q = R ray / rho + t,  rho' = 1 / Q.z,  J = a rho'^2 / rho^2,  s' = J^2 s + process_var[b],
//   (u2, v2) = the projection of Q,  (iu, iv) = the nearest pixel,  j = iv W + iu.
// depth_splat_kernel sends every candidate's key (bits of (float)rho', 0xFFFFFFFF - i) to keys[b, j] by one 64-bit atomicMax: the
// nearest surface wins, the smaller source index on equal fp32 keys, and a maximum does not depend on the order of arrival, so a repeat
// gives the same bits.  depth_fuse_kernel reads the key of every target, recomputes (rho', s') of the winning source with the same
// function (prop_pixel) and applies the fusion table; plain stores, no reduction, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"
#include "dense_reproj_dev.h"
#include "lie_dev.h"

using namespace islam;

namespace {

constexpr int FLAG_PROP = 1, FLAG_MEAS = 2, FLAG_GATED = 4;

// link b as the two kernels see it: where its state and variance lie, the user mask, the intrinsics, T^-1 = (R, t) and process_var[b]
struct PropLink {
    const double *rho, *var;
    const uint8_t* m;      // nullptr: no mask
    Intr in;
    int H, W;
    double R[9], t[3], pv;
};

// source pixel i carried into the next frame: cand (it lands on target j with a usable state), and rho' and s', formed whether or not
// it is a candidate
struct PropPixel {
    bool cand;
    int j;
    double rho, var;
};

// Nothing is contracted into an FMA: the two kernels inline this function into different surroundings, and from the same (R, t) they
// must form the same bits (the fuse kernel takes the winner's rho' and s' from here, after the splat kernel chose the winner by them).
ISLAM_DEV PropPixel prop_pixel(const PropLink& lk, int i) {
#pragma clang fp contract(off)
    PropPixel p{false, 0, 0.0, NAN};
    const int v = i / lk.W, u = i - v * lk.W;
    const double xh = ((double)u - lk.in.cx) / lk.in.fx, yh = ((double)v - lk.in.cy) / lk.in.fy;
    const double rho = lk.rho[i], s = lk.var[i];
    const bool usable = (lk.m ? lk.m[i] != 0 : true) && isfinite(rho) && rho > 0.0 && isfinite(s) && s > 0.0;
    const double* R = lk.R;
    const double dx = R[0] * xh + R[1] * yh + R[2];
    const double dy = R[3] * xh + R[4] * yh + R[5];
    const double a = R[6] * xh + R[7] * yh + R[8];
    const double Qx = dx / rho + lk.t[0], Qy = dy / rho + lk.t[1], Qz = a / rho + lk.t[2];
    const double rp = 1.0 / Qz;
    const double J = a * (rp * rp) / (rho * rho);
    const double sp = J * J * s + lk.pv;
    const double u2 = lk.in.fx * Qx / Qz + lk.in.cx, v2 = lk.in.fy * Qy / Qz + lk.in.cy;
    const double fu = floor(u2 + 0.5), fv = floor(v2 + 0.5);
    // the bounds are tested on the doubles (false for NaN), so the conversions below see values inside the image only
    p.rho = rp;
    p.var = sp;
    if (!(usable && Qz > 0.1 && fu >= 0.0 && fu < (double)lk.W && fv >= 0.0 && fv < (double)lk.H && isfinite(sp))) return p;
    p.cand = true;
    p.j = (int)fv * lk.W + (int)fu;
    return p;
}

// The head of both kernels: thread 0 decodes T^-1 into LDS, every thread takes the link from there.
ISLAM_DEV PropLink prop_link(const double* __restrict__ inv_depth, const double* __restrict__ var_inv_depth, const uint8_t* __restrict__ mask,
                             const double* __restrict__ motion, const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                             const double* __restrict__ process_var, int b, int H, int W) {
    __shared__ double Tp[12];
    if (threadIdx.x == 0) {
        const SE3<double> Ti = camera_inverse(motion + 7 * b, rgb2imu);
        m3_store(qmat(Ti.q), Tp);
        Tp[9] = Ti.t.x;
        Tp[10] = Ti.t.y;
        Tp[11] = Ti.t.z;
    }
    __syncthreads();
    const size_t off = (size_t)b * H * W;
    PropLink lk{inv_depth + off, var_inv_depth + off, mask ? mask + off : nullptr, intr_load(intr4 + 4 * b), H, W, {}, {}, process_var[b]};
#pragma unroll
    for (int k = 0; k < 9; ++k) lk.R[k] = Tp[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) lk.t[k] = Tp[9 + k];
    return lk;
}

// the status of link b: the incoming one if set, BADPRIOR for a process_var[b] that is negative or not finite, else OK
ISLAM_DEV int prop_status(const int* __restrict__ status, const double* __restrict__ process_var, int b) {
    const int s = status ? status[b] : ISLAM_DENSE_REPROJ_OK;
    if (s != ISLAM_DENSE_REPROJ_OK) return s;
    const double pv = process_var[b];
    return (isfinite(pv) && pv >= 0.0) ? ISLAM_DENSE_REPROJ_OK : ISLAM_DENSE_REPROJ_BADPRIOR;
}

// what the fuse kernel writes at one target
struct FusedPixel {
    double rho, var;
    float depth;
    int src, flags;
};

// One target of a link from its key and its measurement (has_meas: there is one; dn, vn: depth_next and var_next there): the winner's
// (rho', s') by prop_pixel, the fusion table.  Not contracted either, so the fused values are the individually rounded operations of
// the header's formulas.  live (uniform over the workgroup): the link propagates at all.
ISLAM_DEV FusedPixel fuse_target(const PropLink& lk, bool live, unsigned long long key, bool has_meas, float dn, float vn, double gate, double g2,
                                 int HW) {
#pragma clang fp contract(off)
    int src = -1;
    double rp = 0.0, sp = NAN;
    if (live) {
        const unsigned i = 0xFFFFFFFFu - (unsigned)key;
        // A key is the splat kernel's word that source i is a candidate for this target: it is not asked again.  (Both kernels decode
        // T^-1 with the same inlined code; were the two copies ever to differ in a last bit, rho' and s' would move by that bit and no
        // target would be dropped.)
        if (key != 0ull && i < (unsigned)HW) {
            const PropPixel p = prop_pixel(lk, (int)i);
            src = (int)i;
            rp = p.rho;
            sp = p.var;
        }
    }
    const double sm = has_meas ? (double)vn : NAN;
    const bool meas = has_meas && isfinite(dn) && dn > 0.0f && isfinite(sm) && sm > 0.0;
    const double rm = meas ? 1.0 / (double)dn : 0.0;
    int flags = (src >= 0 ? FLAG_PROP : 0) | (meas ? FLAG_MEAS : 0);
    double rf = 0.0, sf = NAN;
    if (src >= 0 && meas) {
        const double d = rp - rm, sum = sp + sm;
        if (gate > 0.0 && d * d > g2 * sum) {      // the hypotheses conflict: the measurement alone
            flags |= FLAG_GATED;
            rf = rm;
            sf = sm;
        } else {
            rf = (rp * sm + rm * sp) / sum;
            sf = sp * sm / sum;
        }
    } else if (src >= 0) {
        rf = rp;
        sf = sp;
    } else if (meas) {
        rf = rm;
        sf = sm;
    }
    return {rf, sf, rf > 0.0 ? (float)(1.0 / rf) : dn, src, flags};      // dn: the bits of depth_next, 0 without one
}

// grid (NBLK, B) x 256, grid-stride over the source pixels.  keys (B,H,W) was cleared on the same stream ahead of the launch.
__global__ __launch_bounds__(256) void depth_splat_kernel(const double* __restrict__ inv_depth, const double* __restrict__ var_inv_depth,
                                                           const uint8_t* __restrict__ mask, const double* __restrict__ motion,
                                                           const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                           const int* __restrict__ status, const double* __restrict__ process_var,
                                                           unsigned long long* __restrict__ keys, int H, int W) {
    const int b = blockIdx.y;
    const int HW = H * W;
    if (prop_status(status, process_var, b) != ISLAM_DENSE_REPROJ_OK) return;      // (uniform over the workgroup) nothing lands
    const PropLink lk = prop_link(inv_depth, var_inv_depth, mask, motion, rgb2imu, intr4, process_var, b, H, W);
    unsigned long long* kb = keys + (size_t)b * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) {
        const PropPixel p = prop_pixel(lk, i);
        if (!p.cand) continue;
        const unsigned long long key = ((unsigned long long)__float_as_uint((float)p.rho) << 32) | (0xFFFFFFFFu - (unsigned)i);
        atomicMax(kb + p.j, key);      // p.j lies in [0, HW): prop_pixel tested iu and iv against W and H
    }
}

// the same grid over the target pixels
__global__ __launch_bounds__(256) void depth_fuse_kernel(const double* __restrict__ inv_depth, const double* __restrict__ var_inv_depth,
                                                          const uint8_t* __restrict__ mask, const double* __restrict__ motion,
                                                          const double* __restrict__ rgb2imu, const double* __restrict__ intr4,
                                                          const int* __restrict__ status, const double* __restrict__ process_var,
                                                          const float* __restrict__ depth_next, const float* __restrict__ var_next, double gate,
                                                          const unsigned long long* __restrict__ keys, double* __restrict__ out_inv_depth,
                                                          double* __restrict__ out_var, float* __restrict__ out_depth,
                                                          int* __restrict__ out_source, uint8_t* __restrict__ out_flags,
                                                          int* __restrict__ out_status, int H, int W) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const size_t off = (size_t)b * HW;
    const int st = prop_status(status, process_var, b);
    if (blockIdx.x == 0 && threadIdx.x == 0) out_status[b] = st;
    const bool live = st == ISLAM_DENSE_REPROJ_OK;      // a link with a status: the measurement only, at every pixel
    PropLink lk{};
    if (live) lk = prop_link(inv_depth, var_inv_depth, mask, motion, rgb2imu, intr4, process_var, b, H, W);
    const double g2 = gate * gate;
    const unsigned long long* kb = keys + off;
    const float* dnb = depth_next ? depth_next + off : nullptr;
    const float* vnb = depth_next ? var_next + off : nullptr;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < HW; j += NBLK * 256) {
        const FusedPixel f = fuse_target(lk, live, live ? kb[j] : 0ull, dnb != nullptr, dnb ? dnb[j] : 0.0f, dnb ? vnb[j] : 0.0f, gate, g2, HW);
        out_inv_depth[off + j] = f.rho;
        out_var[off + j] = f.var;
        out_depth[off + j] = f.depth;
        out_source[off + j] = f.src;
        out_flags[off + j] = (uint8_t)f.flags;
    }
}

}  // namespace

extern "C" size_t islam_depth_propagate_scratch_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return align_up((size_t)B * H * W * sizeof(unsigned long long));
}

extern "C" int islam_depth_propagate(const double* inv_depth, const double* var_inv_depth, const uint8_t* mask_or_null, const double* motion,
                                     const double* rgb2imu_or_null, const double* intr4, const int* status_or_null, const double* process_var,
                                     const float* depth_next_or_null, const float* var_next_or_null, double gate, double* out_inv_depth,
                                     double* out_var, float* out_depth, int* out_source, uint8_t* out_flags, int* out_status, void* scratch,
                                     int B, int H, int W, void* stream) {
    const char* who = "islam_depth_propagate";
    // H W <= 2^30 (the family's bound) keeps a source index below 2^32 - 1, so a key of 0 can only mean "nothing landed here"
    if (int rc = check_shape_kind(who, B, H, W, ISLAM_ROBUST_NONE, 1.0)) return rc;
    if (!inv_depth || !var_inv_depth || !motion || !intr4 || !process_var)
        return fail(ISLAM_EARG, "%s: NULL inv_depth / var_inv_depth / motion / intr4 / process_var pointer", who);
    if (!out_inv_depth || !out_var || !out_depth || !out_source || !out_flags || !out_status || !scratch)
        return fail(ISLAM_EARG, "%s: NULL output / scratch pointer", who);
    if ((depth_next_or_null == nullptr) != (var_next_or_null == nullptr))
        return fail(ISLAM_EARG, "%s: depth_next and var_next come together or not at all", who);
    if (!(std::isfinite(gate) && gate >= 0.0)) return fail(ISLAM_EARG, "%s: gate must be finite and non-negative (got %g)", who, gate);
    hipStream_t s = as_stream(stream);
    unsigned long long* keys = static_cast<unsigned long long*>(scratch);
    ISLAM_HIP_CHECK(hipMemsetAsync(keys, 0, (size_t)B * H * W * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(depth_splat_kernel, dim3(NBLK, B), dim3(256), 0, s, inv_depth, var_inv_depth, mask_or_null, motion, rgb2imu_or_null,
                       intr4, status_or_null, process_var, keys, H, W);
    hipLaunchKernelGGL(depth_fuse_kernel, dim3(NBLK, B), dim3(256), 0, s, inv_depth, var_inv_depth, mask_or_null, motion, rgb2imu_or_null,
                       intr4, status_or_null, process_var, depth_next_or_null, var_next_or_null, gate, keys, out_inv_depth, out_var,
                       out_depth, out_source, out_flags, out_status, H, W);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}
