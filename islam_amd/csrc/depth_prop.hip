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
//
// depth_regularize_kernel (islam_depth_regularize) stands between the two when the caller asks for it: on the
// map a pure propagation returned it removes background seen through the holes of a magnified surface, fills holes from their
// neighbours and smooths every value over its compatible neighbours, a stencil on an LDS tile, and ends in the same fusion table.
//
// depth_prop_vjp_kernel and depth_prop_pose_kernel (islam_depth_propagate_vjp) are the vector-Jacobian product
// of the propagation on the piece its forward pass chose: the target pixel, the z-buffer winner and the row of the fusion table are
// read from out_source and out_flags, and the arithmetic of that piece is differentiated with plain stores and fixed-order sums.
//
// depth_reg_front_kernel, depth_reg_smooth_adj_kernel and depth_reg_fill_adj_kernel (islam_depth_regularize_vjp; DESIGN.md section
// 3.33) are the vector-Jacobian product of the regularisation on the piece its forward pass chose: the stencil's decisions are
// recomputed with the forward's own stage functions, and each stage's adjoint is a gather over its window.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"
#include "dense_reproj_dev.h"
#include "lie_dev.h"
#include "lie_vjp_dev.h"

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

// The fusion table at one target: the propagated hypothesis (have: there is one; rp, sp; src: what out_source gets) against the
// measurement (has_meas: the call has one; dn, vn: depth_next and var_next there).  Not contracted, so the fused values are the
// individually rounded operations of the header's formulas.  The fuse kernel and the regularisation kernel both end here.
ISLAM_DEV FusedPixel fuse_table(bool have, double rp, double sp, int src, bool has_meas, float dn, float vn, double gate, double g2) {
#pragma clang fp contract(off)
    const double sm = has_meas ? (double)vn : NAN;
    const bool meas = has_meas && isfinite(dn) && dn > 0.0f && isfinite(sm) && sm > 0.0;
    const double rm = meas ? 1.0 / (double)dn : 0.0;
    int flags = (have ? FLAG_PROP : 0) | (meas ? FLAG_MEAS : 0);
    double rf = 0.0, sf = NAN;
    if (have && meas) {
        const double d = rp - rm, sum = sp + sm;
        if (gate > 0.0 && d * d > g2 * sum) {      // the hypotheses conflict: the measurement alone
            flags |= FLAG_GATED;
            rf = rm;
            sf = sm;
        } else {
            rf = (rp * sm + rm * sp) / sum;
            sf = sp * sm / sum;
        }
    } else if (have) {
        rf = rp;
        sf = sp;
    } else if (meas) {
        rf = rm;
        sf = sm;
    }
    return {rf, sf, rf > 0.0 ? (float)(1.0 / rf) : dn, src, flags};      // dn: the bits of depth_next, 0 without one
}

// One target of a link from its key and its measurement: the winner's (rho', s') by prop_pixel, the fusion table.  live (uniform over
// the workgroup): the link propagates at all.
ISLAM_DEV FusedPixel fuse_target(const PropLink& lk, bool live, unsigned long long key, bool has_meas, float dn, float vn, double gate, double g2,
                                 int HW) {
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
    return fuse_table(src >= 0, rp, sp, src, has_meas, dn, vn, gate, g2);
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

// ------------------------------------------------------------------ regularisation of a propagated map
constexpr int FLAG_FILLED = 8, FLAG_REMOVED = 16;
constexpr int REG_TW = 32, REG_TH = 8;            // the output tile of a workgroup, one pixel per thread
constexpr int REG_RMAX = 2, REG_HALO = 3 * REG_RMAX;
constexpr int REG_CELLS = (REG_TW + 2 * REG_HALO) * (REG_TH + 2 * REG_HALO);      // 44 x 20

// the three stencil stages as the kernel takes them: the radii, the two counts, fill_inflate and reg_gate^2
struct RegStages {
    int r1, occl_min, r2, fill_min, r3;
    double inflate, g2;
};

// compat(k, j): (rho_k - rho_j)^2 <= reg_gate^2 (s_k + s_j); the same bits with k and j exchanged
ISLAM_DEV bool reg_compat(double rk, double sk, double rj, double sj, double g2) {
#pragma clang fp contract(off)
    const double d = rk - rj;
    return d * d <= g2 * (sk + sj);
}

// the status of link b: the incoming one if set, BADPRIOR for a dist_var[b] that is negative or not finite, else OK
ISLAM_DEV int reg_status(const int* __restrict__ status, const double* __restrict__ dist_var, int b) {
    const int s = status ? status[b] : ISLAM_DENSE_REPROJ_OK;
    if (s != ISLAM_DENSE_REPROJ_OK) return s;
    const double dv = dist_var[b];
    return (isfinite(dv) && dv >= 0.0) ? ISLAM_DENSE_REPROJ_OK : ISLAM_DENSE_REPROJ_BADPRIOR;
}

// A workgroup's LDS tile of link b: a 32 x 8 tile with a halo of h = r1 + r2 + r3.  The cell (lx, ly) of the (32 + 2h) x (8 + 2h) region
// is pixel (gx0 + lx, gy0 + ly), and a cell outside the image is not valid, which is all the clipping of a window at the border needs.
struct RegTile {
    double *rho, *var;
    uint8_t *v0, *rem, *fil;      // valid on input; removed by stage 1; filled by stage 2
    int h, LW, LH, gx0, gy0;
};

// The stage functions below are shared by depth_regularize_kernel and depth_reg_front_kernel (the gradient's recomputation): nothing
// in them is contracted, so both kernels form the same bits and take the same decisions from the same inputs.

// the tile of workgroup (tx, ty) over the LDS arrays of the caller
ISLAM_DEV RegTile reg_tile(double* srho, double* svar, uint8_t* sv0, uint8_t* srem, uint8_t* sfil, const RegStages& rs, int tx, int ty) {
    const int h = rs.r1 + rs.r2 + rs.r3;
    return {srho, svar, sv0, srem, sfil, h, REG_TW + 2 * h, REG_TH + 2 * h, tx * REG_TW - h, ty * REG_TH - h};
}

// the region from global memory (rho_b, var_b: the maps of the link), ending in a barrier
ISLAM_DEV void reg_tile_load(const RegTile& t, const double* __restrict__ rho_b, const double* __restrict__ var_b, int H, int W) {
#pragma clang fp contract(off)
    for (int c = threadIdx.x; c < t.LW * t.LH; c += 256) {
        const int ly = c / t.LW, lx = c - ly * t.LW;
        const int gx = t.gx0 + lx, gy = t.gy0 + ly;
        double r = 0.0, s = 0.0;
        bool ok = false;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            r = rho_b[gy * W + gx];
            s = var_b[gy * W + gx];
            ok = isfinite(r) && r > 0.0 && isfinite(s) && s > 0.0;
        }
        t.rho[c] = r;
        t.var[c] = s;
        t.v0[c] = ok;
        t.rem[c] = 0;
        t.fil[c] = 0;
    }
    __syncthreads();
}

// stage 1, occlusion removal on the region less r1: a cell with more nearer incompatible neighbours than compatible ones goes.  Ends in
// a barrier.
ISLAM_DEV void reg_stage_remove(const RegTile& t, const RegStages& rs) {
#pragma clang fp contract(off)
    const int o = rs.r1, w = t.LW - 2 * o, n = w * (t.LH - 2 * o);
    for (int c = threadIdx.x; c < n; c += 256) {
        const int ly = c / w, j = (ly + o) * t.LW + (c - ly * w) + o;
        if (!t.v0[j]) continue;
        const double rj = t.rho[j], sj = t.var[j];
        int nsup = 0, nocc = 0;
        for (int dv = -rs.r1; dv <= rs.r1; ++dv)
            for (int du = -rs.r1; du <= rs.r1; ++du) {
                const int k = j + dv * t.LW + du;
                if (k == j || !t.v0[k]) continue;
                const double rk = t.rho[k];
                if (reg_compat(rk, t.var[k], rj, sj, rs.g2))
                    ++nsup;
                else if (rk > rj)
                    ++nocc;
            }
        if (nocc >= rs.occl_min && nocc > nsup) t.rem[j] = 1;
    }
    __syncthreads();
}

// the cluster of a hole at cell j: the anchor (ka < 0: none; ra, sa), the members' count and their sums of w and w rho
struct RegCluster {
    int ka, cnt;
    double ra, sa, Sw, Swr;
};

// The cluster around the nearest valid1 neighbour of cell j within r2.  It reads valid1 cells only, which stage 2 never writes, so it
// gives the same bits before and after that stage.
ISLAM_DEV RegCluster reg_cluster(const RegTile& t, const RegStages& rs, int j) {
#pragma clang fp contract(off)
    RegCluster c{-1, 0, 0.0, 0.0, 0.0, 0.0};
    for (int dv = -rs.r2; dv <= rs.r2; ++dv)
        for (int du = -rs.r2; du <= rs.r2; ++du) {
            const int k = j + dv * t.LW + du;
            if (!t.v0[k] || t.rem[k]) continue;
            const double rk = t.rho[k];
            if (c.ka < 0 || rk > c.ra) {
                c.ka = k;
                c.ra = rk;
            }
        }
    if (c.ka < 0) return c;
    c.sa = t.var[c.ka];
    for (int dv = -rs.r2; dv <= rs.r2; ++dv)
        for (int du = -rs.r2; du <= rs.r2; ++du) {
            const int k = j + dv * t.LW + du;
            if (!t.v0[k] || t.rem[k]) continue;
            const double rk = t.rho[k], sk = t.var[k];
            if (!reg_compat(rk, sk, c.ra, c.sa, rs.g2)) continue;
            const double wk = 1.0 / sk;
            c.Sw = c.Sw + wk;
            c.Swr = c.Swr + wk * rk;
            ++c.cnt;
        }
    return c;
}

// stage 2, hole filling on the region less r1 + r2, in place: the cluster's weighted mean, one neighbour's variance plus the scatter.
// It writes only cells that are not valid after stage 1 and reads only cells that are, so no thread reads what another writes between
// two barriers.  Ends in a barrier.
ISLAM_DEV void reg_stage_fill(const RegTile& t, const RegStages& rs, int H, int W) {
#pragma clang fp contract(off)
    const int o = rs.r1 + rs.r2, w = t.LW - 2 * o, n = w * (t.LH - 2 * o);
    for (int c = threadIdx.x; c < n; c += 256) {
        const int ly = c / w + o, lx = c - (ly - o) * w + o, j = ly * t.LW + lx;
        const int gx = t.gx0 + lx, gy = t.gy0 + ly;
        if (gx < 0 || gx >= W || gy < 0 || gy >= H || (t.v0[j] && !t.rem[j])) continue;
        const RegCluster cl = reg_cluster(t, rs, j);
        if (cl.ka < 0 || cl.cnt < rs.fill_min) continue;
        const double mean = cl.Swr / cl.Sw;
        double Se = 0.0;
        for (int dv = -rs.r2; dv <= rs.r2; ++dv)
            for (int du = -rs.r2; du <= rs.r2; ++du) {
                const int k = j + dv * t.LW + du;
                if (!t.v0[k] || t.rem[k]) continue;
                const double rk = t.rho[k], sk = t.var[k];
                if (!reg_compat(rk, sk, cl.ra, cl.sa, rs.g2)) continue;
                const double e = rk - mean;
                Se = Se + (1.0 / sk) * (e * e);
            }
        t.rho[j] = mean;
        t.var[j] = rs.inflate * ((double)cl.cnt / cl.Sw + Se / cl.Sw);
        t.fil[j] = 1;
    }
    __syncthreads();
}

// the head of both kernels: the region loaded and stages 1 and 2 run on it (every thread of the workgroup calls it)
ISLAM_DEV void reg_stages_12(const RegTile& t, const RegStages& rs, const double* __restrict__ rho_b, const double* __restrict__ var_b, int H,
                             int W) {
    reg_tile_load(t, rho_b, var_b, H, W);
    if (rs.r1 > 0) reg_stage_remove(t, rs);
    if (rs.r2 > 0) reg_stage_fill(t, rs, H, W);
}

// the two sums of stage 3 at a present cell j of the tile with the stage-2 values (r2, s2): Sw = sum w_k, Swr = sum w_k rho_k over the
// compatible neighbours, j itself among them, so Sw > 0
struct RegSmooth {
    double Sw, Swr;
};

ISLAM_DEV RegSmooth reg_smooth_sums(const RegTile& t, const RegStages& rs, int j, double r2, double s2, double dvar) {
#pragma clang fp contract(off)
    RegSmooth m{0.0, 0.0};
    for (int dv = -rs.r3; dv <= rs.r3; ++dv)
        for (int du = -rs.r3; du <= rs.r3; ++du) {
            const int k = j + dv * t.LW + du;
            if (!((t.v0[k] && !t.rem[k]) || t.fil[k])) continue;
            const double rk = t.rho[k], sk = t.var[k];
            if (!reg_compat(rk, sk, r2, s2, rs.g2)) continue;
            const double wk = 1.0 / (sk + dvar * (double)(du * du + dv * dv));
            m.Sw = m.Sw + wk;
            m.Swr = m.Swr + wk * rk;
        }
    return m;
}

// grid (tiles_x tiles_y, B) x 256.  A workgroup owns a 32 x 8 tile of link b and holds it with a halo of h = r1 + r2 + r3 in LDS.
// Stage 1 marks the removed cells of the region less r1, stage 2 fills the cells of the region less r1 + r2 in place, stages 3 and 4
// run on the tile itself and store to global memory.  Every window is walked row by row, which is the order of the sums.
__global__ __launch_bounds__(256) void depth_regularize_kernel(const double* __restrict__ inv_depth, const double* __restrict__ var_inv_depth,
                                                                const int* __restrict__ source, const int* __restrict__ status,
                                                                const double* __restrict__ dist_var, const float* __restrict__ depth_next,
                                                                const float* __restrict__ var_next, double gate, RegStages rs,
                                                                double* __restrict__ out_inv_depth, double* __restrict__ out_var,
                                                                float* __restrict__ out_depth, int* __restrict__ out_source,
                                                                uint8_t* __restrict__ out_flags, int* __restrict__ out_status, int H, int W,
                                                                int tiles_x) {
#pragma clang fp contract(off)
    __shared__ double srho[REG_CELLS], svar[REG_CELLS];
    __shared__ uint8_t sv0[REG_CELLS], srem[REG_CELLS], sfil[REG_CELLS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const RegTile t = reg_tile(srho, svar, sv0, srem, sfil, rs, tx, ty);
    const size_t off = (size_t)b * H * W;
    const int st = reg_status(status, dist_var, b);
    if (blockIdx.x == 0 && tid == 0) out_status[b] = st;
    const bool live = st == ISLAM_DENSE_REPROJ_OK;      // (uniform over the workgroup) a link with a status: the measurement only
    if (live) reg_stages_12(t, rs, inv_depth + off, var_inv_depth + off, H, W);
    const int lx = (tid & (REG_TW - 1)) + t.h, ly = tid / REG_TW + t.h;
    const int gx = t.gx0 + lx, gy = t.gy0 + ly;
    if (gx >= W || gy >= H) return;      // past the last barrier
    const int j = ly * t.LW + lx, gj = gy * W + gx;
    bool have = false, kept = false;
    int extra = 0;
    double r3 = 0.0, s3 = NAN;
    if (live) {
        kept = sv0[j] && !srem[j];
        have = kept || sfil[j];
        extra = (sfil[j] ? FLAG_FILLED : 0) | (srem[j] ? FLAG_REMOVED : 0);
    }
    if (have) {
        r3 = srho[j];
        s3 = svar[j];
        if (rs.r3 > 0) {      // smoothing: the weighted mean over the compatible neighbours, the variance as it was
            const RegSmooth m = reg_smooth_sums(t, rs, j, r3, s3, dist_var[b]);
            r3 = m.Swr / m.Sw;
        }
    }
    const bool has_meas = depth_next != nullptr;
    const FusedPixel f = fuse_table(have, r3, s3, kept && source ? source[off + gj] : -1, has_meas, has_meas ? depth_next[off + gj] : 0.0f,
                                    has_meas ? var_next[off + gj] : 0.0f, gate, gate * gate);
    out_inv_depth[off + gj] = f.rho;
    out_var[off + gj] = f.var;
    out_depth[off + gj] = f.depth;
    out_source[off + gj] = f.src;
    out_flags[off + gj] = (uint8_t)(f.flags | extra);
}

// ------------------------------------------------------------------ the gradient of the propagation
// The map is piecewise smooth: the target pixel, the z-buffer winner and the row of the fusion table are constant on a piece, and the
// forward pass's source and flags say which piece a target is on.  The two kernels below take them as given and differentiate the
// arithmetic of that piece.  Since (u2, v2) only select a target, rho' and s' see the pose through a = R[2,:].ray and t_z alone.

// the cotangents of (rho', s') and of the measurement at one target
struct FuseGrad {
    double g_rp, g_sp, g_dn, g_vn;
};

// The fusion table differentiated at one target: gr, gs are the cotangents of rho_f and s_f (read by the caller only where flags is not
// 0), (rp, sp) the winner's hypothesis where flags has FLAG_PROP, (dn, vn) the measurement where it has FLAG_MEAS.
ISLAM_DEV FuseGrad fuse_grad(int flags, double gr, double gs, double rp, double sp, float dn, float vn) {
    FuseGrad g{0.0, 0.0, 0.0, 0.0};
    const bool prop = (flags & FLAG_PROP) != 0, meas = (flags & FLAG_MEAS) != 0, gated = (flags & FLAG_GATED) != 0;
    double g_rm = 0.0, g_sm = 0.0;
    if (prop && meas && !gated) {
        const double sm = (double)vn, rm = 1.0 / (double)dn, D = sp + sm;
        const double rf = (rp * sm + rm * sp) / D, wp = sm / D, wm = sp / D;
        g.g_rp = gr * wp;
        g_rm = gr * wm;
        g.g_sp = gr * ((rm - rf) / D) + gs * (wp * wp);
        g_sm = gr * ((rp - rf) / D) + gs * (wm * wm);
    } else if (meas) {      // measured only, or the gate chose the measurement
        g_rm = gr;
        g_sm = gs;
    } else if (prop) {
        g.g_rp = gr;
        g.g_sp = gs;
    }
    if (meas) {
        const double rm = 1.0 / (double)dn;
        g.g_dn = -(rm * rm) * g_rm;
        g.g_vn = g_sm;
    }
    return g;
}

// the cotangents of (rho, s) of source pixel i and of (a, t_z), with the ray of i for the pose sums
struct WarpGrad {
    double G_rho, G_s, G_a, G_tz, xh, yh;
};

// rho' = 1 / (a / rho + t_z) and s' = J^2 s + q differentiated at source pixel i (a usable one: the caller read it from source)
ISLAM_DEV WarpGrad warp_grad(const PropLink& lk, int i, double g_rp, double g_sp) {
    const int v = i / lk.W, u = i - v * lk.W;
    const double xh = ((double)u - lk.in.cx) / lk.in.fx, yh = ((double)v - lk.in.cy) / lk.in.fy;
    const double rho = lk.rho[i], s = lk.var[i];
    const double a = lk.R[6] * xh + lk.R[7] * yh + lk.R[8];
    const double rp = 1.0 / (a / rho + lk.t[2]), ir = 1.0 / rho;
    const double rp2 = rp * rp, J = a * rp2 * (ir * ir);
    const double g_J = 2.0 * J * s * g_sp;
    const double dJ_drho = 2.0 * J * (J / rp - ir), dJ_da = rp2 * (ir * ir) * (1.0 - 2.0 * a * rp * ir), dJ_dtz = -2.0 * J * rp;
    return {g_rp * J + g_J * dJ_drho, J * J * g_sp, g_J * dJ_da - g_rp * rp2 * ir, g_J * dJ_dtz - g_rp * rp2, xh, yh};
}

// grid (NBLK, B) x 256, grid-stride; every pixel index p is a target (the measurement's gradient, the four pose sums) and a source (its
// own gradient if it won its target, zeros if not).  partials (B, NBLK, 4): the workgroup's sums of G_a xh, G_a yh, G_a and G_tz.
__global__ __launch_bounds__(256) void depth_prop_vjp_kernel(const double* __restrict__ inv_depth, const double* __restrict__ var_inv_depth,
                                                              const double* __restrict__ motion, const double* __restrict__ rgb2imu,
                                                              const double* __restrict__ intr4, const double* __restrict__ process_var,
                                                              const float* __restrict__ depth_next, const float* __restrict__ var_next,
                                                              const int* __restrict__ source, const uint8_t* __restrict__ flags,
                                                              const int* __restrict__ out_status, const double* __restrict__ gout_rho,
                                                              const double* __restrict__ gout_var, double* __restrict__ grad_rho,
                                                              double* __restrict__ grad_var, float* __restrict__ grad_dn,
                                                              float* __restrict__ grad_vn, double* __restrict__ partials, int H, int W) {
    const int b = blockIdx.y;
    const int HW = H * W;
    const size_t off = (size_t)b * HW;
    const bool live = out_status[b] == ISLAM_DENSE_REPROJ_OK;      // (uniform over the workgroup) a link with a status propagated nothing
    PropLink lk{};
    if (live) lk = prop_link(inv_depth, var_inv_depth, nullptr, motion, rgb2imu, intr4, process_var, b, H, W);
    const int* sb = source + off;
    const uint8_t* fb = flags + off;
    const float* dnb = depth_next ? depth_next + off : nullptr;
    const float* vnb = depth_next ? var_next + off : nullptr;
    const double* grb = gout_rho ? gout_rho + off : nullptr;      // a NULL cotangent is zero
    const double* gsb = gout_var ? gout_var + off : nullptr;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += NBLK * 256) {
        {      // p as a target
            int fl = fb[p], src = -1;
            double rp = 0.0, sp = 0.0;
            if (live && (fl & FLAG_PROP)) {
                const int i = sb[p];
                if (i >= 0 && i < HW) {
                    const PropPixel w = prop_pixel(lk, i);
                    src = i;
                    rp = w.rho;
                    sp = w.var;
                }
            }
            if (src < 0) fl &= FLAG_MEAS;
            if (!dnb) fl &= ~(FLAG_MEAS | FLAG_GATED);
            // a cotangent is read only where the output depends on an input: where nothing is known it may be NaN
            const FuseGrad g = fuse_grad(fl, fl && grb ? grb[p] : 0.0, fl && gsb ? gsb[p] : 0.0, rp, sp, dnb ? dnb[p] : 0.0f, dnb ? vnb[p] : 0.0f);
            if (grad_dn) {
                grad_dn[off + p] = (float)g.g_dn;
                grad_vn[off + p] = (float)g.g_vn;
            }
            if (src >= 0) {
                const WarpGrad wg = warp_grad(lk, src, g.g_rp, g.g_sp);
                acc[0] += wg.G_a * wg.xh;
                acc[1] += wg.G_a * wg.yh;
                acc[2] += wg.G_a;
                acc[3] += wg.G_tz;
            }
        }
        double Gr = 0.0, Gs = 0.0;      // p as a source: exact zeros unless source says it won its target
        if (live) {
            const PropPixel me = prop_pixel(lk, p);      // me.j lies in [0, HW) where me.cand
            if (me.cand && sb[me.j] == p) {
                int fj = fb[me.j];
                if (!dnb) fj &= ~(FLAG_MEAS | FLAG_GATED);
                if (fj & FLAG_PROP) {
                    const FuseGrad g = fuse_grad(fj, grb ? grb[me.j] : 0.0, gsb ? gsb[me.j] : 0.0, me.rho, me.var, dnb ? dnb[me.j] : 0.0f,
                                                 dnb ? vnb[me.j] : 0.0f);
                    const WarpGrad wg = warp_grad(lk, p, g.g_rp, g.g_sp);
                    Gr = wg.G_rho;
                    Gs = wg.G_s;
                }
            }
        }
        grad_rho[off + p] = Gr;
        grad_var[off + p] = Gs;
    }
    reduce_and_store_row<4>(acc, partials + ((size_t)b * NBLK + blockIdx.x) * 4, true, 0.0);
}

// grid (B) x 64.  The NBLK rows of a link are summed in index order; lane 0 chains the cotangent of (R20, R21, R22, t_z) back through
// qmat, the inverse and the mount conjugation of camera_inverse to the plain components [t, q xyzw] of motion[b], every product taken
// as the forward pass writes it (no unit-norm assumption on a quaternion).  A link with a status gets seven zeros.
__global__ __launch_bounds__(64) void depth_prop_pose_kernel(const double* __restrict__ partials, const double* __restrict__ motion,
                                                              const double* __restrict__ rgb2imu, const int* __restrict__ out_status,
                                                              double* __restrict__ grad_motion) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ double s[4];
    if (i < 4) {
        double v = 0.0;
        for (int k = 0; k < NBLK; ++k) v += partials[((size_t)b * NBLK + k) * 4 + i];
        s[i] = v;
    }
    __syncthreads();
    if (i != 0) return;
    double* gm = grad_motion + (size_t)b * 7;
    if (out_status[b] != ISLAM_DENSE_REPROJ_OK) {
        for (int k = 0; k < 7; ++k) gm[k] = 0.0;
        return;
    }
    // forward: T = C^-1 M C (A = C^-1 M), Ti = T^-1 = (qi, ti), R = qmat(qi)
    const SE3<double> M = se3_load(motion + 7 * b);
    SE3<double> T = M, A = M, C{}, Ci{};
    if (rgb2imu) {
        C = se3_load(rgb2imu);
        Ci = se3_inv(C);
        A = se3_mul(Ci, M);
        T = se3_mul(A, C);
    }
    const Q4<double> qi = qinv(T.q);
    // R20 = 2 (x z - y w), R21 = 2 (y z + x w), R22 = 1 - 2 (x^2 + y^2) of qi
    const double g0 = 2.0 * s[0], g1 = 2.0 * s[1], g2 = 2.0 * s[2];
    Q4<double> gqi{g0 * qi.z + g1 * qi.w - 2.0 * g2 * qi.x, g1 * qi.z - g0 * qi.w - 2.0 * g2 * qi.y, g0 * qi.x + g1 * qi.y,
                   g1 * qi.x - g0 * qi.y};
    // ti = -qact(qi, T.t)
    Q4<double> gq;
    V3<double> gTt;
    qact_vjp(qi, T.t, v3(0.0, 0.0, -s[3]), gq, gTt);
    gqi = gqi + gq;
    const Q4<double> gTq{-gqi.x, -gqi.y, -gqi.z, gqi.w};
    V3<double> gMt = gTt;
    Q4<double> gMq = gTq;
    if (rgb2imu) {
        // T.t = A.t + qact(A.q, C.t), T.q = qmul(A.q, C.q);  A.t = Ci.t + qact(Ci.q, M.t), A.q = qmul(Ci.q, M.q)
        V3<double> unused;
        qact_vjp(A.q, C.t, gTt, gq, unused);
        const Q4<double> gAq = gq + qmul_vjp_a(gTq, C.q);
        qact_vjp(Ci.q, M.t, gTt, gq, gMt);
        gMq = qmul_vjp_b(Ci.q, gAq);
    }
    gm[0] = gMt.x; gm[1] = gMt.y; gm[2] = gMt.z; gm[3] = gMq.x; gm[4] = gMq.y; gm[5] = gMq.z; gm[6] = gMq.w;
}

// ------------------------------------------------------------------ the gradient of the regularisation
// The stencil is piecewise smooth: valid0, every compat decision, the removed set, each hole's anchor and cluster, the filled set,
// each pixel's smoothing set and the row of the fusion table are constant on a piece.  depth_reg_front_kernel recomputes stages 1-3
// with the forward's own functions (the same decisions from the same inputs), differentiates the fusion table and leaves per pixel
// what the two gathers need; depth_reg_smooth_adj_kernel is the adjoint of stage 3 and depth_reg_fill_adj_kernel that of stage 2 with
// the mask of stage 1.  Each output is one thread's fixed-order sum over a window, row by row: plain stores, no atomics.
constexpr int REG_ST_VALID1 = 1, REG_ST_FILLED = 2;      // the state byte of a pixel; 0: nothing present after stage 2
constexpr int REG_ADJ_CELLS = (REG_TW + 2 * REG_RMAX) * (REG_TH + 2 * REG_RMAX);      // 36 x 12: a gather's tile with a halo of 2

// the per-pixel maps between the three kernels, (B,H,W) each, carved from the caller's scratch
struct RegVjpMaps {
    double *rho2, *var2, *rho3, *S3, *g3r, *g3s;      // after stage 2; after stage 3 and its sum of weights; the cotangents of (rho3, s2)
    double *Sf, *ra, *sa;                             // at filled pixels: the cluster's sum of weights and the anchor
    double *g2r, *g2s;                                // the cotangents of (rho2, s2) (the g3 maps themselves where stage 3 is left out)
    uint8_t* state;
};

__global__ __launch_bounds__(256) void depth_reg_front_kernel(const double* __restrict__ inv_depth, const double* __restrict__ var_inv_depth,
                                                               const int* __restrict__ status, const double* __restrict__ dist_var,
                                                               const float* __restrict__ depth_next, const float* __restrict__ var_next,
                                                               RegStages rs, const uint8_t* __restrict__ flags,
                                                               const double* __restrict__ gout_rho, const double* __restrict__ gout_var,
                                                               float* __restrict__ grad_dn, float* __restrict__ grad_vn, RegVjpMaps mp, int H,
                                                               int W, int tiles_x) {
    __shared__ double srho[REG_CELLS], svar[REG_CELLS];
    __shared__ uint8_t sv0[REG_CELLS], srem[REG_CELLS], sfil[REG_CELLS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const RegTile t = reg_tile(srho, svar, sv0, srem, sfil, rs, tx, ty);
    const size_t off = (size_t)b * H * W;
    const bool live = reg_status(status, dist_var, b) == ISLAM_DENSE_REPROJ_OK;      // (uniform over the workgroup)
    if (live) reg_stages_12(t, rs, inv_depth + off, var_inv_depth + off, H, W);
    const int lx = (tid & (REG_TW - 1)) + t.h, ly = tid / REG_TW + t.h;
    const int gx = t.gx0 + lx, gy = t.gy0 + ly;
    if (gx >= W || gy >= H) return;      // past the last barrier
    const int j = ly * t.LW + lx;
    const size_t gj = off + (size_t)gy * W + gx;
    int state = 0;
    if (live) state = (sv0[j] && !srem[j] ? REG_ST_VALID1 : 0) | (sfil[j] ? REG_ST_FILLED : 0);
    double r2 = 0.0, s2 = 0.0, r3 = 0.0, S3 = 1.0;
    if (state) {
        r2 = srho[j];
        s2 = svar[j];
        r3 = r2;
        if (rs.r3 > 0) {
            const RegSmooth m = reg_smooth_sums(t, rs, j, r2, s2, dist_var[b]);
            S3 = m.Sw;
            r3 = m.Swr / m.Sw;      // the forward's own quotient
        }
    }
    int fl = flags[gj] & (FLAG_PROP | FLAG_MEAS | FLAG_GATED);      // the row the forward pass chose
    if (!state) fl &= FLAG_MEAS;
    if (!depth_next) fl &= ~(FLAG_MEAS | FLAG_GATED);
    // a cotangent is read only where the output depends on an input: where nothing is known it may be NaN
    const bool known = (fl & (FLAG_PROP | FLAG_MEAS)) != 0;
    const FuseGrad g = fuse_grad(fl, known && gout_rho ? gout_rho[gj] : 0.0, known && gout_var ? gout_var[gj] : 0.0, r3, s2,
                                 depth_next ? depth_next[gj] : 0.0f, depth_next ? var_next[gj] : 0.0f);
    if (grad_dn) {
        grad_dn[gj] = (float)g.g_dn;
        grad_vn[gj] = (float)g.g_vn;
    }
    mp.state[gj] = (uint8_t)state;
    if (!state) return;      // the gathers read the other maps only where the state is set
    mp.rho2[gj] = r2;
    mp.var2[gj] = s2;
    mp.rho3[gj] = r3;
    mp.S3[gj] = S3;
    mp.g3r[gj] = g.g_rp;
    mp.g3s[gj] = g.g_sp;
    if (state & REG_ST_FILLED) {
        const RegCluster cl = reg_cluster(t, rs, j);      // the cluster stage 2 filled this cell from: the same function, the same cells
        mp.Sf[gj] = cl.Sw;
        mp.ra[gj] = cl.ra;
        mp.sa[gj] = cl.sa;
    }
}

// a gather's 32 x 8 tile with a halo of r: cell (lx, ly) is pixel (x0 - r + lx, y0 - r + ly); LW = 32 + 2r
struct RegAdjTile {
    int r, LW, n, gx0, gy0;
};

ISLAM_DEV RegAdjTile reg_adj_tile(int r, int tiles_x) {
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    return {r, REG_TW + 2 * r, (REG_TW + 2 * r) * (REG_TH + 2 * r), tx * REG_TW - r, ty * REG_TH - r};      // n <= REG_ADJ_CELLS for r <= REG_RMAX
}

// The adjoint of stage 3, gathered at k over the outputs j of k's window that took k into their mean: g2r_k = sum g3r_j w_kj / S_j,
// g2s_k = g3s_k - sum g3r_j w_kj^2 (rho2_k - rho3_j) / S_j, w_kj = 1 / (s2_k + dist_var (du^2 + dv^2)).  compat gives the same bits with
// its arguments exchanged, so it is the decision output j took.  Launched only with r3 > 0.
__global__ __launch_bounds__(256) void depth_reg_smooth_adj_kernel(const double* __restrict__ dist_var, RegStages rs, RegVjpMaps mp, int H, int W,
                                                                    int tiles_x) {
    __shared__ double srho[REG_ADJ_CELLS], svar[REG_ADJ_CELLS], sr3[REG_ADJ_CELLS], sS[REG_ADJ_CELLS], sg[REG_ADJ_CELLS];
    __shared__ uint8_t sst[REG_ADJ_CELLS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const RegAdjTile t = reg_adj_tile(rs.r3, tiles_x);
    const size_t off = (size_t)b * H * W;
    for (int c = tid; c < t.n; c += 256) {
        const int ly = c / t.LW, lx = c - ly * t.LW;
        const int gx = t.gx0 + lx, gy = t.gy0 + ly;
        int st = 0;
        double r = 0.0, s = 0.0, r3 = 0.0, S = 1.0, g = 0.0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t gj = off + (size_t)gy * W + gx;
            st = mp.state[gj];
            if (st) {
                r = mp.rho2[gj];
                s = mp.var2[gj];
                r3 = mp.rho3[gj];
                S = mp.S3[gj];
                g = mp.g3r[gj];
            }
        }
        sst[c] = (uint8_t)st;
        srho[c] = r;
        svar[c] = s;
        sr3[c] = r3;
        sS[c] = S;
        sg[c] = g;
    }
    __syncthreads();
    const int lx = (tid & (REG_TW - 1)) + t.r, ly = tid / REG_TW + t.r;
    const int gx = t.gx0 + lx, gy = t.gy0 + ly;
    if (gx >= W || gy >= H) return;
    const int k = ly * t.LW + lx;
    if (!sst[k]) return;      // the next kernel reads g2 only where the state is set
    const size_t gk = off + (size_t)gy * W + gx;
    const double rk = srho[k], sk = svar[k], dvar = dist_var[b];
    double gr = 0.0, gs = mp.g3s[gk];
    for (int dv = -t.r; dv <= t.r; ++dv)
        for (int du = -t.r; du <= t.r; ++du) {
            const int j = k + dv * t.LW + du;
            if (!sst[j] || !reg_compat(rk, sk, srho[j], svar[j], rs.g2)) continue;
            const double w = 1.0 / (sk + dvar * (double)(du * du + dv * dv));
            const double q = sg[j] * w / sS[j];
            gr += q;
            gs -= q * w * (rk - sr3[j]);
        }
    mp.g2r[gk] = gr;
    mp.g2s[gk] = gs;
}

// The adjoint of stage 2 gathered at a valid1 k over the filled j within r2 whose cluster holds k (compat(k, a_j)), the mask of stage
// 1 and the final stores: with w = 1 / s_k, S the cluster's sum of weights, e = rho_k - rho2_j and f = fill_inflate,
//   g1r_k = g2r_k + sum (g2r_j w + g2s_j 2 f w e) / S,   g1s_k = g2s_k + sum (-g2r_j w^2 e + g2s_j w^2 (s2_j - f e^2)) / S,
// and exact zeros at every pixel that is not valid1.
__global__ __launch_bounds__(256) void depth_reg_fill_adj_kernel(RegStages rs, RegVjpMaps mp, double* __restrict__ grad_rho,
                                                                  double* __restrict__ grad_var, int H, int W, int tiles_x) {
    __shared__ double srho[REG_ADJ_CELLS], svar[REG_ADJ_CELLS], sgr[REG_ADJ_CELLS], sgs[REG_ADJ_CELLS], sSf[REG_ADJ_CELLS], sra[REG_ADJ_CELLS],
        ssa[REG_ADJ_CELLS];
    __shared__ uint8_t sst[REG_ADJ_CELLS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const RegAdjTile t = reg_adj_tile(rs.r2, tiles_x);
    const size_t off = (size_t)b * H * W;
    for (int c = tid; c < t.n; c += 256) {
        const int ly = c / t.LW, lx = c - ly * t.LW;
        const int gx = t.gx0 + lx, gy = t.gy0 + ly;
        int st = 0;
        double r = 0.0, s = 0.0, gr = 0.0, gs = 0.0, Sf = 1.0, ra = 0.0, sa = 0.0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t gj = off + (size_t)gy * W + gx;
            st = mp.state[gj];
            if (st) {
                r = mp.rho2[gj];
                s = mp.var2[gj];
                gr = mp.g2r[gj];
                gs = mp.g2s[gj];
            }
            if (st & REG_ST_FILLED) {
                Sf = mp.Sf[gj];
                ra = mp.ra[gj];
                sa = mp.sa[gj];
            }
        }
        sst[c] = (uint8_t)st;
        srho[c] = r;
        svar[c] = s;
        sgr[c] = gr;
        sgs[c] = gs;
        sSf[c] = Sf;
        sra[c] = ra;
        ssa[c] = sa;
    }
    __syncthreads();
    const int lx = (tid & (REG_TW - 1)) + t.r, ly = tid / REG_TW + t.r;
    const int gx = t.gx0 + lx, gy = t.gy0 + ly;
    if (gx >= W || gy >= H) return;
    const int k = ly * t.LW + lx;
    const size_t gk = off + (size_t)gy * W + gx;
    double gr = 0.0, gs = 0.0;
    if (sst[k] & REG_ST_VALID1) {
        const double rk = srho[k], sk = svar[k], w = 1.0 / sk;      // a valid1 pixel keeps its input through stage 2
        gr = sgr[k];
        gs = sgs[k];
        for (int dv = -t.r; dv <= t.r; ++dv)
            for (int du = -t.r; du <= t.r; ++du) {
                const int j = k + dv * t.LW + du;
                if (!(sst[j] & REG_ST_FILLED) || !reg_compat(rk, sk, sra[j], ssa[j], rs.g2)) continue;
                const double e = rk - srho[j], wS = w / sSf[j];
                gr += sgr[j] * wS + sgs[j] * (2.0 * rs.inflate * e * wS);
                gs += sgs[j] * (w * wS * (svar[j] - rs.inflate * (e * e))) - sgr[j] * (w * wS * e);
            }
    }
    grad_rho[gk] = gr;
    grad_var[gk] = gs;
}

}  // namespace

extern "C" size_t islam_depth_regularize_vjp_scratch_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const size_t n = (size_t)B * H * W;
    return 11 * align_up(n * sizeof(double)) + align_up(n);      // the maps of RegVjpMaps
}

extern "C" int islam_depth_regularize_vjp(const double* inv_depth, const double* var_inv_depth, const int* status_or_null, const double* dist_var,
                                          const float* depth_next_or_null, const float* var_next_or_null, double gate, int occl_radius,
                                          int occl_min, int fill_radius, int fill_min, double fill_inflate, int smooth_radius, double reg_gate,
                                          const uint8_t* flags, const double* grad_out_inv_depth_or_null, const double* grad_out_var_or_null,
                                          double* grad_inv_depth, double* grad_var_inv_depth, float* grad_depth_next_or_null,
                                          float* grad_var_next_or_null, void* scratch, int B, int H, int W, void* stream) {
    const char* who = "islam_depth_regularize_vjp";
    if (int rc = check_shape_kind(who, B, H, W, ISLAM_ROBUST_NONE, 1.0)) return rc;
    if (!inv_depth || !var_inv_depth || !dist_var || !flags)
        return fail(ISLAM_EARG, "%s: NULL inv_depth / var_inv_depth / dist_var / flags pointer", who);
    if (!grad_inv_depth || !grad_var_inv_depth || !scratch) return fail(ISLAM_EARG, "%s: NULL output / scratch pointer", who);
    if ((depth_next_or_null == nullptr) != (var_next_or_null == nullptr))
        return fail(ISLAM_EARG, "%s: depth_next and var_next come together or not at all", who);
    if ((grad_depth_next_or_null == nullptr) != (grad_var_next_or_null == nullptr))
        return fail(ISLAM_EARG, "%s: grad_depth_next and grad_var_next come together or not at all", who);
    if (grad_depth_next_or_null && !depth_next_or_null) return fail(ISLAM_EARG, "%s: a measurement gradient without a measurement", who);
    if (!(std::isfinite(gate) && gate >= 0.0)) return fail(ISLAM_EARG, "%s: gate must be finite and non-negative (got %g)", who, gate);
    for (int r : {occl_radius, fill_radius, smooth_radius})
        if (r < 0 || r > REG_RMAX)
            return fail(ISLAM_EARG, "%s: a radius must be 0..%d (got %d, %d, %d)", who, REG_RMAX, occl_radius, fill_radius, smooth_radius);
    if (occl_min < 1 || fill_min < 1) return fail(ISLAM_EARG, "%s: occl_min and fill_min must be at least 1 (got %d, %d)", who, occl_min, fill_min);
    if (!(std::isfinite(fill_inflate) && fill_inflate >= 1.0))
        return fail(ISLAM_EARG, "%s: fill_inflate must be finite and at least 1 (got %g)", who, fill_inflate);
    if (!(std::isfinite(reg_gate) && reg_gate > 0.0)) return fail(ISLAM_EARG, "%s: reg_gate must be finite and positive (got %g)", who, reg_gate);
    const int tiles_x = (W + REG_TW - 1) / REG_TW, tiles_y = (H + REG_TH - 1) / REG_TH;
    const RegStages rs{occl_radius, occl_min, fill_radius, fill_min, smooth_radius, fill_inflate, reg_gate * reg_gate};
    const size_t n = (size_t)B * H * W, step = align_up(n * sizeof(double));
    char* base = static_cast<char*>(scratch);
    double* d[11];
    for (int i = 0; i < 11; ++i) d[i] = reinterpret_cast<double*>(base + i * step);
    RegVjpMaps mp{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], reinterpret_cast<uint8_t*>(base + 11 * step)};
    if (smooth_radius == 0) {      // stage 3 left out: g2 = g3
        mp.g2r = mp.g3r;
        mp.g2s = mp.g3s;
    }
    hipStream_t s = as_stream(stream);
    const dim3 grid(tiles_x * tiles_y, B);
    hipLaunchKernelGGL(depth_reg_front_kernel, grid, dim3(256), 0, s, inv_depth, var_inv_depth, status_or_null, dist_var, depth_next_or_null,
                       var_next_or_null, rs, flags, grad_out_inv_depth_or_null, grad_out_var_or_null, grad_depth_next_or_null,
                       grad_var_next_or_null, mp, H, W, tiles_x);
    if (smooth_radius > 0) hipLaunchKernelGGL(depth_reg_smooth_adj_kernel, grid, dim3(256), 0, s, dist_var, rs, mp, H, W, tiles_x);
    hipLaunchKernelGGL(depth_reg_fill_adj_kernel, grid, dim3(256), 0, s, rs, mp, grad_inv_depth, grad_var_inv_depth, H, W, tiles_x);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" size_t islam_depth_propagate_vjp_scratch_bytes(int B) { return B < 1 ? 0 : align_up((size_t)B * NBLK * 4 * sizeof(double)); }

extern "C" int islam_depth_propagate_vjp(const double* inv_depth, const double* var_inv_depth, const double* motion, const double* rgb2imu_or_null,
                                         const double* intr4, const double* process_var, const float* depth_next_or_null,
                                         const float* var_next_or_null, const int* source, const uint8_t* flags, const int* out_status,
                                         const double* grad_out_inv_depth_or_null, const double* grad_out_var_or_null, double* grad_inv_depth,
                                         double* grad_var_inv_depth, double* grad_motion, float* grad_depth_next_or_null,
                                         float* grad_var_next_or_null, void* scratch, int B, int H, int W, void* stream) {
    const char* who = "islam_depth_propagate_vjp";
    if (int rc = check_shape_kind(who, B, H, W, ISLAM_ROBUST_NONE, 1.0)) return rc;
    if (!inv_depth || !var_inv_depth || !motion || !intr4 || !process_var || !source || !flags || !out_status)
        return fail(ISLAM_EARG, "%s: NULL inv_depth / var_inv_depth / motion / intr4 / process_var / source / flags / out_status pointer", who);
    if (!grad_inv_depth || !grad_var_inv_depth || !grad_motion || !scratch) return fail(ISLAM_EARG, "%s: NULL output / scratch pointer", who);
    if ((depth_next_or_null == nullptr) != (var_next_or_null == nullptr))
        return fail(ISLAM_EARG, "%s: depth_next and var_next come together or not at all", who);
    if ((grad_depth_next_or_null == nullptr) != (grad_var_next_or_null == nullptr))
        return fail(ISLAM_EARG, "%s: grad_depth_next and grad_var_next come together or not at all", who);
    if (grad_depth_next_or_null && !depth_next_or_null) return fail(ISLAM_EARG, "%s: a measurement gradient without a measurement", who);
    hipStream_t s = as_stream(stream);
    double* partials = static_cast<double*>(scratch);
    hipLaunchKernelGGL(depth_prop_vjp_kernel, dim3(NBLK, B), dim3(256), 0, s, inv_depth, var_inv_depth, motion, rgb2imu_or_null, intr4,
                       process_var, depth_next_or_null, var_next_or_null, source, flags, out_status, grad_out_inv_depth_or_null,
                       grad_out_var_or_null, grad_inv_depth, grad_var_inv_depth, grad_depth_next_or_null, grad_var_next_or_null, partials, H, W);
    hipLaunchKernelGGL(depth_prop_pose_kernel, dim3(B), dim3(64), 0, s, partials, motion, rgb2imu_or_null, out_status, grad_motion);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

extern "C" size_t islam_depth_regularize_scratch_bytes(int B, int H, int W) { return 0; }      // one fused launch: nothing in between

extern "C" int islam_depth_regularize(const double* inv_depth, const double* var_inv_depth, const int* source_or_null, const int* status_or_null,
                                      const double* dist_var, const float* depth_next_or_null, const float* var_next_or_null, double gate,
                                      int occl_radius, int occl_min, int fill_radius, int fill_min, double fill_inflate, int smooth_radius,
                                      double reg_gate, double* out_inv_depth, double* out_var, float* out_depth, int* out_source,
                                      uint8_t* out_flags, int* out_status, void* scratch, int B, int H, int W, void* stream) {
    const char* who = "islam_depth_regularize";
    if (int rc = check_shape_kind(who, B, H, W, ISLAM_ROBUST_NONE, 1.0)) return rc;
    if (!inv_depth || !var_inv_depth || !dist_var) return fail(ISLAM_EARG, "%s: NULL inv_depth / var_inv_depth / dist_var pointer", who);
    if (!out_inv_depth || !out_var || !out_depth || !out_source || !out_flags || !out_status)
        return fail(ISLAM_EARG, "%s: NULL output pointer", who);
    if ((depth_next_or_null == nullptr) != (var_next_or_null == nullptr))
        return fail(ISLAM_EARG, "%s: depth_next and var_next come together or not at all", who);
    if (!(std::isfinite(gate) && gate >= 0.0)) return fail(ISLAM_EARG, "%s: gate must be finite and non-negative (got %g)", who, gate);
    for (int r : {occl_radius, fill_radius, smooth_radius})
        if (r < 0 || r > REG_RMAX)
            return fail(ISLAM_EARG, "%s: a radius must be 0..%d (got %d, %d, %d)", who, REG_RMAX, occl_radius, fill_radius, smooth_radius);
    if (occl_min < 1 || fill_min < 1) return fail(ISLAM_EARG, "%s: occl_min and fill_min must be at least 1 (got %d, %d)", who, occl_min, fill_min);
    if (!(std::isfinite(fill_inflate) && fill_inflate >= 1.0))
        return fail(ISLAM_EARG, "%s: fill_inflate must be finite and at least 1 (got %g)", who, fill_inflate);
    if (!(std::isfinite(reg_gate) && reg_gate > 0.0)) return fail(ISLAM_EARG, "%s: reg_gate must be finite and positive (got %g)", who, reg_gate);
    const int tiles_x = (W + REG_TW - 1) / REG_TW, tiles_y = (H + REG_TH - 1) / REG_TH;      // H W <= 2^30: at most 2^30 tiles
    const RegStages rs{occl_radius, occl_min, fill_radius, fill_min, smooth_radius, fill_inflate, reg_gate * reg_gate};
    hipLaunchKernelGGL(depth_regularize_kernel, dim3(tiles_x * tiles_y, B), dim3(256), 0, as_stream(stream), inv_depth, var_inv_depth,
                       source_or_null, status_or_null, dist_var, depth_next_or_null, var_next_or_null, gate, rs, out_inv_depth, out_var,
                       out_depth, out_source, out_flags, out_status, H, W, tiles_x);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

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
