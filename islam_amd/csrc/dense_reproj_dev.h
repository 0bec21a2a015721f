// What the two dense reprojection files share (dense_reproj.hip: DESIGN.md sections 3.23 / 3.24; dense_ba.hip: sections 3.25 / 3.26).
// On the device: the camera-frame pose of a link, Ad(C^-1) and its transpose on a 6-vector, the head of the pixel loop (LinkPixels,
// pixel_in: the link's base pointers, u / v, the ray, the flow target, the mask byte), the per-pixel front of the five pixel kernels
// (reproj_pixel: back-projection, T^-1, the validity clauses, the residual, the robust kernel, dr/dQ and the rows of J_cam;
// robust_terms), the stores of the two VJP kernels (LinkGrads), the reduction epilogue of the three partial kernels, the 6x6 damped
// Cholesky step, the head and the tail of the two adjoint solve kernels (tangent_gradient, adjoint_solve_tail), and the body of the
// per-link final kernel -- the fixed-order sum of the NBLK workgroup rows, A = Ad(C^-1) applied once, and under refinement the LM
// bookkeeping of the link on lane 0.  On the host: the argument checks of the entry points and the size of the partial-sum scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "lie_dev.h"

namespace islam {
namespace {

constexpr int NS = ISLAM_DENSE_REPROJ_NSUM;
constexpr int NBLK = ISLAM_DENSE_REPROJ_NBLK;
constexpr int S_G = 21, S_COST = 27, S_L1 = 28, S_COUNT = 29;

// T^-1 = (C^-1 motion C)^-1; rgb2imu == nullptr: C = identity
ISLAM_DEV SE3<double> camera_inverse(const double* pose7, const double* rgb2imu) {
    SE3<double> T = se3_load(pose7);
    if (rgb2imu) {
        const SE3<double> C = se3_load(rgb2imu);
        T = se3_mul(se3_mul(se3_inv(C), T), C);
    }
    return se3_inv(T);
}

// C^-1 applied to a body-frame 6-vector, in place: Ad(C^-1) [rho; phi] = [R_c rho + t_c x (R_c phi); R_c phi].  TRANSPOSE: its
// transpose on a camera-frame 6-vector, Ad(C^-1)^T [rho; phi] = [R_c^T rho; R_c^T (phi - t_c x rho)]
template <bool TRANSPOSE = false>
ISLAM_DEV void adjoint_apply(const double* rgb2imu, V3<double>& rho3, V3<double>& phi3) {
    if (!rgb2imu) return;
    const SE3<double> Ci = se3_inv(se3_load(rgb2imu));
    const M3<double> Rc = qmat(Ci.q);
    if constexpr (TRANSPOSE) {
        phi3 = tmul(Rc, phi3 - cross(Ci.t, rho3));
        rho3 = tmul(Rc, rho3);
    } else {
        phi3 = Rc * phi3;
        rho3 = Rc * rho3 + cross(Ci.t, phi3);
    }
}

// a body-frame 6-vector into the camera frame: dst6 = Ad(C^-1) src6 (one thread; dst6 is LDS in the joint kernels)
ISLAM_DEV void adjoint_to_camera(const double* rgb2imu, const double* src6, double* dst6) {
    V3<double> r{src6[0], src6[1], src6[2]}, f{src6[3], src6[4], src6[5]};
    adjoint_apply(rgb2imu, r, f);
    dst6[0] = r.x; dst6[1] = r.y; dst6[2] = r.z; dst6[3] = f.x; dst6[4] = f.y; dst6[5] = f.z;
}

// The robust kernel at s = |r|^2: rho(s), c = rho'(s), cp = dc/ds.  The one place the Huber / Cauchy branches live; what a caller
// does not use falls away once this is inlined.
ISLAM_DEV void robust_terms(int kind, double delta, double d2, double s, double& rho, double& c, double& cp) {
    rho = s;
    c = 1.0;
    cp = 0.0;
    if (kind == ISLAM_ROBUST_HUBER) {
        if (s > d2) {
            const double rs = sqrt(s);
            rho = 2.0 * delta * rs - d2;
            c = delta / rs;
            cp = -delta / (2.0 * s * rs);
        }
    } else if (kind == ISLAM_ROBUST_CAUCHY) {
        const double k = 1.0 + s / d2;
        rho = d2 * log1p(s / d2);
        c = 1.0 / k;
        cp = -1.0 / (d2 * k * k);
    }
}

struct Intr {
    double fx, fy, cx, cy;
};

ISLAM_DEV Intr intr_load(const double* intr4) { return {intr4[0], intr4[1], intr4[2], intr4[3]}; }

// The head of the pixel loop.  LinkPixels: link b as the pixel kernels see it -- where its depth, flow and mask lie, its intrinsics and
// the robust kernel; PixelIn: pixel i as the front takes it -- the stored depth z, the ray (xh, yh, 1), (tu, tv) = where the flow says
// the pixel went, and m = the user mask.
struct LinkPixels {
    const float *z, *fu, *fv;
    const uint8_t* m;      // nullptr: no mask
    Intr in;
    int W, kind;
    double delta, d2;
};

ISLAM_DEV LinkPixels link_pixels(const float* depth, const float* flow, const uint8_t* mask, const double* intr4, int b, int HW, int W,
                                 int kind, double delta) {
    const size_t off = (size_t)b * HW;
    const float* fu = flow + 2 * off;
    return {depth + off, fu, fu + HW, mask ? mask + off : nullptr, intr_load(intr4 + 4 * b), W, kind, delta, delta * delta};
}

struct PixelIn {
    double z, xh, yh, tu, tv;
    bool m;
};

ISLAM_DEV PixelIn pixel_in(const LinkPixels& lp, int i) {
    const int v = i / lp.W, u = i - v * lp.W;
    const double ud = (double)u, vd = (double)v;
    return {(double)lp.z[i], (ud - lp.in.cx) / lp.in.fx, (vd - lp.in.cy) / lp.in.fy, (double)lp.fu[i] + ud, (double)lp.fv[i] + vd,
            lp.m ? lp.m[i] != 0 : true};
}

// one pixel at T^-1 = (R, t): everything ahead of the accumulators.  dr/dQ = [[a, 0, bq], [0, cq, dq]], iz = 1 / Q_z, and ju, jv: the
// two rows of J_cam = dr/dQ [-I, [Q]x]
struct Pixel {
    bool valid;
    double ru, rv, s, rob, c, cp;
    V3<double> Q;
    double iz, a, bq, cq, dq, ju[6], jv[6];
};

// The per-pixel front.  z: the depth along the ray of q (q.z, or 1 / rho in the joint kernels).  Straight-line: an invalid pixel carries
// numbers nobody may use; what a caller does not read (the rows in the gradient kernel) falls away once this is inlined.
ISLAM_DEV Pixel reproj_pixel(const M3<double>& R, const V3<double>& t, double z, const PixelIn& q, const LinkPixels& lp) {
    Pixel p;
    const Intr& in = lp.in;
    const V3<double> P{z * q.xh, z * q.yh, z};
    p.Q = R * P + t;
    p.valid = q.m && p.Q.z > 0.1;
    const double px = p.Q.x / p.Q.z, py = p.Q.y / p.Q.z;
    p.valid = p.valid && fabs(px) <= 1.0 && fabs(py) <= 1.0;
    p.ru = in.fx * px + in.cx - q.tu;
    p.rv = in.fy * py + in.cy - q.tv;
    p.s = p.ru * p.ru + p.rv * p.rv;
    robust_terms(lp.kind, lp.delta, lp.d2, p.s, p.rob, p.c, p.cp);
    // dr/dQ in locals and the rows right here, not in a function of their own: with either the compiler contracts the sums over
    // column 2 of J_cam (-bq, -dq) into other FMAs, and the joint kernel's last bits move
    const V3<double>& Q = p.Q;
    const double iz = 1.0 / Q.z;
    const double a = in.fx * iz, bq = -(a * px), cq = in.fy * iz, dq = -(cq * py);
    p.ju[0] = -a; p.ju[1] = 0.0; p.ju[2] = -bq; p.ju[3] = -bq * Q.y; p.ju[4] = bq * Q.x - a * Q.z; p.ju[5] = a * Q.y;
    p.jv[0] = 0.0; p.jv[1] = -cq; p.jv[2] = -dq; p.jv[3] = cq * Q.z - dq * Q.y; p.jv[4] = dq * Q.x; p.jv[5] = -cq * Q.x;
    p.iz = iz; p.a = a; p.bq = bq; p.cq = cq; p.dq = dq;
    return p;
}

// Where a VJP kernel writes the gradients of link b: three float stores per pixel, and zeros over the whole link for one without a
// gradient, whatever its pixels hold.
struct LinkGrads {
    float *z, *u, *v;
};

ISLAM_DEV LinkGrads link_grads(float* grad_depth, float* grad_flow, int b, int HW) {
    const size_t off = (size_t)b * HW;
    float* gu = grad_flow + 2 * off;
    return {grad_depth + off, gu, gu + HW};
}

ISLAM_DEV void grad_store(const LinkGrads& g, int i, double gz, double gu, double gv) {
    g.z[i] = (float)gz; g.u[i] = (float)gu; g.v[i] = (float)gv;
}

ISLAM_DEV void grad_zero_link(const LinkGrads& g, int HW) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += NBLK * 256) g.z[i] = g.u[i] = g.v[i] = 0.0f;
}

// The epilogue of a partial kernel (256 threads): the workgroup's sum of every accumulator, one row of N by plain stores.
// ok = false stores bad: NaN, which the final kernel reports (the sums), or 0 (the adjoint's row of six, section 3.26).
template <int N>
ISLAM_DEV void reduce_and_store_row(const double* acc, double* __restrict__ row, bool ok, double bad) {
    __shared__ double red[4][N];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double x = acc[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) red[wv][i] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) row[threadIdx.x] = ok ? red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] : bad;
}

// what the final kernel writes per link; under refinement these arrays ARE the link's current state
struct Outputs {
    double *H, *g, *cost, *l1, *count, *sums;
};

// the LM bookkeeping of refinement (motion == nullptr: normal equations only)
struct Refine {
    double* motion;        // (B,7) current pose
    double* trial;         // (B,7) next pose to evaluate
    double* lambda;        // (B)
    int *accepted, *rejected, *status;
    double* trace;         // (trace_cap,B) mean cost of each evaluation, or nullptr
    int trace_cap;
    int eval;              // index of this evaluation
    int last;              // no further evaluation follows
    double min_count, lambda0;
};

// what the joint (pose, inverse depth) refinement keeps beside Refine (section 3.25)
struct Joint {
    const double* prior_weight;   // (B) w; a link with w <= 0 (or NaN) gets ISLAM_DENSE_REPROJ_BADPRIOR at evaluation 0
    double* delta;                // (B,6) the pose step that led to the trial pose, for the next evaluation's back-substitution
    int* select;                  // (B) which of the two inverse-depth buffers holds the link's current state
};

// index of (i, j), i <= j, in the row-major upper triangle of a 6x6
ISLAM_DEV int tri(int i, int j) { return i * (11 - i) / 2 + j; }

// (H + lambda diag H) x = -g by Cholesky, everything in LDS (runtime-indexed: private arrays would go to scratch memory);
// false on a non-positive (or NaN) pivot
ISLAM_DEV bool lm_step(const double* Hn, const double* gn, double lambda, double (*L)[6], double* x) {
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) L[i][j] = Hn[i * 6 + j] + (i == j ? lambda * Hn[i * 6 + i] : 0.0);
    for (int j = 0; j < 6; ++j) {
        double d = L[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        L[j][j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double v = L[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / d;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = -gn[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * x[k];
        x[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = x[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    return true;
}

// A loss's gradient on [t, q xyzw] in the right tangent of the pose, v = dL/dxi on motion Exp(xi): v_rho = R^T dL/dt, v_phi = 1/2 E^T dL/dq
// with E = d(q (x, 1))/dx at 0 = [[q_w I + [q_v]x], [-q_v^T]]
ISLAM_DEV void tangent_gradient(const double* motion7, const double* gm, V3<double>& vr, V3<double>& vf) {
    const SE3<double> X = se3_load(motion7);
    vr = tmul(qmat(X.q), v3(gm[0], gm[1], gm[2]));
    const V3<double> qv{X.q.x, X.q.y, X.q.z}, gq{gm[3], gm[4], gm[5]};
    vf = 0.5 * (X.q.w * gq - cross(qv, gq) - gm[6] * qv);
}

// The tail of an adjoint solve kernel (64 threads; Hn, vn, L, x in LDS, vn written by lane 0 or ahead of a barrier): x = -Hn^-1 vn for
// a link that comes with s = OK, the link's status out, and its row of six -- zeros for a link with a status or a non-positive pivot.
ISLAM_DEV void adjoint_solve_tail(int s, const double* Hn, const double* vn, double (*L)[6], double* x, int* status_out, double* row) {
    __shared__ int st;
    if (threadIdx.x == 0) {
        if (s == ISLAM_DENSE_REPROJ_OK && !lm_step(Hn, vn, 0.0, L, x)) s = ISLAM_DENSE_REPROJ_NOTPD;
        st = s;
        *status_out = s;
    }
    __syncthreads();
    if (threadIdx.x < 6) row[threadIdx.x] = st == ISLAM_DENSE_REPROJ_OK ? x[threadIdx.x] : 0.0;
}

// The final kernel of a link: one 64-lane workgroup.  JOINT = false is dense_reproj_final_kernel as section 3.23 describes it;
// JOINT = true (dense_ba_final_kernel) additionally refuses a non-positive prior weight, leaves the pose step for the next
// evaluation's back-substitution and flips the link's inverse-depth selector when the trial is taken.
template <bool JOINT>
ISLAM_DEV void final_body(const double* __restrict__ partial, const double* __restrict__ rgb2imu, const double* __restrict__ pose_eval,
                          Outputs out, Refine rf, Joint jt, int B) {
    const int b = blockIdx.x, i = threadIdx.x;
    __shared__ double s[NS], Rm[9], Sm[9], A[36], Hn[36], gn[6], L[6][6], x[6], cur[7];
    __shared__ int take;
    if (i < NS) {
        double v = 0.0;
        for (int k = 0; k < NBLK; ++k) v += partial[((size_t)b * NBLK + k) * NS + i];
        s[i] = v;
    }
    if (i == 0) {      // C^-1 = (R, t)
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
    if (i < 36) {      // H = A^T H_cam A; (r, c) and (c, r) run the same operations, so H is symmetric to the bit
        const int r0 = i / 6, c0 = i - 6 * r0;
        const int r = min(r0, c0), c = max(r0, c0);
        double v = 0.0;
        for (int k = 0; k < 6; ++k) {
            double w = 0.0;
            for (int l = 0; l < 6; ++l) w += s[tri(min(k, l), max(k, l))] * A[l * 6 + c];
            v += A[k * 6 + r] * w;
        }
        Hn[i] = v;
    } else if (i < 42) {
        const int r = i - 36;
        double v = 0.0;
        for (int k = 0; k < 6; ++k) v += A[k * 6 + r] * s[S_G + k];
        gn[r] = v;
    }
    __syncthreads();

    const bool refine = rf.motion != nullptr;
    if (refine && i == 0) {
        bool finite = true;
        for (int k = 0; k < NS; ++k) finite = finite && isfinite(s[k]);
        const double n = s[S_COUNT];
        int acc = 0;
        if (rf.eval == 0) {        // the state at the pose as given
            acc = 1;
            rf.lambda[b] = rf.lambda0;
            rf.accepted[b] = 0;
            rf.rejected[b] = 0;
            if constexpr (JOINT)
                rf.status[b] = !(jt.prior_weight[b] > 0.0)      ? ISLAM_DENSE_REPROJ_BADPRIOR
                               : (finite && n >= rf.min_count) ? ISLAM_DENSE_REPROJ_OK
                                                               : ISLAM_DENSE_REPROJ_FEW;
            else
                rf.status[b] = (finite && n >= rf.min_count) ? ISLAM_DENSE_REPROJ_OK : ISLAM_DENSE_REPROJ_FEW;
            if constexpr (JOINT) jt.select[b] = 0;         // evaluation 0 wrote the prior into buffer 0
        } else if (rf.status[b] == ISLAM_DENSE_REPROJ_OK) {
            // the MEAN is compared: the pixel set moves with the pose, and losing pixels must not count as progress
            acc = finite && n >= rf.min_count && s[S_COST] / n < out.cost[b] / out.count[b];
            if (acc) {
                rf.lambda[b] = fmax(rf.lambda[b] / 10.0, ISLAM_DENSE_REPROJ_LAMBDA_MIN);
                rf.accepted[b] += 1;
                if constexpr (JOINT) jt.select[b] ^= 1;    // the trial inverse depths become the state
            } else {
                rf.lambda[b] = fmin(rf.lambda[b] * 10.0, ISLAM_DENSE_REPROJ_LAMBDA_MAX);
                rf.rejected[b] += 1;
            }
        }
        if (rf.trace && rf.eval < rf.trace_cap) rf.trace[(size_t)rf.eval * B + b] = s[S_COST] / n;
        take = acc;
    }
    if (!refine && i == 0) take = 1;
    __syncthreads();
    if (take) {
        if (i < 36) out.H[(size_t)b * 36 + i] = Hn[i];
        if (i < 6) out.g[(size_t)b * 6 + i] = gn[i];
        if (i < NS) out.sums[(size_t)b * NS + i] = s[i];
        if (i == 0) {
            out.cost[b] = s[S_COST];
            out.l1[b] = s[S_L1];
            out.count[b] = s[S_COUNT];
        }
        if (refine && i < 7) {
            cur[i] = pose_eval[(size_t)b * 7 + i];
            rf.motion[(size_t)b * 7 + i] = cur[i];
        }
    } else {           // (refinement only) the step below starts from the state an earlier evaluation left
        if (i < 36) Hn[i] = out.H[(size_t)b * 36 + i];
        if (i < 6) gn[i] = out.g[(size_t)b * 6 + i];
        if (i < 7) cur[i] = rf.motion[(size_t)b * 7 + i];
    }
    if (!refine || rf.last) return;
    __syncthreads();
    if (i == 0) {
        SE3<double> X = se3_load(cur);
        if (rf.status[b] == ISLAM_DENSE_REPROJ_OK) {
            if (lm_step(Hn, gn, rf.lambda[b], L, x)) {
                X = se3_mul(X, se3_exp(v3(x[0], x[1], x[2]), v3(x[3], x[4], x[5])));
                const double qn = 1.0 / sqrt(X.q.x * X.q.x + X.q.y * X.q.y + X.q.z * X.q.z + X.q.w * X.q.w);
                X.q = {qn * X.q.x, qn * X.q.y, qn * X.q.z, qn * X.q.w};
                if constexpr (JOINT)
                    for (int k = 0; k < 6; ++k) jt.delta[(size_t)b * 6 + k] = x[k];
            } else {
                rf.status[b] = ISLAM_DENSE_REPROJ_NOTPD;
            }
        }
        se3_store(X, rf.trial + (size_t)b * 7);      // a link whose status is set keeps being evaluated where it stands
    }
}

// ------------------------------------------------------------------ host side: the argument checks of the entry points
inline size_t partial_bytes(int B) { return align_up((size_t)B * NBLK * NS * sizeof(double)); }

inline int check_shape_kind(const char* who, int B, int H, int W, int kind, double delta) {
    if (B < 1 || H < 1 || W < 1 || (long long)H * W > (1ll << 30)) return fail(ISLAM_EARG, "%s: bad shape (%d,%d,%d)", who, B, H, W);
    if (kind != ISLAM_ROBUST_NONE && kind != ISLAM_ROBUST_HUBER && kind != ISLAM_ROBUST_CAUCHY)
        return fail(ISLAM_EARG, "%s: unknown robust kind %d", who, kind);
    if (!(delta > 0.0)) return fail(ISLAM_EARG, "%s: robust delta must be positive (got %g)", who, delta);
    return ISLAM_OK;
}

// prior_ok: the joint entry points pass prior_weight != nullptr
inline int check_common(const char* who, const float* depth, const float* flow, const double* motion, const double* intr4, int kind,
                        double delta, const Outputs& o, const void* scratch, int B, int H, int W, bool prior_ok = true) {
    if (int rc = check_shape_kind(who, B, H, W, kind, delta)) return rc;
    if (!depth || !flow || !motion || !intr4 || !o.H || !o.g || !o.cost || !o.l1 || !o.count || !o.sums || !scratch)
        return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 / output / scratch pointer", who);
    if (!prior_ok) return fail(ISLAM_EARG, "%s: NULL prior_weight", who);
    return ISLAM_OK;
}

// what the two entry points of the joint adjoint (section 3.26) share; lambda_p is an output of one and an input of the other
inline int check_joint_adjoint(const char* who, const float* depth, const float* flow, const double* motion, const double* intr4,
                               const double* prior_weight, const double* inv_depth, const double* lambda_p, int kind, double delta, int B,
                               int H, int W) {
    if (int rc = check_shape_kind(who, B, H, W, kind, delta)) return rc;
    if (!depth || !flow || !motion || !intr4) return fail(ISLAM_EARG, "%s: NULL depth / flow / motion / intr4 pointer", who);
    if (!prior_weight) return fail(ISLAM_EARG, "%s: NULL prior_weight", who);
    if (!inv_depth || !lambda_p) return fail(ISLAM_EARG, "%s: NULL inv_depth / lambda_p pointer", who);
    return ISLAM_OK;
}

// the LM arguments of a _refine entry point, from rf as the entry point filled it; trace: the pointer as the caller gave it
inline int check_refine(const char* who, int iters, const Refine& rf, const double* trace) {
    if (iters < 1) return fail(ISLAM_EARG, "%s: iters must be at least 1 (got %d)", who, iters);
    if (!(rf.lambda0 >= 0.0) || !(rf.min_count >= 0.0)) return fail(ISLAM_EARG, "%s: damping and min_count must be non-negative", who);
    if (!rf.motion || !rf.lambda || !rf.accepted || !rf.rejected || !rf.status)
        return fail(ISLAM_EARG, "%s: NULL out_motion / out_lambda / out_accepted / out_rejected / out_status", who);
    if (rf.trace_cap < 0 || (rf.trace_cap > 0 && !trace)) return fail(ISLAM_EARG, "%s: trace_cap %d without a trace buffer", who, rf.trace_cap);
    return ISLAM_OK;
}

}  // namespace
}  // namespace islam
