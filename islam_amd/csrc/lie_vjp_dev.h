// Cotangents through the quaternion algebra of lie_dev.h, for the kernels that chain a gradient on T^-1 = camera_inverse(motion, rgb2imu)
// back to the plain components [t, q xyzw] of motion (depth_prop.hip: DESIGN.md section 3.31; dense_ba.hip: section 3.32).  Every
// product is taken as the forward pass writes it: no unit-norm assumption on a quaternion.
#pragma once
#include <hip/hip_runtime.h>

#include "lie_dev.h"

namespace islam {

// the cotangents of q and p in r = qact(q, p) = p + q.w uv + u x uv, uv = 2 u x p, from the cotangent g of r
ISLAM_DEV void qact_vjp(Q4<double> q, V3<double> p, V3<double> g, Q4<double>& gq, V3<double>& gp) {
    const V3<double> u{q.x, q.y, q.z};
    const V3<double> uv = 2.0 * cross(u, p);
    const V3<double> guv = q.w * g + cross(g, u);
    const V3<double> gu = cross(uv, g) + 2.0 * cross(p, guv);
    gq = {gu.x, gu.y, gu.z, dot(g, uv)};
    gp = g + 2.0 * cross(guv, u);
}

// the cotangents of a and b in qmul(a, b) from the cotangent g of the product
ISLAM_DEV Q4<double> qmul_vjp_a(Q4<double> g, Q4<double> b) {
    return {g.x * b.w - g.y * b.z + g.z * b.y - g.w * b.x, g.x * b.z + g.y * b.w - g.z * b.x - g.w * b.y,
            -g.x * b.y + g.y * b.x + g.z * b.w - g.w * b.z, g.x * b.x + g.y * b.y + g.z * b.z + g.w * b.w};
}
ISLAM_DEV Q4<double> qmul_vjp_b(Q4<double> a, Q4<double> g) {
    return {g.x * a.w + g.y * a.z - g.z * a.y - g.w * a.x, -g.x * a.z + g.y * a.w + g.z * a.x - g.w * a.y,
            g.x * a.y - g.y * a.x + g.z * a.w - g.w * a.z, g.x * a.x + g.y * a.y + g.z * a.z + g.w * a.w};
}
ISLAM_DEV Q4<double> operator+(Q4<double> a, Q4<double> b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// the cotangent of q in R = qmat(q) from the cotangent G (row-major 3x3) of R
ISLAM_DEV Q4<double> qmat_vjp(Q4<double> q, const double* G) {
    const double x = q.x, y = q.y, z = q.z, w = q.w;
    return {2.0 * ((G[1] + G[3]) * y + (G[2] + G[6]) * z + (G[7] - G[5]) * w - 2.0 * (G[4] + G[8]) * x),
            2.0 * ((G[1] + G[3]) * x + (G[5] + G[7]) * z + (G[2] - G[6]) * w - 2.0 * (G[0] + G[8]) * y),
            2.0 * ((G[2] + G[6]) * x + (G[5] + G[7]) * y + (G[3] - G[1]) * w - 2.0 * (G[0] + G[4]) * z),
            2.0 * ((G[7] - G[5]) * x + (G[2] - G[6]) * y + (G[3] - G[1]) * z)};
}

// The cotangents GR (row-major 3x3) and gt of (R, t) = T^-1, T^-1 = (qi, ti) = camera_inverse(motion7, rgb2imu) with R = qmat(qi), chained
// through the inverse and the mount conjugation T = C^-1 M C to the plain components of M = motion7: gm[0..6] = [t, q xyzw].
ISLAM_DEV void camera_inverse_vjp(const double* motion7, const double* rgb2imu, const double* GR, V3<double> gt, double* gm) {
    // forward: T = C^-1 M C (A = C^-1 M), Ti = T^-1 = (qi, ti), ti = -qact(qi, T.t)
    const SE3<double> M = se3_load(motion7);
    SE3<double> T = M, A = M, C{}, Ci{};
    if (rgb2imu) {
        C = se3_load(rgb2imu);
        Ci = se3_inv(C);
        A = se3_mul(Ci, M);
        T = se3_mul(A, C);
    }
    const Q4<double> qi = qinv(T.q);
    Q4<double> gq;
    V3<double> gTt;
    qact_vjp(qi, T.t, -gt, gq, gTt);
    const Q4<double> gqi = qmat_vjp(qi, GR) + gq;
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

}  // namespace islam
