// SO(3)/SE(3) device helpers for the gfx950 kernels (PVGO linearisation, retraction, losses).
//
// Conventions are the ones PyPose's LieTensor uses and the reference relies on
// (reference pvgo.py:36-51, Datasets/transformation.py:72-124): quaternion [x,y,z,w],
// SE3 = [t, q], tangent [rho, phi], left perturbation Exp(d)*X.
//
// Everything is register-resident: 3x3 matrices are nine named scalars in a struct that is only
// ever indexed with compile-time constants (runtime-indexed arrays would go to scratch memory).
// Small-angle branches switch to Taylor series below 1e-2 rad (se3_Q: below 0.1 rad, see there): PyPose
// switches only at machine eps, where its closed forms lose up to all digits to cancellation
// ((t^2+2cos t-2)/2t^4 ...); tests/test_lie_gpu.py holds every branch to a 50-digit reference.
//
// The unit is built without fast-math, so a product with a structural zero stays in the code.  Products of skew matrices are therefore
// never formed as 3x3 products: [a]x [b]x = b a^T - (a.b) I gives [phi]x^2 = phi phi^T - th^2 I (skew_sq) and the vector form of
// Barfoot's Q (derivation at se3_Q).  se3_log hands out the Jl^-1 it has to form anyway, and se3_exp takes one sqrt and one half-angle
// sincos for both of its parts.  tests/lie_f64_fast.py is the float64 transcription of these forms; tests/test_lie_fast_cpu.py holds
// them to the matrix forms they replaced (tests/lie_f64.py) and to the 50-digit reference.
#pragma once
#include <hip/hip_runtime.h>

namespace islam {

#define ISLAM_DEV __device__ __forceinline__

template <class T> struct V3 { T x, y, z; };
template <class T> struct Q4 { T x, y, z, w; };
template <class T> struct M3 { T a00, a01, a02, a10, a11, a12, a20, a21, a22; };
template <class T> struct SE3 { V3<T> t; Q4<T> q; };

template <class T> ISLAM_DEV V3<T> v3(T x, T y, T z) { return V3<T>{x, y, z}; }
template <class T> ISLAM_DEV V3<T> operator+(V3<T> a, V3<T> b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
template <class T> ISLAM_DEV V3<T> operator-(V3<T> a, V3<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <class T> ISLAM_DEV V3<T> operator-(V3<T> a) { return {-a.x, -a.y, -a.z}; }
template <class T> ISLAM_DEV V3<T> operator*(T s, V3<T> a) { return {s * a.x, s * a.y, s * a.z}; }
template <class T> ISLAM_DEV T dot(V3<T> a, V3<T> b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
template <class T> ISLAM_DEV V3<T> cross(V3<T> a, V3<T> b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

template <class T> ISLAM_DEV M3<T> m3_identity() { return {T(1), T(0), T(0), T(0), T(1), T(0), T(0), T(0), T(1)}; }
template <class T> ISLAM_DEV M3<T> skew(V3<T> v) { return {T(0), -v.z, v.y, v.z, T(0), -v.x, -v.y, v.x, T(0)}; }
// a b^T
template <class T> ISLAM_DEV M3<T> outer(V3<T> a, V3<T> b) {
    return {a.x * b.x, a.x * b.y, a.x * b.z, a.y * b.x, a.y * b.y, a.y * b.z, a.z * b.x, a.z * b.y, a.z * b.z};
}
// [phi]x^2 = phi phi^T - th^2 I, th2 = phi.phi (six products; the dense 3x3 product multiplies nine structural zeros)
template <class T> ISLAM_DEV M3<T> skew_sq(V3<T> phi, T th2) {
    const T xy = phi.x * phi.y, xz = phi.x * phi.z, yz = phi.y * phi.z;
    return {phi.x * phi.x - th2, xy, xz, xy, phi.y * phi.y - th2, yz, xz, yz, phi.z * phi.z - th2};
}
template <class T> ISLAM_DEV M3<T> operator+(M3<T> a, M3<T> b) {
    return {a.a00 + b.a00, a.a01 + b.a01, a.a02 + b.a02, a.a10 + b.a10, a.a11 + b.a11, a.a12 + b.a12,
            a.a20 + b.a20, a.a21 + b.a21, a.a22 + b.a22};
}
template <class T> ISLAM_DEV M3<T> operator-(M3<T> a, M3<T> b) {
    return {a.a00 - b.a00, a.a01 - b.a01, a.a02 - b.a02, a.a10 - b.a10, a.a11 - b.a11, a.a12 - b.a12,
            a.a20 - b.a20, a.a21 - b.a21, a.a22 - b.a22};
}
template <class T> ISLAM_DEV M3<T> operator*(T s, M3<T> a) {
    return {s * a.a00, s * a.a01, s * a.a02, s * a.a10, s * a.a11, s * a.a12, s * a.a20, s * a.a21, s * a.a22};
}
template <class T> ISLAM_DEV M3<T> operator*(M3<T> a, M3<T> b) {
    return {a.a00 * b.a00 + a.a01 * b.a10 + a.a02 * b.a20, a.a00 * b.a01 + a.a01 * b.a11 + a.a02 * b.a21,
            a.a00 * b.a02 + a.a01 * b.a12 + a.a02 * b.a22,
            a.a10 * b.a00 + a.a11 * b.a10 + a.a12 * b.a20, a.a10 * b.a01 + a.a11 * b.a11 + a.a12 * b.a21,
            a.a10 * b.a02 + a.a11 * b.a12 + a.a12 * b.a22,
            a.a20 * b.a00 + a.a21 * b.a10 + a.a22 * b.a20, a.a20 * b.a01 + a.a21 * b.a11 + a.a22 * b.a21,
            a.a20 * b.a02 + a.a21 * b.a12 + a.a22 * b.a22};
}
template <class T> ISLAM_DEV M3<T> transpose(M3<T> a) {
    return {a.a00, a.a10, a.a20, a.a01, a.a11, a.a21, a.a02, a.a12, a.a22};
}
template <class T> ISLAM_DEV V3<T> operator*(M3<T> a, V3<T> v) {
    return {a.a00 * v.x + a.a01 * v.y + a.a02 * v.z, a.a10 * v.x + a.a11 * v.y + a.a12 * v.z,
            a.a20 * v.x + a.a21 * v.y + a.a22 * v.z};
}
// a^T v
template <class T> ISLAM_DEV V3<T> tmul(M3<T> a, V3<T> v) {
    return {a.a00 * v.x + a.a10 * v.y + a.a20 * v.z, a.a01 * v.x + a.a11 * v.y + a.a21 * v.z,
            a.a02 * v.x + a.a12 * v.y + a.a22 * v.z};
}
template <class T> ISLAM_DEV void m3_store(M3<T> a, T* p) {
    p[0] = a.a00; p[1] = a.a01; p[2] = a.a02; p[3] = a.a10; p[4] = a.a11; p[5] = a.a12;
    p[6] = a.a20; p[7] = a.a21; p[8] = a.a22;
}
template <class T> ISLAM_DEV M3<T> m3_load(const T* p) { return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8]}; }

// ------------------------------------------------------------------ quaternions
template <class T> ISLAM_DEV Q4<T> qmul(Q4<T> a, Q4<T> b) {
    return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
            a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
template <class T> ISLAM_DEV Q4<T> qinv(Q4<T> q) { return {-q.x, -q.y, -q.z, q.w}; }
template <class T> ISLAM_DEV V3<T> qact(Q4<T> q, V3<T> p) {
    V3<T> u{q.x, q.y, q.z};
    V3<T> uv = T(2) * cross(u, p);
    return p + q.w * uv + cross(u, uv);
}
template <class T> ISLAM_DEV M3<T> qmat(Q4<T> q) {
    T x = q.x, y = q.y, z = q.z, w = q.w;
    return {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
}

// Exp(phi) from th2 = phi.phi, th = sqrt(th2) and the HALF-angle sincos (s, co) = sincos(th / 2); s and co are read only where th > 1e-2
template <class T> ISLAM_DEV Q4<T> so3_exp_half(V3<T> phi, T th2, T th, T s, T co) {
    T imag, real;
    if (th > T(1e-2)) {
        imag = s / th;
        real = co;
    } else {
        T th4 = th2 * th2;
        imag = T(0.5) - th2 * T(1.0 / 48.0) + th4 * T(1.0 / 3840.0) - th4 * th2 * T(1.0 / 645120.0);
        real = T(1.0) - th2 * T(1.0 / 8.0) + th4 * T(1.0 / 384.0) - th4 * th2 * T(1.0 / 46080.0);
    }
    return {phi.x * imag, phi.y * imag, phi.z * imag, real};
}
template <class T> ISLAM_DEV Q4<T> so3_exp(V3<T> phi) {
    T th2 = dot(phi, phi);
    T th = sqrt(th2);
    T s = T(0), co = T(1);
    if (th > T(1e-2)) sincos(T(0.5) * th, &s, &co);
    return so3_exp_half(phi, th2, th, s, co);
}

template <class T> ISLAM_DEV V3<T> so3_log(Q4<T> q) {
    V3<T> v{q.x, q.y, q.z};
    T vn2 = dot(v, v);
    T vn = sqrt(vn2);
    T f;
    if (vn > T(1e-3)) {
        f = T(2) * atan(vn / q.w) / vn;          // atan (not atan2), as PyPose SO3_Log
    } else {
        T w2 = q.w * q.w;                          // 2*atan(x)/vn, x = vn/w:  2/w (1 - x^2/3 + x^4/5)
        T x2 = vn2 / w2;
        f = (T(2) / q.w) * (T(1) - x2 * T(1.0 / 3.0) + x2 * x2 * T(0.2));
    }
    return f * v;
}

// I + a K + c K^2 with K = [phi]x, K^2 = skew_sq: the three terms entry by entry, no product with a zero of K or I
template <class T> ISLAM_DEV M3<T> so3_poly(V3<T> phi, T th2, T a, T c) {
    const M3<T> S = skew_sq(phi, th2);
    const V3<T> k = a * phi;
    return {T(1) + c * S.a00, c * S.a01 - k.z, c * S.a02 + k.y,
            c * S.a10 + k.z, T(1) + c * S.a11, c * S.a12 - k.x,
            c * S.a20 - k.y, c * S.a21 + k.x, T(1) + c * S.a22};
}

// Jl^-1(phi) = I - K/2 + c K^2
template <class T> ISLAM_DEV M3<T> so3_Jl_inv(V3<T> phi) {
    T th2 = dot(phi, phi);
    T c;
    if (th2 > T(1e-4)) {
        T th = sqrt(th2);
        T s, co;
        sincos(T(0.5) * th, &s, &co);
        c = (T(1) - th * co / (T(2) * s)) / th2;
    } else {
        c = T(1.0 / 12.0) + th2 * T(1.0 / 720.0) + th2 * th2 * T(1.0 / 30240.0);
    }
    return so3_poly(phi, th2, T(-0.5), c);
}

// Jl(phi) = I + c1 K + c2 K^2 from th2, th and the HALF-angle sincos (read only where th2 > 1e-4):
// 1 - cos th = 2 sin^2(th/2) (no cancellation, unlike 1 - cos th) and sin th = 2 sin(th/2) cos(th/2)
template <class T> ISLAM_DEV M3<T> so3_Jl_half(V3<T> phi, T th2, T th, T s, T co) {
    T c1, c2;
    if (th2 > T(1e-4)) {
        c1 = T(2) * s * s / th2;
        c2 = (th - T(2) * s * co) / (th2 * th);
    } else {
        c1 = T(0.5) - th2 * T(1.0 / 24.0) + th2 * th2 * T(1.0 / 720.0);
        c2 = T(1.0 / 6.0) - th2 * T(1.0 / 120.0) + th2 * th2 * T(1.0 / 5040.0);
    }
    return so3_poly(phi, th2, c1, c2);
}
template <class T> ISLAM_DEV M3<T> so3_Jl(V3<T> phi) {
    T th2 = dot(phi, phi);
    T th = sqrt(th2);
    T s = T(0), co = T(1);
    if (th2 > T(1e-4)) sincos(T(0.5) * th, &s, &co);
    return so3_Jl_half(phi, th2, th, s, co);
}

// Barfoot's Q(rho, phi) (PyPose calcQ).  Its closed forms cancel harder than the others: th^2 + 2cos th - 2 keeps th^4/12 of
// terms of size th^2, so at th = 1e-2 c2 has 1e-8 left and Q (times rho) is off by ~1e-12 -- 600 rounding floors, measured
// against a 50-digit reference (tests/golden/make_lie_golden.py).  Hence the series up to th = 0.1, two more terms each;
// there the closed forms are good to ~4e-14 |rho|.
//
// The matrix part.  With T = [rho]x, P = [phi]x:  Q = T/2 + c1 (PT + TP + PTP) + c2 (P.PT + TP.P - 3 PTP) + c3 (PTP.P + P.PTP),
// seven dense products of matrices that are two thirds zeros.  With [a]x [b]x = b a^T - (a.b) I, phi^T [phi]x = 0, s = phi.rho and
// u = phi x rho ([phi]x rho = u, rho^T [phi]x = u^T):
//   PT = rho phi^T - s I,  TP = phi rho^T - s I                     PT + TP = rho phi^T + phi rho^T - 2 s I
//   PTP = (rho phi^T - s I) P = -s P
//   P.PT = u phi^T - s P,  TP.P = -phi u^T - s P                     P.PT + TP.P = u phi^T - phi u^T - 2 s P
//   PTP.P + P.PTP = -2 s P^2                                        = -2 s (phi phi^T - th^2 I)
// so  Q = T/2 + c1 (rho phi^T + phi rho^T - 2 s I) + (c2 - c1) s P + c2 (u phi^T - phi u^T) - 2 c3 s (phi phi^T - th^2 I).
// u phi^T - phi u^T is the skew matrix of phi x u (entry by entry the same products), so T/2, P and it are ONE skew matrix [w]x,
// w = rho/2 + (c2 - c1) s phi + c2 (phi x u); the rest is symmetric.
template <class T> ISLAM_DEV M3<T> se3_Q(V3<T> rho, V3<T> phi) {
    T th2 = dot(phi, phi);
    T c1, c2, c3;
    if (th2 > T(1e-2)) {
        T th = sqrt(th2);
        T s, co;
        sincos(th, &s, &co);
        T th4 = th2 * th2;
        c1 = (th - s) / (th2 * th);
        c2 = (th2 + T(2) * co - T(2)) / (T(2) * th4);
        c3 = (T(2) * th - T(3) * s + th * co) / (T(2) * th4 * th);
    } else {
        T th4 = th2 * th2;
        c1 = T(1.0 / 6.0) - th2 * T(1.0 / 120.0) + th4 * T(1.0 / 5040.0) - th4 * th2 * T(1.0 / 362880.0) +
             th4 * th4 * T(1.0 / 39916800.0);
        c2 = T(1.0 / 24.0) - th2 * T(1.0 / 720.0) + th4 * T(1.0 / 40320.0) - th4 * th2 * T(1.0 / 3628800.0) +
             th4 * th4 * T(1.0 / 479001600.0);
        c3 = T(1.0 / 120.0) - th2 * T(1.0 / 2520.0) + th4 * T(1.0 / 120960.0) - th4 * th2 * T(1.0 / 9979200.0) +
             th4 * th4 * T(1.0 / 1245404160.0);
    }
    const T sp = dot(phi, rho);
    const V3<T> u = cross(phi, rho);
    const V3<T> w = T(0.5) * rho + ((c2 - c1) * sp) * phi + c2 * cross(phi, u);
    const M3<T> S = skew_sq(phi, th2);
    const T b = T(-2) * (c3 * sp), d = T(-2) * (c1 * sp);
    const T m01 = c1 * (rho.x * phi.y + phi.x * rho.y) + b * S.a01;
    const T m02 = c1 * (rho.x * phi.z + phi.x * rho.z) + b * S.a02;
    const T m12 = c1 * (rho.y * phi.z + phi.y * rho.z) + b * S.a12;
    return {c1 * (T(2) * (rho.x * phi.x)) + b * S.a00 + d, m01 - w.z, m02 + w.y,
            m01 + w.z, c1 * (T(2) * (rho.y * phi.y)) + b * S.a11 + d, m12 - w.x,
            m02 - w.y, m12 + w.x, c1 * (T(2) * (rho.z * phi.z)) + b * S.a22 + d};
}

// ------------------------------------------------------------------ SE3
template <class T> ISLAM_DEV SE3<T> se3_load(const T* p) { return {{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}}; }
template <class T> ISLAM_DEV void se3_store(SE3<T> X, T* p) {
    p[0] = X.t.x; p[1] = X.t.y; p[2] = X.t.z; p[3] = X.q.x; p[4] = X.q.y; p[5] = X.q.z; p[6] = X.q.w;
}
template <class T> ISLAM_DEV SE3<T> se3_mul(SE3<T> X, SE3<T> Y) { return {X.t + qact(X.q, Y.t), qmul(X.q, Y.q)}; }
template <class T> ISLAM_DEV SE3<T> se3_inv(SE3<T> X) {
    Q4<T> qi = qinv(X.q);
    return {-qact(qi, X.t), qi};
}
// Exp([rho, phi]) = [Jl(phi) rho, Exp(phi)]: one sqrt and one half-angle sincos serve both parts; each keeps its own threshold
template <class T> ISLAM_DEV SE3<T> se3_exp(V3<T> rho, V3<T> phi) {
    T th2 = dot(phi, phi);
    T th = sqrt(th2);
    T s = T(0), co = T(1);
    if (th > T(1e-2) || th2 > T(1e-4)) sincos(T(0.5) * th, &s, &co);
    return {so3_Jl_half(phi, th2, th, s, co) * rho, so3_exp_half(phi, th2, th, s, co)};
}
// Log(X) = [Jl^-1(phi) t, phi]; Ji = Jl^-1(phi) is what the Jacobian of the logarithm starts from, so the callers that linearise take it
template <class T> ISLAM_DEV void se3_log(SE3<T> X, V3<T>& rho, V3<T>& phi, M3<T>& Ji) {
    phi = so3_log(X.q);
    Ji = so3_Jl_inv(phi);
    rho = Ji * X.t;
}
template <class T> ISLAM_DEV void se3_log(SE3<T> X, V3<T>& rho, V3<T>& phi) {
    M3<T> Ji;
    se3_log(X, rho, phi, Ji);
}

}  // namespace islam
