"""Tests only: NumPy float64 transcription of the reduced-arithmetic formulas of islam_amd/csrc/lie_dev.h -- skew_sq for the squared
skew matrix in so3_Jl_inv / so3_Jl, the vector form of se3_Q, the shared half-angle sincos of se3_exp -- and of the kernels built on
them.  tests/lie_f64.py keeps the matrix forms these replaced; tests/test_lie_fast_cpu.py holds the two against each other and this
file against the 50-digit reference of tests/golden/make_lie_golden.py.  What did not change (vectors, quaternions, so3_exp, so3_log,
align) is imported from tests/lie_f64.py.

`mutant(name)` switches one deliberate mistake on for the duration of a with-block."""
import contextlib

import numpy as np

from tests.lie_f64 import (_block_sums, align, cross, dot, mv, qact, qinv, qmat, qmul, se3_inv, se3_mul, skew, so3_log,  # noqa: F401
                           tmv)

MUTANTS = ('q_u_sign', 'q_c2_c1_swap', 'q_no_2sI', 'jl_sin2')
_on = set()


@contextlib.contextmanager
def mutant(name):
    assert name in MUTANTS, name
    _on.add(name)
    try:
        yield
    finally:
        _on.discard(name)


# ------------------------------------------------------------------ lie_dev.h
def outer(a, b):
    return a[..., :, None] * b[..., None, :]


def skew_sq(phi, th2):
    """[phi]x^2 = phi phi^T - th^2 I"""
    return outer(phi, phi) - th2[..., None, None] * np.eye(3)


def _half_sincos(th2, big):
    th = np.sqrt(np.where(big, th2, 1.0))
    return th, np.sin(0.5 * th), np.cos(0.5 * th)


def so3_exp_half(phi, th2, th, s, co):
    """so3_exp from the half-angle sincos the caller took (lie_f64.so3_exp: the same numbers)."""
    big = np.sqrt(th2) > 1e-2
    th4 = th2 * th2
    imag_s = 0.5 - th2 * (1.0 / 48.0) + th4 * (1.0 / 3840.0) - th4 * th2 * (1.0 / 645120.0)
    real_s = 1.0 - th2 * (1.0 / 8.0) + th4 * (1.0 / 384.0) - th4 * th2 * (1.0 / 46080.0)
    imag = np.where(big, s / th, imag_s)
    real = np.where(big, co, real_s)
    return np.concatenate([phi * imag[..., None], real[..., None]], -1)


def so3_exp(phi):
    th2 = dot(phi, phi)
    th, s, co = _half_sincos(th2, np.sqrt(th2) > 1e-2)
    return so3_exp_half(phi, th2, th, s, co)


def so3_Jl_inv(phi):
    th2 = dot(phi, phi)
    big = th2 > 1e-4
    th, s, co = _half_sincos(th2, big)
    c_c = (1.0 - th * co / (2.0 * s)) / np.where(big, th2, 1.0)
    c_s = 1.0 / 12.0 + th2 * (1.0 / 720.0) + th2 * th2 * (1.0 / 30240.0)
    c = np.where(big, c_c, c_s)[..., None, None]
    return np.eye(3) - 0.5 * skew(phi) + c * skew_sq(phi, th2)


def so3_Jl_half(phi, th2, th, s, co):
    """Jl(phi) = I + c1 K + c2 K^2 from the HALF-angle sincos: 1 - cos th = 2 sin^2(th/2), sin th = 2 sin(th/2) cos(th/2)."""
    big = th2 > 1e-4
    t2 = np.where(big, th2, 1.0)
    two = 1.0 if 'jl_sin2' in _on else 2.0
    c1 = np.where(big, two * s * s / t2, 0.5 - th2 * (1.0 / 24.0) + th2 * th2 * (1.0 / 720.0))
    c2 = np.where(big, (th - 2.0 * s * co) / (t2 * th), 1.0 / 6.0 - th2 * (1.0 / 120.0) + th2 * th2 * (1.0 / 5040.0))
    return np.eye(3) + c1[..., None, None] * skew(phi) + c2[..., None, None] * skew_sq(phi, th2)


def so3_Jl(phi):
    th2 = dot(phi, phi)
    th, s, co = _half_sincos(th2, th2 > 1e-4)
    return so3_Jl_half(phi, th2, th, s, co)


def se3_Q(rho, phi):
    """Q = 1/2 [rho]x + c1 (rho phi^T + phi rho^T - 2 s I) + (c2 - c1) s [phi]x + c2 (u phi^T - phi u^T) - 2 c3 s (phi phi^T - th^2 I),
    s = phi . rho, u = phi x rho; u phi^T - phi u^T = [phi x u]x, so the three skew terms are one skew matrix."""
    th2 = dot(phi, phi)
    big = th2 > 1e-2
    t2 = np.where(big, th2, 1.0)
    th = np.sqrt(t2)
    s_, co = np.sin(th), np.cos(th)
    th4 = t2 * t2
    c1, c2, c3 = (th - s_) / (t2 * th), (t2 + 2.0 * co - 2.0) / (2.0 * th4), (2.0 * th - 3.0 * s_ + th * co) / (2.0 * th4 * th)
    th4 = th2 * th2
    c1 = np.where(big, c1, 1.0 / 6.0 - th2 * (1.0 / 120.0) + th4 * (1.0 / 5040.0) - th4 * th2 * (1.0 / 362880.0)
                  + th4 * th4 * (1.0 / 39916800.0))
    c2 = np.where(big, c2, 1.0 / 24.0 - th2 * (1.0 / 720.0) + th4 * (1.0 / 40320.0) - th4 * th2 * (1.0 / 3628800.0)
                  + th4 * th4 * (1.0 / 479001600.0))
    c3 = np.where(big, c3, 1.0 / 120.0 - th2 * (1.0 / 2520.0) + th4 * (1.0 / 120960.0) - th4 * th2 * (1.0 / 9979200.0)
                  + th4 * th4 * (1.0 / 1245404160.0))
    s = dot(phi, rho)
    u = cross(phi, rho)
    a = ((c1 - c2) if 'q_c2_c1_swap' in _on else (c2 - c1)) * s
    pu = cross(phi, u)
    if 'q_u_sign' in _on:
        pu = -pu
    w = 0.5 * rho + a[..., None] * phi + c2[..., None] * pu
    d = 0.0 if 'q_no_2sI' in _on else -2.0 * (c1 * s)
    b = lambda c: c[..., None, None]
    sym = b(c1) * (outer(rho, phi) + outer(phi, rho)) + b(-2.0 * (c3 * s)) * skew_sq(phi, th2) + b(d + 0.0 * s) * np.eye(3)
    return sym + skew(w)


def se3_exp(rho, phi):
    """One sqrt and one half-angle sincos for the translation (so3_Jl) and the rotation (so3_exp); each keeps its threshold."""
    th2 = dot(phi, phi)
    th, s, co = _half_sincos(th2, (np.sqrt(th2) > 1e-2) | (th2 > 1e-4))
    return np.concatenate([mv(so3_Jl_half(phi, th2, th, s, co), rho), so3_exp_half(phi, th2, th, s, co)], -1)


def se3_log(X):
    """(rho, phi, Jl^-1(phi)): the callers that linearise reuse the third."""
    phi = so3_log(X[..., 3:])
    Ji = so3_Jl_inv(phi)
    return mv(Ji, X[..., :3]), phi, Ji


# ------------------------------------------------------------------ the kernels
def _vo_blocks(Xi, Xj, P):
    """vo_link: e = Log(P^-1 Xi^-1 Xj) and G, C of d e / d delta_j, Jl^-1(e) taken once."""
    pre = se3_mul(se3_inv(P), se3_inv(Xi))
    rho, phi, Ji = se3_log(se3_mul(pre, Xj))
    R = qmat(pre[..., 3:])
    G = Ji @ R
    C = Ji @ (skew(pre[..., :3]) @ R - se3_Q(rho, phi) @ G)
    return rho, phi, G, C


def _link_residuals(Xi, Xj, vi, vj, P, dR, dp, dv, dt):
    rho, phi, G, C = _vo_blocks(Xi, Xj, P)
    rv = dv - (vj - vi)
    rpre = qmul(qinv(dR), qinv(Xi[..., 3:]))
    er = so3_log(qmul(rpre, Xj[..., 3:]))
    rt = (Xj[..., :3] - Xi[..., :3]) - (dt[..., None] * vi + dp)
    return rho, phi, G, C, er, rpre, rv, rt


def linearize(nodes, vels, poses, drots, dtrans, dvels, dts):
    rho, phi, G, C, er, rpre, rv, rt = _link_residuals(nodes[:-1], nodes[1:], vels[:-1], vels[1:], poses, drots, dtrans, dvels, dts)
    B = so3_Jl_inv(er) @ qmat(rpre)
    M = len(poses)
    lin = np.concatenate([rho, phi, G.reshape(M, 9), C.reshape(M, 9), er, B.reshape(M, 9), rv, rt], 1).T
    sq = dot(rho, rho) + dot(phi, phi) + dot(rv, rv) + dot(er, er) + dot(rt, rt)
    return np.ascontiguousarray(lin), _block_sums(sq)


def linearize_edges(nodes, edges, poses):
    rho, phi, G, C = _vo_blocks(nodes[edges[:, 0]], nodes[edges[:, 1]], poses)
    E = len(poses)
    return np.ascontiguousarray(np.concatenate([rho, phi, G.reshape(E, 9), C.reshape(E, 9)], 1).T)


def retract(nodes, vels, dx, sign):
    X = se3_mul(se3_exp(sign * dx[:, :3], sign * dx[:, 3:6]), nodes)
    return X, vels + sign * dx[:, 6:]


def vo_loss_fwd(nodes, edges, poses):
    rho, phi, _ = se3_log(se3_mul(se3_mul(se3_inv(poses), se3_inv(nodes[edges[:, 0]])), nodes[edges[:, 1]]))
    return np.concatenate([rho, phi], 1), dot(rho, rho), dot(phi, phi)


def vo_loss_bwd(poses, err6, g_trans, g_rot):
    rho, phi = err6[:, :3], err6[:, 3:]
    gr, gp = (2.0 * g_trans)[:, None] * rho, (2.0 * g_rot)[:, None] * phi
    Ji, Q = so3_Jl_inv(phi), se3_Q(rho, phi)
    a = tmv(Ji, gr)
    b = tmv(Ji, gp) - tmv(Ji, tmv(Q, a))
    Pi = se3_inv(poses)
    R = qmat(Pi[:, 3:])
    o0 = tmv(R, a)
    o1 = tmv(R, tmv(skew(Pi[:, :3]), a)) + tmv(R, b)
    return np.concatenate([-o0, -o1, np.zeros((len(poses), 1))], 1)


def trial(nodes, vels, dx, poses, drots, dtrans, dvels, dts, lin):
    Xt, vt = retract(nodes, vels, dx, 1.0)
    rho, phi, _, _, er, _, rv, rt = _link_residuals(Xt[:-1], Xt[1:], vt[:-1], vt[1:], poses, drots, dtrans, dvels, dts)
    sq = dot(rho, rho) + dot(phi, phi) + dot(rv, rv) + dot(er, er) + dot(rt, rt)
    L = lin.T
    M = len(poses)
    G, C, B = L[:, 6:15].reshape(M, 3, 3), L[:, 15:24].reshape(M, 3, 3), L[:, 27:36].reshape(M, 3, 3)
    di, dj = dx[:-1], dx[1:]
    ddr, ddp = dj[:, :3] - di[:, :3], dj[:, 3:6] - di[:, 3:6]
    j0, j1, j2, j3, j4 = mv(G, ddr) + mv(C, ddp), mv(G, ddp), di[:, 6:] - dj[:, 6:], mv(B, ddp), ddr - dts[:, None] * di[:, 6:]
    R0, R1, R2, R3, R4 = L[:, 0:3], L[:, 3:6], L[:, 36:39], L[:, 24:27], L[:, 39:42]
    qd = dot(j0, 2.0 * R0 + j0) + dot(j1, 2.0 * R1 + j1) + dot(j2, 2.0 * R2 + j2) + dot(j3, 2.0 * R3 + j3) + dot(j4, 2.0 * R4 + j4)
    return Xt, vt, np.stack([_block_sums(sq), _block_sums(qd)], 1), np.stack([sq, qd], 1)


def transcription_outputs(z):
    """What make_lie_golden.case_errors wants (its transcription_outputs, from this module)."""
    from tests.golden.make_lie_golden import N_PARTIAL as n
    a = (z['nodes'], z['vels'], z['poses'], z['drots'], z['dtrans'], z['dvels'], z['dts'])
    lin, part = linearize(*a)
    err6, tl, rl = vo_loss_fwd(z['nodes'], z['edges'], z['edge_poses'])
    return dict(lin=lin, loss_part=part, retract_pos=retract(z['nodes'], z['vels'], z['dx'], 1.0),
                retract_neg=retract(z['nodes'][:n], z['vels'][:n], z['dx'][:n], -1.0),
                edge_lin=linearize_edges(z['nodes'], z['edges'], z['edge_poses']), vo_loss=(tl, rl),
                vo_grad=vo_loss_bwd(z['edge_poses'], err6, z['g_trans'], z['g_rot']),
                align=align(z['nodes'][:n], z['vels'][:n], z['align_target']),
                trial=trial(*a[:2], z['dx'], *a[2:], z['lin_ref'])[:3])
