"""The float64 numpy restatement of the dense reprojection family (include/islam_hip.h, "dense reprojection"; DESIGN.md sections 3.23 -
3.25), a helper module beside imu_f64.py and lie_f64.py and not a test file.  One per-pixel front (link_front: mount, T^-1, ray, Q,
validity clauses, residual, robust kernel, dr/dQ and the rows of J_cam) under the three restatements built on it -- the pose-only sums
(reproj_reference_link), the gradient of w^T g in depth and flow (vjp_reference_link) and the per-pixel Schur sums of the joint problem
(ba_reference_link) -- their two Levenberg-Marquardt loops, the seeded scenes, and what the GPU test files share.  The CPU test files
check this module against central differences and explicitly assembled systems; the GPU test files hold the kernels to it."""
import functools
import math

import numpy as np
import torch

from islam_amd import robust
from islam_amd._lib import DENSE_REPROJ_BADPRIOR as BADPRIOR
from islam_amd._lib import DENSE_REPROJ_FEW as FEW
from islam_amd._lib import DENSE_REPROJ_NOTPD as NOTPD
from islam_amd._lib import DENSE_REPROJ_NSUM as NSUM
from islam_amd._lib import DENSE_REPROJ_OK as OK
from oracle import lie

S_G, S_COST, S_L1, S_COUNT = 21, 27, 28, 29
TRIU = np.triu_indices(6)
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12          # ISLAM_DENSE_REPROJ_LAMBDA_MIN / _MAX
MOUNT = np.concatenate([[0.1, -0.05, 0.2], lie.so3_exp(np.array([0.3, -0.2, 0.4]))])
U = 2.0 ** -52
# Roundings in one term of a camera-frame sum of the joint problem, counted from dense_ba_partial_kernel's arithmetic (DESIGN.md section
# 3.25).  The kernel forms a pixel's term as J^T M J with the 2x2 M = c I - e e^T / h_dd, e = c jd (J^T (c r - e g_d / h_dd) on the
# right-hand side), so it has section 3.23's 64 for everything up to c, r and J_cam and the product with J, and on top 1/rho (1), R ray
# (10), -1/rho^2 (2), jd (8), e (2), h_dd (4), g_d with rho0 and rho - rho0 (7), 1/h_dd (1), e / h_dd (2), the entries of M or of
# c r - e g_d / h_dd (4 each), and M J in place of c J (3 more per entry): 48 more, 112, rounded up.
K_ROUND = 128


# ------------------------------------------------------------------------------------------------ sums
def _fsum_cols(t):
    return np.array([math.fsum(t[:, k]) for k in range(t.shape[1])]) if t.shape[0] else np.zeros(t.shape[1])


def _seq_cols(t):
    return np.cumsum(t, axis=0)[-1] if t.shape[0] else np.zeros(t.shape[1])        # cumsum adds in index order


def body_from_sums(sums, A):
    """(H, g) in the body frame from the 30 camera-frame sums: H = A^T H_cam A, g = A^T g_cam."""
    Hc = np.zeros((6, 6))
    Hc[TRIU] = sums[:21]
    Hc = Hc + np.triu(Hc, 1).T
    return A.T @ Hc @ A, A.T @ sums[S_G:S_G + 6]


# ------------------------------------------------------------------------------------------------ the per-pixel front
def link_front(z, flow, keep, motion, rgb2imu, intr, kernel=None):
    """Everything of one link ahead of the sums, pixel by pixel from the header's definitions, float64, over the whole image.  z (H,W):
    the depth along the ray; flow (2,H,W); keep (H,W) bool: the pixels the caller admits (the user mask, and for the joint problem a
    usable inverse depth); motion (7); rgb2imu (7) or None; intr (4); kernel None / robust.Huber / robust.Cauchy.  Returns a dict:
    A = Ad(C^-1), u, v, ray, dQ = R ray (= dQ/dz), valid = keep and the three clauses, margin ((n,3) over the kept pixels: the margin of
    each clause relative to its threshold, NaN where an earlier clause already dropped the pixel), rejects (3: how many kept pixels
    each clause drops), Qx, Qy, Qz (Qz = 1 at an invalid pixel, whose further entries mean nothing), fl, ru, rv, s, rob = rho(s),
    c = rho'(s), cp = dc/ds, dr/dQ = [[a, 0, bq], [0, cq, dq]], and ju, jv (H,W,6): the rows of dr/dQ [-I, [Q]x]."""
    Hh, Ww = z.shape
    fx, fy, cx, cy = (float(x) for x in intr)
    M = np.asarray(motion, np.float64)
    if rgb2imu is None:
        T, A = M, np.eye(6)
    else:
        C = np.asarray(rgb2imu, np.float64)
        T = lie.se3_mul(lie.se3_mul(lie.se3_inv(C), M), C)
        A = lie.se3_adj(lie.se3_inv(C))
    Ti = lie.se3_inv(T)
    R, t = lie.quat_matrix(Ti[3:]), Ti[:3]
    v, u = np.meshgrid(np.arange(Hh, dtype=np.float64), np.arange(Ww, dtype=np.float64), indexing='ij')
    xh, yh = (u - cx) / fx, (v - cy) / fy
    ray = np.stack([xh, yh, np.ones_like(xh)], -1)
    P = np.stack([z * xh, z * yh, z], -1)
    Q = P @ R.T + t
    dQ = ray @ R.T
    with np.errstate(divide='ignore', invalid='ignore'):
        px, py = Q[..., 0] / Q[..., 2], Q[..., 1] / Q[..., 2]
    c1 = Q[..., 2] > 0.1
    c2 = np.abs(px) <= 1.0
    c3 = np.abs(py) <= 1.0
    valid = keep & c1 & c2 & c3
    margin = np.stack([np.abs(Q[..., 2] - 0.1) / 0.1, np.where(c1, np.abs(1.0 - np.abs(px)), np.nan),
                       np.where(c1, np.abs(1.0 - np.abs(py)), np.nan)], -1)[keep]
    rejects = np.array([(keep & ~c1).sum(), (keep & c1 & ~c2).sum(), (keep & c1 & ~c3).sum()])
    fl = np.asarray(flow, np.float64)
    Qx, Qy = Q[..., 0], Q[..., 1]
    Qz = np.where(valid, Q[..., 2], 1.0)
    with np.errstate(all='ignore'):          # an invalid pixel may hold anything
        ru = fx * (Qx / Qz) + cx - (fl[0] + u)
        rv = fy * (Qy / Qz) + cy - (fl[1] + v)
        s = ru * ru + rv * rv
        cp = np.zeros_like(s)
        if kernel is None:
            rob, c = s, np.ones_like(s)
        else:
            rob, c = kernel.rho(s), kernel.weight(s)
            if isinstance(kernel, robust.Huber):
                d = kernel.delta
                out = s > d * d
                cp[out] = -d / (2.0 * s[out] ** 1.5)
            elif isinstance(kernel, robust.Cauchy):
                d2 = kernel.delta ** 2
                cp = -1.0 / (d2 * (1.0 + s / d2) ** 2)
            else:
                raise ValueError(kernel)
        a, bq, cq, dq = fx / Qz, -fx * Qx / Qz ** 2, fy / Qz, -fy * Qy / Qz ** 2
        zero = np.zeros_like(a)
        ju = np.stack([-a, zero, -bq, -bq * Qy, bq * Qx - a * Qz, a * Qy], -1)          # rows of dr/dQ [-I, [Q]x]
        jv = np.stack([zero, -cq, -dq, cq * Qz - dq * Qy, dq * Qx, -cq * Qx], -1)
    return dict(A=A, u=u, v=v, ray=ray, dQ=dQ, valid=valid, margin=margin, rejects=rejects, Qx=Qx, Qy=Qy, Qz=Qz, fl=fl, ru=ru, rv=rv, s=s,
                rob=rob, c=c, cp=cp, a=a, bq=bq, cq=cq, dq=dq, ju=ju, jv=jv, fx=fx, fy=fy, cx=cx, cy=cy)


def _user(mask, shape):
    return np.ones(shape, bool) if mask is None else np.asarray(mask) != 0


# ------------------------------------------------------------------------------------------------ section 3.23: the pose-only sums
def reproj_reference_link(depth, flow, mask, motion, rgb2imu, intr, kernel=None):
    """One link, pixel by pixel from the header's definitions, float64.  depth (H,W), flow (2,H,W), mask (H,W) or None, motion (7),
    rgb2imu (7) or None, intr (4).  Returns a dict: sums (30, camera frame, each the correctly rounded sum of its terms), abs
    (30, sum |term|), fwd / bwd (30, the terms added in pixel order and in reverse), H, g (body frame, from sums), Habs, gabs (abs
    pushed through |A|), cost, l1, count, A, valid (H,W) and, for every pixel the user mask keeps, the margin of each clause
    relative to its threshold (margin, (n,3); NaN where an earlier clause already dropped the pixel) and rejects (3): how many
    pixels each clause drops."""
    f = link_front(np.asarray(depth, np.float64), flow, _user(mask, depth.shape), motion, rgb2imu, intr, kernel)
    A, valid = f['A'], f['valid']
    ru, rv, rho, c, ju, jv = (f[k][valid] for k in ('ru', 'rv', 'rob', 'c', 'ju', 'jv'))
    terms = np.zeros((ru.shape[0], NSUM))
    terms[:, :21] = (c[:, None, None] * (ju[:, :, None] * ju[:, None, :] + jv[:, :, None] * jv[:, None, :]))[:, TRIU[0], TRIU[1]]
    terms[:, S_G:S_G + 6] = c[:, None] * (ju * ru[:, None] + jv * rv[:, None])
    terms[:, S_COST] = rho
    terms[:, S_L1] = np.abs(ru) + np.abs(rv)
    terms[:, S_COUNT] = 1.0
    # sum |term|: for H and g the two products of a term are taken separately (the kernel adds them one after the other)
    absterms = terms.copy()
    absterms[:, :21] = (c[:, None, None] * (np.abs(ju[:, :, None] * ju[:, None, :]) + np.abs(jv[:, :, None] * jv[:, None, :])))[:, TRIU[0], TRIU[1]]
    absterms[:, S_G:S_G + 6] = c[:, None] * (np.abs(ju * ru[:, None]) + np.abs(jv * rv[:, None]))
    sums, ab = _fsum_cols(terms), _fsum_cols(np.abs(absterms))
    H, g = body_from_sums(sums, A)
    Habs, gabs = body_from_sums(ab, np.abs(A))
    return dict(sums=sums, abs=ab, fwd=_seq_cols(terms), bwd=_seq_cols(terms[::-1]), H=H, g=g, Habs=Habs, gabs=gabs, cost=sums[S_COST],
                l1=sums[S_L1], count=int(ru.shape[0]), A=A, valid=valid, margin=f['margin'], rejects=f['rejects'])


def reproj_reference(depth, flow, mask, motion, rgb2imu, intr, kernel=None):
    """reproj_reference_link for every link of a batch: a list of dicts."""
    B = depth.shape[0]
    intr = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (B, 4))
    return [reproj_reference_link(depth[b], flow[b], None if mask is None else mask[b], motion[b], rgb2imu, intr[b], kernel) for b in range(B)]


def right_perturb(motion, xi):
    """motion Exp(xi), quaternion normalised."""
    X = lie.se3_mul(np.asarray(motion, np.float64), lie.se3_exp(np.asarray(xi, np.float64)))
    X[..., 3:] /= np.linalg.norm(X[..., 3:], axis=-1, keepdims=True)
    return X


def refine_reference_link(depth, flow, mask, motion, rgb2imu, intr, kernel=None, iters=10, damping=1e-4, min_count=16, order='sums'):
    """The LM of islam_dense_reproj_refine for one link, same accept rule and schedule; ``order`` picks which of the restatement's
    sums drives it ('sums', 'fwd' or 'bwd').  Returns dict(motion, status, accepted, rejected, damping, last_step, trace)."""
    def evaluate(X):
        r = reproj_reference_link(depth, flow, mask, X, rgb2imu, intr, kernel)
        H, g = body_from_sums(r[order], r['A'])
        return dict(H=H, g=g, cost=r[order][S_COST], count=r['count'], finite=bool(np.isfinite(r[order]).all()))

    cur = np.asarray(motion, np.float64).copy()
    st = evaluate(cur)
    out = dict(motion=cur, status=OK, accepted=0, rejected=0, damping=float(damping), last_step=float('nan'),
               trace=[st['cost'] / st['count'] if st['count'] else float('nan')])
    if not (st['finite'] and st['count'] >= min_count):
        out['status'] = FEW
        return out
    for _ in range(1, iters):
        Hd = st['H'] + out['damping'] * np.diag(np.diag(st['H']))
        try:
            L = np.linalg.cholesky(Hd)
        except np.linalg.LinAlgError:
            out['status'], out['motion'] = NOTPD, cur
            return out
        delta = np.linalg.solve(L.T, np.linalg.solve(L, -st['g']))
        out['last_step'] = float(np.linalg.norm(delta))
        trial = right_perturb(cur, delta)
        tr = evaluate(trial)
        out['trace'].append(tr['cost'] / tr['count'] if tr['count'] else float('nan'))
        if tr['finite'] and tr['count'] >= min_count and tr['cost'] / tr['count'] < st['cost'] / st['count']:
            cur, st = trial, tr
            out['damping'] = max(out['damping'] / 10.0, LAMBDA_MIN)
            out['accepted'] += 1
        else:
            out['damping'] = min(out['damping'] * 10.0, LAMBDA_MAX)
            out['rejected'] += 1
    out['motion'] = cur
    return out


# ------------------------------------------------------------------------------------------------ section 3.24: the gradient in depth and flow
def _vjp_terms(a, bq, cq, dq, Qx, Qy, Qz, iz, dQx, dQy, dQz, wr, wf, c, cp, ru, rv, neg):
    """The header's formulas from their leaves.  neg = -1: the values.  neg = +1 on the magnitudes of the leaves: every product the
    values are summed from, taken positive (sum |term|).  Returns (e.(Jq dQ), c r.[dJq m + Jq (dQ x w_phi)], dPhi/dflow_u, _v)."""
    m0 = neg * wr[0] + Qy * wf[2] + neg * Qz * wf[1]          # m = -w_rho + Q x w_phi
    m1 = neg * wr[1] + Qz * wf[0] + neg * Qx * wf[2]
    m2 = neg * wr[2] + Qx * wf[1] + neg * Qy * wf[0]
    qu, qv = a * m0 + bq * m2, cq * m1 + dq * m2              # q = Jq m
    k2 = 2.0 * cp * (qu * ru + qv * rv)
    eu, ev = c * qu + k2 * ru, c * qv + k2 * rv               # e = c q + 2 c' (q.r) r
    da, dcq = neg * (a * iz) * dQz, neg * (cq * iz) * dQz     # the differential of a, bq, cq, dq along dQ
    dbq = neg * (a * iz) * dQx + neg * 2.0 * (bq * iz) * dQz
    ddq = neg * (cq * iz) * dQy + neg * 2.0 * (dq * iz) * dQz
    n0 = dQy * wf[2] + neg * dQz * wf[1]                      # dQ x w_phi
    n1 = dQz * wf[0] + neg * dQx * wf[2]
    n2 = dQx * wf[1] + neg * dQy * wf[0]
    tu = da * m0 + dbq * m2 + a * n0 + bq * n2
    tv = dcq * m1 + ddq * m2 + cq * n1 + dq * n2
    return eu * (a * dQx + bq * dQz) + ev * (cq * dQy + dq * dQz), c * (ru * tu + rv * tv), neg * eu, neg * ev


def vjp_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, kernel=None):
    """d(w^T g)/d(depth, flow) of one link at a fixed pose and valid set, pixel by pixel from the header's formulas, float64; the
    arguments of reproj_reference_link and w (6, body frame).  Returns a dict: grad_depth (H,W), grad_flow (2,H,W) (0 where
    invalid), depth_dJ (H,W): the part of grad_depth that comes from dq/dz (the "dJ/dz term"), abs_depth, abs_flow: per element the
    sum of |term| over the products the value is summed from (a, bq, cq, dq, Q, dQ, w_cam, c and c' are leaves; r, a difference
    of numbers of the size of the image, enters with |fx p| + |cx| + |flow| + |u|), valid (H,W) and s (H,W; NaN where invalid)."""
    Hh, Ww = depth.shape
    f = link_front(np.asarray(depth, np.float64), flow, _user(mask, depth.shape), motion, rgb2imu, intr, kernel)
    valid = f['valid']
    wc = f['A'] @ np.asarray(w, np.float64)
    a, bq, cq, dq, Qx, Qy, Qz, c, cp, ru, rv, s = (f[k][valid] for k in ('a', 'bq', 'cq', 'dq', 'Qx', 'Qy', 'Qz', 'c', 'cp', 'ru', 'rv', 's'))
    dQx, dQy, dQz = (f['dQ'][..., k][valid] for k in range(3))
    rua = np.abs(f['fx'] * (Qx / Qz)) + abs(f['cx']) + np.abs(f['fl'][0][valid]) + f['u'][valid]
    rva = np.abs(f['fy'] * (Qy / Qz)) + abs(f['cy']) + np.abs(f['fl'][1][valid]) + f['v'][valid]
    val = _vjp_terms(a, bq, cq, dq, Qx, Qy, Qz, 1.0 / Qz, dQx, dQy, dQz, wc[:3], wc[3:], c, cp, ru, rv, -1.0)
    mag = _vjp_terms(*(np.abs(x) for x in (a, bq, cq, dq, Qx, Qy, Qz, 1.0 / Qz, dQx, dQy, dQz, wc[:3], wc[3:], c, cp)), rua, rva, 1.0)

    def image(x):
        full = np.zeros((Hh, Ww))
        full[valid] = x
        return full

    smap = np.full((Hh, Ww), np.nan)
    smap[valid] = s
    return dict(grad_depth=image(val[0] + val[1]), grad_flow=np.stack([image(val[2]), image(val[3])]), depth_dJ=image(val[1]),
                abs_depth=image(mag[0] + mag[1]), abs_flow=np.stack([image(mag[2]), image(mag[3])]), valid=valid, s=smap)


def tangent_from_pose_grad(motion, grad7):
    """v = dL/dxi on motion Exp(xi) from grad7 = dL/d[t, q xyzw]: v_rho = R^T dL/dt, v_phi = 1/2 E^T dL/dq with E = d(q (x, 1))/dx at
    0 = [[q_w I + [q_v]x], [-q_v^T]]."""
    motion, grad7 = np.asarray(motion, np.float64), np.asarray(grad7, np.float64)
    qv, qw = motion[3:6], motion[6]
    return np.concatenate([lie.quat_matrix(motion[3:]).T @ grad7[:3], 0.5 * (qw * grad7[3:6] - np.cross(qv, grad7[3:6]) - grad7[6] * qv)])


def ift_weights_reference(H, motion, grad7):
    """w = -H^-1 v."""
    return -np.linalg.solve(np.asarray(H, np.float64), tangent_from_pose_grad(motion, grad7))


# ------------------------------------------------------------------------------------------------ section 3.25: the joint problem
def ba_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho=None, kernel=None):
    """One link of the joint problem at (motion, rho), pixel by pixel from the header's definitions, float64.  depth (H,W), flow
    (2,H,W), mask (H,W) or None, motion (7), rgb2imu (7) or None, intr (4), w > 0, rho (H,W) or None (the prior 1/depth).  Returns a
    dict: sums (30, camera frame, each the correctly rounded sum of its terms), abs (30: per sum, the sum over the pixels of the
    magnitudes of the term's two parts, |c J^T J| + |h_pd h_pd^T / h_dd|), fwd / bwd (the terms added in pixel order and in
    reverse), S, g (body frame), Sabs, gabs (abs pushed through |A|), cost, l1, count, A; per pixel of the whole image (c = 0 at an
    invalid one) hpd (H,W,6, camera frame), hdd, gd, and valid, prior (the depth gives a prior), rho0, rho; Hpp / gp: the body-frame
    pose block sum c J^T J and sum c J^T r before the depths are eliminated; margin / rejects as reproj_reference_link."""
    z = np.asarray(depth, np.float64)
    prior = np.isfinite(z) & (z > 0)
    rho0 = np.where(prior, 1.0 / np.where(prior, z, 1.0), 0.0)
    rho = rho0.copy() if rho is None else np.asarray(rho, np.float64)
    usable = prior & np.isfinite(rho) & (rho > 0)
    rs = np.where(usable, rho, 1.0)
    f = link_front(1.0 / rs, flow, _user(mask, depth.shape) & usable, motion, rgb2imu, intr, kernel)
    A, valid, ru, rv, rob, ju, jv, dR = (f[k] for k in ('A', 'valid', 'ru', 'rv', 'rob', 'ju', 'jv', 'dQ'))
    c = np.where(valid, f['c'], 0.0)
    k = -1.0 / (rs * rs)
    jdu = (f['a'] * dR[..., 0] + f['bq'] * dR[..., 2]) * k
    jdv = (f['cq'] * dR[..., 1] + f['dq'] * dR[..., 2]) * k
    hpd = c[..., None] * (ju * jdu[..., None] + jv * jdv[..., None])
    dprior = rho - rho0
    hdd = c * (jdu * jdu + jdv * jdv) + w
    gd = c * (jdu * ru + jdv * rv) + w * dprior

    sel = valid
    cs, jus, jvs, hs, hds, gds = c[sel], ju[sel], jv[sel], hpd[sel], hdd[sel], gd[sel]
    n = int(sel.sum())
    first = np.zeros((n, NSUM))
    second = np.zeros((n, NSUM))
    first[:, :21] = (cs[:, None, None] * (jus[:, :, None] * jus[:, None, :] + jvs[:, :, None] * jvs[:, None, :]))[:, TRIU[0], TRIU[1]]
    second[:, :21] = (hs[:, :, None] * hs[:, None, :] / hds[:, None, None])[:, TRIU[0], TRIU[1]]
    first[:, S_G:S_G + 6] = cs[:, None] * (jus * ru[sel][:, None] + jvs * rv[sel][:, None])
    second[:, S_G:S_G + 6] = hs * (gds / hds)[:, None]
    first[:, S_COST] = rob[sel]
    second[:, S_COST] = -w * dprior[sel] ** 2
    first[:, S_L1] = np.abs(ru[sel]) + np.abs(rv[sel])
    first[:, S_COUNT] = 1.0
    terms = first - second
    sums, ab = _fsum_cols(terms), _fsum_cols(np.abs(first) + np.abs(second))
    S, g = body_from_sums(sums, A)
    Sabs, gabs = body_from_sums(ab, np.abs(A))
    Hpp, gp = body_from_sums(_fsum_cols(first), A)
    return dict(sums=sums, abs=ab, fwd=_seq_cols(terms), bwd=_seq_cols(terms[::-1]), S=S, g=g, Sabs=Sabs, gabs=gabs, cost=sums[S_COST],
                l1=sums[S_L1], count=n, A=A, valid=valid, prior=prior, rho0=rho0, rho=rho, hpd=hpd, hdd=hdd, gd=gd, Hpp=Hpp, gp=gp,
                margin=f['margin'], rejects=f['rejects'], c=c, ju=ju, jv=jv, jdu=jdu, jdv=jdv, ru=ru, rv=rv)


def ba_reference(depth, flow, mask, motion, rgb2imu, intr, w, rho=None, kernel=None):
    """ba_reference_link for every link of a batch: a list of dicts.  w: a number or (B,)."""
    B = depth.shape[0]
    intr = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (B, 4))
    w = np.broadcast_to(np.asarray(w, np.float64).reshape(-1), (B,))
    return [ba_reference_link(depth[b], flow[b], None if mask is None else mask[b], motion[b], rgb2imu, intr[b], float(w[b]),
                              None if rho is None else rho[b], kernel) for b in range(B)]


def ba_refine_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, kernel=None, iters=20, damping=1e-4, min_count=16, order='sums'):
    """The joint LM of islam_dense_ba_refine for one link: section 3.23's schedule and accept rule, the damping on the pose block
    only, the device's inverse-depth update (a trial that is not finite or is <= 0 keeps the pixel's rho; a pixel invalid at the
    current state returns to its prior; a pixel without a prior stays at 0).  ``order`` picks which of the restatement's sums drives
    it.  Returns dict(motion, rho, status, accepted, rejected, damping, last_step (the larger of |delta| and max |delta rho| of the
    last trial), trace, valid).  (Beside refine_reference_link and not folded into it: the two loops differ in the trial state, the
    BADPRIOR exit and what a failed factorisation leaves behind, not only in the state they carry.)"""
    def evaluate(X, rho):
        r = ba_reference_link(depth, flow, mask, X, rgb2imu, intr, w, rho, kernel)
        r['Sd'], r['gsd'] = body_from_sums(r[order], r['A'])
        r['cost_o'] = r[order][S_COST]
        r['finite'] = bool(np.isfinite(r[order]).all())
        return r

    cur = np.asarray(motion, np.float64).copy()
    st = evaluate(cur, None)
    rho = st['rho0'].copy()
    out = dict(motion=cur, rho=rho, status=OK, accepted=0, rejected=0, damping=float(damping), last_step=float('nan'),
               trace=[st['cost_o'] / st['count'] if st['count'] else float('nan')], valid=st['valid'])
    if not w > 0:
        out['status'] = BADPRIOR
        return out
    if not (st['finite'] and st['count'] >= min_count):
        out['status'] = FEW
        return out
    for _ in range(1, iters):
        Sd = st['Sd'] + out['damping'] * np.diag(np.diag(st['Sd']))
        try:
            L = np.linalg.cholesky(Sd)
        except np.linalg.LinAlgError:
            out['status'] = NOTPD
            break
        delta = np.linalg.solve(L.T, np.linalg.solve(L, -st['gsd']))
        dcam = st['A'] @ delta
        trial_pose = right_perturb(cur, delta)
        with np.errstate(all='ignore'):
            stepped = rho - (st['gd'] + st['hpd'] @ dcam) / st['hdd']
        stepped = np.where(np.isfinite(stepped) & (stepped > 0), stepped, rho)
        trial_rho = np.where(st['valid'], stepped, st['rho0'])
        out['last_step'] = float(max(np.linalg.norm(delta), np.abs(trial_rho - rho)[st['valid']].max()))
        tr = evaluate(trial_pose, trial_rho)
        out['trace'].append(tr['cost_o'] / tr['count'] if tr['count'] else float('nan'))
        if tr['finite'] and tr['count'] >= min_count and tr['cost_o'] / tr['count'] < st['cost_o'] / st['count']:
            cur, rho, st = trial_pose, trial_rho, tr
            out['damping'] = max(out['damping'] / 10.0, LAMBDA_MIN)
            out['accepted'] += 1
        else:
            out['damping'] = min(out['damping'] * 10.0, LAMBDA_MAX)
            out['rejected'] += 1
    out['motion'], out['rho'], out['valid'] = cur, rho, st['valid']
    return out


# ------------------------------------------------------------------------------------------------ seeded scenes
# (H, W): fx, fy, cx, cy of link 0.  fx is below half the width (the |Q_x/Q_z| <= 1 clause drops border columns), fy just below
# cy (it drops the border rows).
INTRINSICS = {(7, 9): (4.3, 3.2, 3.6, 2.7), (24, 40): (15.0, 11.0, 19.5, 11.5), (72, 96): (40.0, 34.0, 47.5, 35.5),
              (136, 168): (70.0, 65.0, 83.5, 67.5)}


def make_scene(B, H, W, seed, noise=0.0, outliers=0.0, intr0=None, low_depth=True, user_mask=True, flow_dtype=np.float32, motion=None,
               vary=True):
    """B links of H x W: depth in [2, 10] (float32; every 17th pixel at 0.05 when low_depth), a planted body-frame motion per link
    (a few tenths of a metre, a few hundredths of a radian), the mount MOUNT, per-link intrinsics, a user mask with about 10 %
    zeros, and the flow that makes the residual zero at the planted motion, plus Gaussian ``noise`` (pixels) and a fraction
    ``outliers`` of pixels moved by up to +-20 px.  motion (B,7): planted motions to use instead of the drawn ones; vary=False:
    one set of intrinsics for all links.  Returns a dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = INTRINSICS[(H, W)] if intr0 is None else intr0
    k = 1.0 if vary else 0.0          # vary: every link has its own intrinsics
    intr = np.stack([[fx * (1 + 0.02 * k * b), fy * (1 - 0.015 * k * b), cx + 0.3 * k * b, cy - 0.2 * k * b] for b in range(B)])
    planted = lie.se3_exp(np.concatenate([rng.uniform(-0.3, 0.3, (B, 3)), rng.uniform(-0.04, 0.04, (B, 3))], 1))
    motion = planted if motion is None else np.asarray(motion, np.float64)
    depth = rng.uniform(2.0, 10.0, (B, H, W)).astype(np.float32)
    if low_depth:
        depth.reshape(B, -1)[:, 3::17] = 0.05
    mask = (rng.random((B, H, W)) > 0.1) if user_mask else np.ones((B, H, W), bool)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    flow = np.zeros((B, 2, H, W))
    for b in range(B):
        T = lie.se3_mul(lie.se3_mul(lie.se3_inv(MOUNT), motion[b]), MOUNT)
        Ti = lie.se3_inv(T)
        z = depth[b].astype(np.float64)
        P = np.stack([z * ((u - intr[b, 2]) / intr[b, 0]), z * ((v - intr[b, 3]) / intr[b, 1]), z], -1)
        Q = P @ lie.quat_matrix(Ti[3:]).T + Ti[:3]
        ok = Q[..., 2] > 0.05
        Qz = np.where(ok, Q[..., 2], 1.0)
        flow[b, 0] = np.where(ok, intr[b, 0] * Q[..., 0] / Qz + intr[b, 2] - u, 0.0)
        flow[b, 1] = np.where(ok, intr[b, 1] * Q[..., 1] / Qz + intr[b, 3] - v, 0.0)
    flow = np.clip(flow, -4.0 * W, 4.0 * W)
    if noise:
        flow += noise * rng.standard_normal(flow.shape)
    if outliers:
        hit = rng.random((B, 1, H, W)) < outliers
        flow += np.where(hit, rng.uniform(-20.0, 20.0, flow.shape), 0.0)
    return dict(depth=depth, flow=flow.astype(flow_dtype), mask=mask, motion=motion, intr=intr, rgb2imu=MOUNT.copy())


def scene_args(sc, motion=None):
    return (sc['depth'], sc['flow'], sc['mask'], sc['motion'] if motion is None else motion, sc['rgb2imu'], sc['intr'])


SIGMA_RHO = 0.02          # 1/m: the inverse-depth noise of the planted scenes
PRIOR_W = (0.3 / SIGMA_RHO) ** 2          # w = sigma_px^2 / sigma_rho^2 at their 0.3 px of flow noise
XI0 = np.array([0.03, -0.04, 0.03, 0.03, -0.02, 0.03]) * (0.08 / np.linalg.norm([0.03, -0.04, 0.03, 0.03, -0.02, 0.03]))


def noisy_prior(sc, seed, sigma_rho=SIGMA_RHO):
    """The scene of make_scene with its depth map replaced by a noisy prior: 1 / (1/depth + sigma_rho N(0,1)), float32.  The flow
    stays the one of the true depth; ``rho_true`` keeps 1/depth of the true map."""
    rng = np.random.default_rng(seed)
    true = sc['depth'].astype(np.float64)
    rho = 1.0 / true + sigma_rho * rng.standard_normal(true.shape)
    assert (rho > 0).all()
    return dict(sc, depth=(1.0 / rho).astype(np.float32), rho_true=1.0 / true)


def planted_scene(H, W, seed, sigma_rho=SIGMA_RHO, noise=0.3):
    """The planted two-view scene of DESIGN.md section 3.25: one link, identity mount, fx = fy = 0.6 W, principal point at the centre,
    true depth uniform in [3, 8] m, a true motion of up to 0.3 m / 0.04 rad per axis, the exact flow of the true depth plus
    ``noise`` px, and as the depth map the true inverse depth plus ``sigma_rho`` N(0,1), stored as float32 depth.  No mask."""
    rng = np.random.default_rng(seed)
    intr = np.array([[0.6 * W, 0.6 * W, (W - 1) / 2.0, (H - 1) / 2.0]])
    motion = lie.se3_exp(np.concatenate([rng.uniform(-0.3, 0.3, (1, 3)), rng.uniform(-0.04, 0.04, (1, 3))], 1))
    true = rng.uniform(3.0, 8.0, (1, H, W))
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    Ti = lie.se3_inv(motion[0])
    P = np.stack([true[0] * ((u - intr[0, 2]) / intr[0, 0]), true[0] * ((v - intr[0, 3]) / intr[0, 1]), true[0]], -1)
    Q = P @ lie.quat_matrix(Ti[3:]).T + Ti[:3]
    flow = np.stack([intr[0, 0] * Q[..., 0] / Q[..., 2] + intr[0, 2] - u, intr[0, 1] * Q[..., 1] / Q[..., 2] + intr[0, 3] - v])[None]
    flow = flow + noise * rng.standard_normal(flow.shape)
    rho = 1.0 / true + sigma_rho * rng.standard_normal(true.shape)
    assert (rho > 0).all()
    return dict(depth=(1.0 / rho).astype(np.float32), flow=flow.astype(np.float32), mask=np.ones((1, H, W), bool), motion=motion, intr=intr,
                rgb2imu=None, rho_true=1.0 / true, start=right_perturb(motion, XI0))


PLANTED_SEED = 0


@functools.lru_cache(maxsize=None)
def planted_case(H, W):
    """The planted scene of a size, the restatement's joint refinement of it in the three summation orders (20 evaluations) and its
    pose-only refinement (computed once, shared between the CPU and the GPU tests)."""
    sc = planted_scene(H, W, PLANTED_SEED)
    w = PRIOR_W
    run = lambda order: ba_refine_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['start'][0], None, sc['intr'][0], w, iters=20,
                                                 order=order)
    pose_only = refine_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['start'][0], sc['rgb2imu'], sc['intr'][0], iters=20)
    return sc, w, {o: run(o) for o in ('sums', 'fwd', 'bwd')}, pose_only


def pose_dist(a, b):
    return float(np.linalg.norm(lie.se3_log(lie.se3_mul(lie.se3_inv(a), b))))


# ------------------------------------------------------------------------------------------------ what the GPU test files share
KERNELS = {'none': None, 'huber': robust.Huber(1.0), 'cauchy': robust.Cauchy(1.0)}
SHAPES = [(1, 7, 9), (3, 24, 40), (1, 24, 40), (3, 136, 168)]
SEEDS = {7: 107, 24: 124, 136: 201}          # seeds at which test_scene_conditions holds on every link (the 0.05 depths of a link pass or fail
                                             # the Q_z clause together, depending on the planted translation)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to('cuda')
    return t if dtype is None else t.to(dtype)


def _dev_args(sc, motion=None):
    return (_dev(sc['depth']), _dev(sc['flow']), _dev(sc['mask']), _dev(sc['motion'] if motion is None else motion), _dev(sc['intr']))
