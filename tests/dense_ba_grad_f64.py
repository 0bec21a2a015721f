"""The float64 numpy restatement of the gradient of the joint dense bundle adjustment in depth and flow (include/islam_hip.h,
islam_dense_ba_ift_weights / islam_dense_ba_vjp), a helper module beside dense_reproj_f64.py and not a test
file.  Built on that module's ba_reference_link (the per-pixel terms of the joint problem) and link_front (c' and the parts of r):
the adjoint solve by per-pixel elimination (ba_adjoint_reference_link), the gradient of Phi = lambda^T G in depth and flow with, per
element, the sum of the magnitudes of the products it is summed from (ba_vjp_reference_link), Phi itself (ba_phi), and the implicit
gradient of a loss on a refinement's outputs (ba_implicit_gradient).  tests/test_dense_ba_grad_cpu.py checks this module against
central differences, an explicitly assembled system and re-refinement; tests/test_dense_ba_grad_gpu.py holds the kernels to it."""
import math

import numpy as np

from tests.dense_reproj_f64 import _fsum_cols, _user, ba_reference_link, link_front, tangent_from_pose_grad

# Roundings in one term of u_cam = sum h_pd v_d / h_dd, counted from joint_adj_partial_kernel's arithmetic as section 3.25 counts its
# 128: section 3.23's 64 for everything up to c and J_cam, then 1/rho (1), R ray (10), -1/rho^2 (2), jd (8), e = c jd (2), h_dd (4),
# v_d / h_dd (1), an entry of h_pd = e_u ju + e_v jv (3) and its product with v_d / h_dd (1): 96, rounded up to the same 128.
K_ADJ = 128


def _front(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel):
    """ba_reference_link at (motion, rho) and the link_front call it makes (for c' = dc/ds, s and the parts of r)."""
    r = ba_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel)
    usable = r['prior'] & np.isfinite(r['rho']) & (r['rho'] > 0)
    f = link_front(1.0 / np.where(usable, r['rho'], 1.0), flow, _user(mask, depth.shape) & usable, motion, rgb2imu, intr, kernel)
    assert np.array_equal(f['valid'], r['valid'])
    return r, f


def _lambda_d(r, lam_cam, v_d):
    """lambda_d = -(v_d + h_pd^T lambda_cam) / h_dd at every pixel with a prior (c = 0, h_dd = w at an invalid one), 0 elsewhere."""
    with np.errstate(all='ignore'):
        ld = -(v_d + r['hpd'] @ lam_cam) / r['hdd']
    return np.where(r['prior'], ld, 0.0)


def ba_adjoint_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, v_p, v_d=None, kernel=None, S=None):
    """The adjoint solve H_full lambda = -v of one link at the state (motion, rho) by per-pixel elimination.  Arguments of
    ba_reference_link, then v_p (6): the loss's gradient in the right tangent of the pose (body frame), v_d (H,W) or None (0): its
    gradient on every inverse depth, S (6,6) or None: the Schur matrix to solve with (None: the restatement's own).  Returns a dict:
    u_cam (6, each the correctly rounded sum of its terms), u_abs (6: the sum over the pixels of |c ju jd v_d / h_dd| +
    |c jv jd v_d / h_dd|), lam_p (6, body frame), lam_cam = A lam_p, lam_d (H,W; 0 where the depth gives no prior), S, A, valid,
    prior, count."""
    r = ba_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel)
    v_d = np.zeros(depth.shape) if v_d is None else np.asarray(v_d, np.float64)
    sel = r['valid']
    k = (v_d[sel] / r['hdd'][sel])[:, None]
    c, ju, jv, jdu, jdv = (r[x][sel] for x in ('c', 'ju', 'jv', 'jdu', 'jdv'))
    u = _fsum_cols(r['hpd'][sel] * k)
    u_abs = _fsum_cols(c[:, None] * (np.abs(ju * jdu[:, None]) + np.abs(jv * jdv[:, None])) * np.abs(k))
    S = r['S'] if S is None else np.asarray(S, np.float64)
    lam_p = -np.linalg.solve(S, np.asarray(v_p, np.float64) - r['A'].T @ u)
    lam_cam = r['A'] @ lam_p
    return dict(u_cam=u, u_abs=u_abs, lam_p=lam_p, lam_cam=lam_cam, lam_d=_lambda_d(r, lam_cam, v_d), S=S, A=r['A'], valid=sel, prior=r['prior'],
                count=r['count'])


def ba_vjp_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, lam_p, v_d=None, kernel=None):
    """dPhi/d(depth, flow) of one link, Phi = lam_p^T g_p + sum lam_d g_d with the state, lambda and the valid set held fixed, pixel by
    pixel from the header's formulas, float64.  Arguments of ba_reference_link, lam_p (6, body frame) and v_d (H,W) or None (0).
    Returns a dict: grad_depth (H,W) = w lam_d / depth^2 (0 without a prior), grad_flow (2,H,W) = -(c q + 2 c' (q.r) r) (0 where
    invalid), abs_depth, abs_flow: per element the sum of |term| over the products the value is summed from (the entries of dr/dQ, Q,
    R ray, lambda_cam, c, c', h_dd and v_d are leaves; the rows of J_cam and jd enter with the magnitudes of their own products, r
    with |fx p| + |cx| + |flow| + |u| as in vjp_reference_link), lam_d, valid, prior, s (NaN where invalid)."""
    r, f = _front(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel)
    v_d = np.zeros(depth.shape) if v_d is None else np.asarray(v_d, np.float64)
    valid, prior = r['valid'], r['prior']
    lam_cam = r['A'] @ np.asarray(lam_p, np.float64)
    lam_d = _lambda_d(r, lam_cam, v_d)
    z = np.where(prior, np.asarray(depth, np.float64), 1.0)
    grad_depth = np.where(prior, w * lam_d / (z * z), 0.0)
    la = np.abs(lam_cam)
    a, bq, cq, dq, Qx, Qy, Qz = (np.abs(f[k]) for k in ('a', 'bq', 'cq', 'dq', 'Qx', 'Qy', 'Qz'))
    zero = np.zeros_like(a)
    with np.errstate(all='ignore'):          # an invalid pixel may hold anything
        c, cp, ru, rv = r['c'], np.where(valid, f['cp'], 0.0), r['ru'], r['rv']
        du, dv = r['ju'] @ lam_cam, r['jv'] @ lam_cam
        qu, qv = du + r['jdu'] * lam_d, dv + r['jdv'] * lam_d
        k2 = 2.0 * cp * (qu * ru + qv * rv)
        eu, ev = c * qu + k2 * ru, c * qv + k2 * rv
        # the same from the magnitudes of the leaves
        jua = np.stack([a, zero, bq, bq * Qy, bq * Qx + a * Qz, a * Qy], -1)
        jva = np.stack([zero, cq, dq, cq * Qz + dq * Qy, dq * Qx, cq * Qx], -1)
        dR = np.abs(f['dQ'])
        kk = 1.0 / np.where(valid, r['rho'], 1.0) ** 2
        jdua, jdva = (a * dR[..., 0] + bq * dR[..., 2]) * kk, (cq * dR[..., 1] + dq * dR[..., 2]) * kk
        dua, dva = jua @ la, jva @ la
        lda = np.where(prior, (np.abs(v_d) + c * (jdua * dua + jdva * dva)) / r['hdd'], 0.0)
        rua = np.abs(f['fx'] * (f['Qx'] / f['Qz'])) + abs(f['cx']) + np.abs(f['fl'][0]) + f['u']
        rva = np.abs(f['fy'] * (f['Qy'] / f['Qz'])) + abs(f['cy']) + np.abs(f['fl'][1]) + f['v']
        qua, qva = dua + jdua * lda, dva + jdva * lda
        k2a = 2.0 * np.abs(cp) * (qua * rua + qva * rva)
        eua, eva = c * qua + k2a * rua, c * qva + k2a * rva
    img = lambda x: np.where(valid, x, 0.0)
    smap = np.where(valid, f['s'], np.nan)
    return dict(grad_depth=grad_depth, grad_flow=np.stack([img(-eu), img(-ev)]), abs_depth=np.where(prior, w * lda / (z * z), 0.0),
                abs_flow=np.stack([img(eua), img(eva)]), lam_d=lam_d, valid=valid, prior=prior, s=smap)


def ba_phi(depth, flow, mask, motion, rgb2imu, intr, w, rho, lam_p, lam_d, kernel=None):
    """Phi = lam_p^T g_p + sum lam_d g_d from ba_reference_link's gradient blocks at the state (motion, rho): g_p = A^T sum c J_cam^T r
    (its 'gp'), g_d per pixel (its 'gd'; w (rho - rho0) at an invalid pixel).  Returns (Phi, the sum of the magnitudes of the products
    Phi is summed from, valid, s (NaN where invalid))."""
    r, f = _front(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel)
    sel, prior = r['valid'], r['prior']
    ld = np.where(prior, lam_d, 0.0)
    phi = float(lam_p @ r['gp']) + math.fsum((ld * r['gd'])[prior])
    c, ju, jv, jdu, jdv, ru, rv = (r[k][sel] for k in ('c', 'ju', 'jv', 'jdu', 'jdv', 'ru', 'rv'))
    gp_abs = np.abs(r['A']).T @ _fsum_cols(c[:, None] * (np.abs(ju * ru[:, None]) + np.abs(jv * rv[:, None])))
    mag = float(np.abs(lam_p) @ gp_abs) + math.fsum(np.abs(ld[sel]) * c * (np.abs(jdu * ru) + np.abs(jdv * rv))) + \
        math.fsum((np.abs(ld) * w * (np.abs(r['rho']) + r['rho0']))[prior])
    return phi, mag, sel, np.where(sel, f['s'], np.nan)


def ba_implicit_gradient(depth, flow, mask, motion, rgb2imu, intr, w, rho, grad7, v_d=None, kernel=None, S=None):
    """The implicit-function gradient in depth and flow of a loss with gradient grad7 on [t, q xyzw] of the refined pose and v_d on the
    refined inverse depths, at the state (motion, rho): the adjoint solve, then the gradient of Phi.  Returns ba_vjp_reference_link's dict
    with the adjoint's (u_cam, u_abs, lam_p, S, A, count) added."""
    adj = ba_adjoint_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, tangent_from_pose_grad(motion, grad7), v_d, kernel, S)
    out = ba_vjp_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, adj['lam_p'], v_d, kernel)
    out.update({k: adj[k] for k in ('u_cam', 'u_abs', 'lam_p', 'S', 'A', 'count')})
    return out


def ba_implicit_gradient_batch(depth, flow, mask, motion, rgb2imu, intr, w, rho, grad7, v_d, S, status=None, kernel=None):
    """ba_implicit_gradient for every link of a batch with the status rule of the entry points: a link whose incoming status is not 0,
    whose prior weight is not > 0 (status 3) or whose S has no Cholesky factor (status 2) gets zeros and lam_p = 0, the others carry
    on.  v_d (B,H,W) or None, S (B,6,6), w a number or (B,), status (B) or None.  Returns (list of dicts with grad_depth, grad_flow,
    lam_p and, for a healthy link, everything of ba_implicit_gradient; the outgoing status (B))."""
    B = depth.shape[0]
    intr = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (B, 4))
    w = np.broadcast_to(np.asarray(w, np.float64).reshape(-1), (B,))
    out, st = [], np.zeros(B, int) if status is None else np.array(status, int)
    for b in range(B):
        if st[b] == 0 and not w[b] > 0:
            st[b] = 3
        if st[b] == 0:
            try:
                np.linalg.cholesky(S[b])
            except np.linalg.LinAlgError:
                st[b] = 2
        if st[b] != 0:
            out.append(dict(grad_depth=np.zeros(depth.shape[1:]), grad_flow=np.zeros((2,) + depth.shape[1:]), lam_p=np.zeros(6)))
            continue
        out.append(ba_implicit_gradient(depth[b], flow[b], None if mask is None else mask[b], motion[b], rgb2imu, intr[b], float(w[b]), rho[b],
                                        grad7[b], None if v_d is None else v_d[b], kernel, S[b]))
    return out, st
