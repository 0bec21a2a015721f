"""Dense reprojection normal equations (include/islam_hip.h, "dense reprojection"): the float64 numpy
restatement of the definitions, its Levenberg-Marquardt, the seeded scenes the GPU tests share, and everything that can be checked
without a GPU -- the convention (gradient against central differences, the quadratic form, the mount conjugation),
PvgoInfo.from_dense_reproj, the host-side argument errors and the kernels' register metadata."""
import math
import os

import numpy as np
import pytest
import torch

from islam_amd import robust
from islam_amd.information import PvgoInfo
from oracle import lie

NSUM, S_G, S_COST, S_L1, S_COUNT = 30, 21, 27, 28, 29
TRIU = np.triu_indices(6)
LAMBDA_MIN, LAMBDA_MAX = 1e-12, 1e12          # ISLAM_DENSE_REPROJ_LAMBDA_MIN / _MAX
OK, FEW, NOTPD = 0, 1, 2                      # ISLAM_DENSE_REPROJ_OK / _FEW / _NOTPD
MOUNT = np.concatenate([[0.1, -0.05, 0.2], lie.so3_exp(np.array([0.3, -0.2, 0.4]))])


# ------------------------------------------------------------------------------------------------ the restatement
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


def reproj_reference_link(depth, flow, mask, motion, rgb2imu, intr, kernel=None):
    """One link, pixel by pixel from the header's definitions, float64.  depth (H,W), flow (2,H,W), mask (H,W) or None, motion (7),
    rgb2imu (7) or None, intr (4).  Returns a dict: sums (30, camera frame, each the correctly rounded sum of its terms), abs
    (30, sum |term|), fwd / bwd (30, the terms added in pixel order and in reverse), H, g (body frame, from sums), Habs, gabs (abs
    pushed through |A|), cost, l1, count, A, valid (H,W) and, for every pixel the user mask keeps, the margin of each clause
    relative to its threshold (margin, (n,3); NaN where an earlier clause already dropped the pixel) and rejects (3): how many
    pixels each clause drops."""
    Hh, Ww = depth.shape
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
    z = np.asarray(depth, np.float64)
    P = np.stack([z * ((u - cx) / fx), z * ((v - cy) / fy), z], -1)
    Q = P @ R.T + t
    user = np.ones((Hh, Ww), bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(divide='ignore', invalid='ignore'):
        px, py = Q[..., 0] / Q[..., 2], Q[..., 1] / Q[..., 2]
    c1 = Q[..., 2] > 0.1
    c2 = np.abs(px) <= 1.0
    c3 = np.abs(py) <= 1.0
    valid = user & c1 & c2 & c3
    margin = np.stack([np.abs(Q[..., 2] - 0.1) / 0.1, np.where(c1, np.abs(1.0 - np.abs(px)), np.nan),
                       np.where(c1, np.abs(1.0 - np.abs(py)), np.nan)], -1)[user]
    rejects = np.array([(user & ~c1).sum(), (user & c1 & ~c2).sum(), (user & c1 & ~c3).sum()])
    Qx, Qy, Qz = (Q[..., k][valid] for k in range(3))
    uu, vv = u[valid], v[valid]
    fl = np.asarray(flow, np.float64)
    ru = fx * (Qx / Qz) + cx - (fl[0][valid] + uu)
    rv = fy * (Qy / Qz) + cy - (fl[1][valid] + vv)
    s = ru * ru + rv * rv
    if kernel is None:
        rho, c = s, np.ones_like(s)
    else:
        rho, c = kernel.rho(s), kernel.weight(s)
    a, bq, cq, dq = fx / Qz, -fx * Qx / Qz ** 2, fy / Qz, -fy * Qy / Qz ** 2
    zero = np.zeros_like(a)
    ju = np.stack([-a, zero, -bq, -bq * Qy, bq * Qx - a * Qz, a * Qy], -1)          # rows of dr/dQ [-I, [Q]x]
    jv = np.stack([zero, -cq, -dq, cq * Qz - dq * Qy, dq * Qx, -cq * Qx], -1)
    terms = np.zeros((s.shape[0], NSUM))
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
                l1=sums[S_L1], count=int(s.shape[0]), A=A, valid=valid, margin=margin, rejects=rejects)


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


# ------------------------------------------------------------------------------------------------ the convention
def _cost(sc, motion, kernel, b=0):
    r = reproj_reference_link(sc['depth'][b], sc['flow'][b], sc['mask'][b], motion, sc['rgb2imu'], sc['intr'][b], kernel)
    return r['cost'], r['valid']


@pytest.mark.parametrize('kernel', [None, robust.Cauchy(1.0)], ids=['none', 'cauchy'])
def test_gradient_matches_central_differences(kernel):
    """2 g = d cost / d xi under motion Exp(xi).  The difference quotient D(h) has truncation error (D(2h) - D(h)) / 3 + O(h^4)
    (Richardson); the check holds |D(h) - 2 g| to three times that estimate plus the quotient's rounding, 64 eps cost / h.  The
    scene keeps every pixel well inside the validity clauses, so the cost is smooth over the stencil (asserted)."""
    sc = make_scene(1, 24, 40, seed=3, noise=0.3, intr0=(40.0, 40.0, 19.5, 11.5), low_depth=False, flow_dtype=np.float64)
    start = right_perturb(sc['motion'][0], [0.01, -0.02, 0.015, 0.004, -0.003, 0.005])
    ref = reproj_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], start, sc['rgb2imu'], sc['intr'][0], kernel)
    assert ref['count'] > 800 and np.linalg.norm(ref['g']) > 1.0
    h = 1e-4
    for k in range(6):
        D = []
        for step in (h, 2 * h):
            e = np.zeros(6)
            e[k] = step
            (cp, vp), (cm, vm) = _cost(sc, right_perturb(start, e), kernel), _cost(sc, right_perturb(start, -e), kernel)
            assert np.array_equal(vp, ref['valid']) and np.array_equal(vm, ref['valid'])
            D.append((cp - cm) / (2 * step))
        tol = abs(D[1] - D[0]) + 64 * np.finfo(np.float64).eps * ref['cost'] / h
        print('dir %d: D(h) %.12e  2g %.12e  diff %.3e  tol %.3e' % (k, D[0], 2 * ref['g'][k], abs(D[0] - 2 * ref['g'][k]), tol))
        assert abs(D[0] - 2 * ref['g'][k]) <= tol
        assert tol < 1e-4 * np.abs(2 * ref['g']).max()          # the bound itself is tight enough to see a wrong sign or column
    assert np.abs(ref['g']).min() > 1e-3 * np.abs(ref['g']).max()  # ... in every direction


@pytest.mark.parametrize('mount', [True, False], ids=['mount', 'identity'])
def test_cost_is_the_quadratic_form_of_H(mount):
    """Flow with r = 0 at the pose: cost(motion Exp(xi)) = xi^T H xi up to third order.  Pins the frame and the row order
    independently of the Jacobian code.  |xi| = 2e-4: the relative defect is O(|xi|) times the ratio of the third to the second
    derivative, measured 1e-5 .. 1e-4; held to 1e-3 (a wrong frame, sign or row order gives O(1))."""
    sc = make_scene(1, 24, 40, seed=5, intr0=(40.0, 40.0, 19.5, 11.5), low_depth=False, flow_dtype=np.float64)
    if not mount:
        sc['rgb2imu'] = None
        sc = dict(sc, flow=_zero_residual_flow(sc))
    ref = reproj_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['motion'][0], sc['rgb2imu'], sc['intr'][0])
    assert ref['cost'] < 1e-20 and ref['count'] > 800
    rng = np.random.default_rng(0)
    for _ in range(5):
        xi = rng.standard_normal(6)
        xi *= 2e-4 / np.linalg.norm(xi)
        cost, valid = _cost(sc, right_perturb(sc['motion'][0], xi), None)
        assert np.array_equal(valid, ref['valid'])
        quad = xi @ ref['H'] @ xi
        print('cost %.6e quad %.6e rel %.2e' % (cost, quad, abs(cost - quad) / quad))
        assert abs(cost - quad) <= 1e-3 * quad


def _zero_residual_flow(sc):
    """The flow of make_scene recomputed for an identity mount."""
    B, H, W = sc['depth'].shape
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    flow = np.zeros((B, 2, H, W))
    for b in range(B):
        Ti = lie.se3_inv(sc['motion'][b])
        z = sc['depth'][b].astype(np.float64)
        fx, fy, cx, cy = sc['intr'][b]
        Q = np.stack([z * ((u - cx) / fx), z * ((v - cy) / fy), z], -1) @ lie.quat_matrix(Ti[3:]).T + Ti[:3]
        flow[b, 0] = fx * Q[..., 0] / Q[..., 2] + cx - u
        flow[b, 1] = fy * Q[..., 1] / Q[..., 2] + cy - v
    return flow


def test_mount_conjugates_by_the_adjoint():
    """With a mount C the body-frame result is the identity-mount result at T = C^-1 motion C, conjugated by A = Ad(C^-1)."""
    sc = make_scene(2, 24, 40, seed=7, noise=0.3)
    for b in range(2):
        body = reproj_reference_link(sc['depth'][b], sc['flow'][b], sc['mask'][b], sc['motion'][b], MOUNT, sc['intr'][b], robust.Huber(1.0))
        T = lie.se3_mul(lie.se3_mul(lie.se3_inv(MOUNT), sc['motion'][b]), MOUNT)
        cam = reproj_reference_link(sc['depth'][b], sc['flow'][b], sc['mask'][b], T, None, sc['intr'][b], robust.Huber(1.0))
        A = lie.se3_adj(lie.se3_inv(MOUNT))
        assert body['count'] == cam['count'] > 400
        np.testing.assert_allclose(body['H'], A.T @ cam['H'] @ A, rtol=0, atol=1e-12 * np.abs(body['H']).max())
        np.testing.assert_allclose(body['g'], A.T @ cam['g'], rtol=0, atol=1e-12 * np.abs(body['g']).max())
        assert (np.abs(body['sums'] - cam['sums']) <= 1e-12 * cam['abs']).all()
        assert np.abs(body['H'] - cam['H']).max() > 1e-3 * np.abs(cam['H']).max()          # the mount matters


def test_restatement_l1_is_the_loss_call():
    """l1 / count of the restatement is DenseReprojectionLoss.__call__ (float64, CPU tensors) on the same scene."""
    from islam_amd import lietensor as pp
    from islam_amd.dense_ba import DenseReprojectionLoss
    sc = make_scene(1, 24, 40, seed=9, noise=0.3)
    fx, fy, cx, cy = sc['intr'][0]
    loss = DenseReprojectionLoss(torch.from_numpy(sc['depth']).double(), torch.from_numpy(sc['flow']).double(), fx, fy, cx, cy,
                                 torch.from_numpy(sc['mask']), pp.SE3(torch.from_numpy(MOUNT)), device='cpu')
    start = right_perturb(sc['motion'], [0.02, 0.01, -0.02, 0.01, 0.0, -0.01])
    got = loss(pp.SE3(torch.from_numpy(start))).numpy()
    ref = reproj_reference(*scene_args(sc, start))[0]
    assert ref['rejects'].min() > 0 and ref['count'] > 480
    assert abs(got[0] - ref['l1'] / ref['count']) <= 2.0 ** -52 * (64 + ref['count']) * ref['abs'][S_L1] / ref['count']


def test_refine_reference_converges():
    """The LM restatement on a planted case: from 0.08 away it ends at least 5 x closer, and its last step is below 1e-6."""
    sc = make_scene(1, 24, 40, seed=23, noise=0.3)
    xi0 = np.array([0.03, -0.04, 0.03, 0.03, -0.02, 0.03])
    xi0 *= 0.08 / np.linalg.norm(xi0)
    start = right_perturb(sc['motion'][0], xi0)
    r = refine_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], start, MOUNT, sc['intr'][0], iters=10)
    end = np.linalg.norm(lie.se3_log(lie.se3_mul(lie.se3_inv(sc['motion'][0]), r['motion'])))
    print('start 0.08, end %.3e, last step %.3e, accepted %d rejected %d' % (end, r['last_step'], r['accepted'], r['rejected']))
    assert r['status'] == OK and end * 5 <= 0.08 and r['last_step'] < 1e-6
    assert r['accepted'] + r['rejected'] == 9


# ------------------------------------------------------------------------------------------------ PvgoInfo.from_dense_reproj
def test_from_dense_reproj_algebra_and_errors():
    rng = np.random.default_rng(2)
    J = rng.standard_normal((4, 30, 6))
    H = np.einsum('eki,ekj->eij', J, J)
    info = PvgoInfo.from_dense_reproj(H, sigma_px=0.5)
    np.testing.assert_array_equal(info.vo, 0.5 * (H / 0.25 + np.swapaxes(H / 0.25, 1, 2)))
    assert info.vel is None and info.rot is None and info.transvel is None and info.imu is None
    fl = PvgoInfo.from_dense_reproj(torch.from_numpy(H), sigma_px=2.0, floor=1e-3, vel=np.full(4, 3.0))
    np.testing.assert_allclose(fl.vo, H / 4.0 + 1e-3 * np.eye(6), rtol=1e-15)
    np.testing.assert_array_equal(fl.vel, 3.0 * np.broadcast_to(np.eye(3), (4, 3, 3)))
    imu = np.broadcast_to(np.eye(9), (4, 9, 9))
    np.testing.assert_array_equal(PvgoInfo.from_dense_reproj(H, imu=imu).imu, imu)
    off = H.copy()
    off[2] = 0.0                                                   # an edge without valid pixels: factor off
    assert np.array_equal(PvgoInfo.from_dense_reproj(off).vo[2], np.zeros((6, 6)))
    vo = info.matrices(4, 4, (1, 1, 1, 1))[0]
    np.testing.assert_array_equal(vo, info.vo)
    with pytest.raises(ValueError, match='graph has 5'):
        info.matrices(5, 5, (1, 1, 1, 1))
    bad = H.copy()
    bad[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match='vo: factor 1 has a non-finite'):
        PvgoInfo.from_dense_reproj(bad)
    neg = H.copy()
    neg[3] = -neg[3]
    with pytest.raises(ValueError, match='vo: factor 3 is not positive semi-definite'):
        PvgoInfo.from_dense_reproj(neg)
    for kw in (dict(sigma_px=0.0), dict(sigma_px=-1.0), dict(sigma_px=float('nan')), dict(floor=-1.0)):
        with pytest.raises(ValueError):
            PvgoInfo.from_dense_reproj(H, **kw)
    with pytest.raises(ValueError, match=r'\(E,6,6\)'):
        PvgoInfo.from_dense_reproj(H[:, :5, :5])
    with pytest.raises(ValueError, match='imu'):
        PvgoInfo.from_dense_reproj(H, imu=imu, rot=np.ones(4))


# ------------------------------------------------------------------------------------------------ the library without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    from islam_amd import _lib
    one = 1        # any non-NULL address: a refused call never reads it
    assert lib.islam_dense_reproj_scratch_bytes(0, 0) == 0
    b0, b1 = lib.islam_dense_reproj_scratch_bytes(3, 0), lib.islam_dense_reproj_scratch_bytes(3, 10)
    assert b0 >= 8 * 3 * _lib.DENSE_REPROJ_NBLK * _lib.DENSE_REPROJ_NSUM and b1 >= b0 + 8 * 3 * 7

    def normal(B=1, H=2, W=2, kind=0, delta=1.0, depth=one, out=one, scratch=one):
        return lib.islam_dense_reproj_normal(depth, one, None, one, None, one, kind, delta, out, one, one, one, one, one, scratch, B, H, W, None)

    def refine(B=1, H=2, W=2, kind=0, delta=1.0, iters=3, status=one, trace=None, cap=0, damping=1e-4):
        return lib.islam_dense_reproj_refine(one, one, None, one, None, one, kind, delta, iters, damping, 16.0, one, one, one, one, one, one, one,
                                             one, one, one, status, trace, cap, one, B, H, W, None)

    for call, name in ((normal, b'islam_dense_reproj_normal'), (refine, b'islam_dense_reproj_refine')):
        for kw, what in ((dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
                         (dict(kind=3), b'robust kind'), (dict(kind=-1), b'robust kind'), (dict(kind=1, delta=0.0), b'delta'),
                         (dict(delta=-2.0), b'delta'), (dict(delta=float('nan')), b'delta')):
            assert call(**kw) == -1, kw
            msg = lib.islam_last_error()
            assert name in msg and what in msg, (kw, msg)
    for kw in (dict(depth=None), dict(out=None), dict(scratch=None)):
        assert normal(**kw) == -1 and b'islam_dense_reproj_normal: NULL' in lib.islam_last_error()
    for kw, what in ((dict(iters=0), b'iters'), (dict(iters=-4), b'iters'), (dict(status=None), b'NULL'), (dict(cap=4), b'trace'),
                     (dict(damping=-1.0), b'damping')):
        assert refine(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_dense_reproj_refine' in msg and what in msg, (kw, msg)


def test_ops_refuse_cpu_tensors():
    from islam_amd import ops
    sc = make_scene(1, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (t(sc['depth']), t(sc['flow']), t(sc['mask']), t(sc['motion']), t(sc['intr']))
    with pytest.raises(RuntimeError):
        ops.dense_reproj_normal(*args)
    with pytest.raises(RuntimeError):
        ops.dense_reproj_refine(*args, iters=3)


def test_dense_reproj_kernels_do_not_spill(lib):
    """Thirty fp64 accumulators plus the pose are tight: neither kernel may have a private segment or a spilled VGPR."""
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = {n: blk for n, blk in _kernels().items() if 'dense_reproj' in n}
    assert any('dense_reproj_partial_kernel' in n for n in ks) and any('dense_reproj_final_kernel' in n for n in ks) and len(ks) == 2
    for n, blk in ks.items():
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, n
