"""Joint (pose, inverse depth) dense bundle adjustment (include/islam_hip.h, islam_dense_ba_normal / _refine):
the float64 numpy restatement of the per-pixel Schur sums and of the joint Levenberg-Marquardt, the planted scenes the GPU tests
share, and everything that can be checked without a GPU -- the Schur complement against the explicitly assembled dense system, the
full gradient against central differences, the two limits (H - S >= 0, S -> H), the planted refinement, the host-side argument
errors and the new kernels' register metadata."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from islam_amd import robust
from oracle import lie
from tests.test_dense_reproj_cpu import (FEW, LAMBDA_MAX, LAMBDA_MIN, MOUNT, NOTPD, NSUM, OK, S_COST, S_COUNT, S_G, S_L1, TRIU, _fsum_cols,
                                         _seq_cols, body_from_sums, make_scene, reproj_reference_link, right_perturb)

BADPRIOR = 3                  # ISLAM_DENSE_REPROJ_BADPRIOR
U = 2.0 ** -52
# Roundings in one term of a camera-frame sum, counted from dense_ba_partial_kernel's arithmetic.  The kernel
# forms a pixel's term as J^T M J with the 2x2 M = c I - e e^T / h_dd, e = c jd (J^T (c r - e g_d / h_dd) on the right-hand side), so
# it has section 3.23's 64 for everything up to c, r and J_cam and the product with J, and on top 1/rho (1), R ray (10), -1/rho^2 (2),
# jd (8), e (2), h_dd (4), g_d with rho0 and rho - rho0 (7), 1/h_dd (1), e / h_dd (2), the entries of M or of c r - e g_d / h_dd (4
# each), and M J in place of c J (3 more per entry): 48 more, 112, rounded up.
K_ROUND = 128


# ------------------------------------------------------------------------------------------------ the restatement
def ba_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho=None, kernel=None):
    """One link of the joint problem at (motion, rho), pixel by pixel from the header's definitions, float64.  depth (H,W), flow
    (2,H,W), mask (H,W) or None, motion (7), rgb2imu (7) or None, intr (4), w > 0, rho (H,W) or None (the prior 1/depth).  Returns a
    dict: sums (30, camera frame, each the correctly rounded sum of its terms), abs (30: per sum, the sum over the pixels of the
    magnitudes of the term's two parts, |c J^T J| + |h_pd h_pd^T / h_dd|), fwd / bwd (the terms added in pixel order and in
    reverse), S, g (body frame), Sabs, gabs (abs pushed through |A|), cost, l1, count, A; per pixel of the whole image (c = 0 at an
    invalid one) hpd (H,W,6, camera frame), hdd, gd, and valid, prior (the depth gives a prior), rho0, rho; Hpp / gp: the body-frame
    pose block sum c J^T J and sum c J^T r before the depths are eliminated; margin / rejects as reproj_reference_link."""
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
    prior = np.isfinite(z) & (z > 0)
    rho0 = np.where(prior, 1.0 / np.where(prior, z, 1.0), 0.0)
    rho = rho0.copy() if rho is None else np.asarray(rho, np.float64)
    usable = prior & np.isfinite(rho) & (rho > 0)
    rs = np.where(usable, rho, 1.0)
    zi = 1.0 / rs
    xh, yh = (u - cx) / fx, (v - cy) / fy
    ray = np.stack([xh, yh, np.ones_like(xh)], -1)
    P = np.stack([zi * xh, zi * yh, zi], -1)
    Q = P @ R.T + t
    dR = ray @ R.T
    user = np.ones((Hh, Ww), bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(divide='ignore', invalid='ignore'):
        px, py = Q[..., 0] / Q[..., 2], Q[..., 1] / Q[..., 2]
    c1 = Q[..., 2] > 0.1
    c2 = np.abs(px) <= 1.0
    c3 = np.abs(py) <= 1.0
    keep = user & usable
    valid = keep & c1 & c2 & c3
    margin = np.stack([np.abs(Q[..., 2] - 0.1) / 0.1, np.where(c1, np.abs(1.0 - np.abs(px)), np.nan),
                       np.where(c1, np.abs(1.0 - np.abs(py)), np.nan)], -1)[keep]
    rejects = np.array([(keep & ~c1).sum(), (keep & c1 & ~c2).sum(), (keep & c1 & ~c3).sum()])
    fl = np.asarray(flow, np.float64)
    Qx, Qy = Q[..., 0], Q[..., 1]
    Qz = np.where(valid, Q[..., 2], 1.0)
    ru = fx * (Qx / Qz) + cx - (fl[0] + u)
    rv = fy * (Qy / Qz) + cy - (fl[1] + v)
    s = ru * ru + rv * rv
    if kernel is None:
        rob, c = s, np.ones_like(s)
    else:
        rob, c = kernel.rho(s), kernel.weight(s)
    c = np.where(valid, c, 0.0)
    a, bq, cq, dq = fx / Qz, -fx * Qx / Qz ** 2, fy / Qz, -fy * Qy / Qz ** 2
    zero = np.zeros_like(a)
    ju = np.stack([-a, zero, -bq, -bq * Qy, bq * Qx - a * Qz, a * Qy], -1)
    jv = np.stack([zero, -cq, -dq, cq * Qz - dq * Qy, dq * Qx, -cq * Qx], -1)
    k = -1.0 / (rs * rs)
    jdu = (a * dR[..., 0] + bq * dR[..., 2]) * k
    jdv = (cq * dR[..., 1] + dq * dR[..., 2]) * k
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
                margin=margin, rejects=rejects, c=c, ju=ju, jv=jv, jdu=jdu, jdv=jdv, ru=ru, rv=rv)


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
    last trial), trace, valid)."""
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


def pose_only_reference_link(sc, iters):
    from tests.test_dense_reproj_cpu import refine_reference_link
    return refine_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['start'][0], sc['rgb2imu'], sc['intr'][0], iters=iters)


@functools.lru_cache(maxsize=None)
def planted_case(H, W):
    """The planted scene of a size, the restatement's joint refinement of it in the three summation orders (20 evaluations) and its
    pose-only refinement (computed once, shared with the GPU tests)."""
    sc = planted_scene(H, W, PLANTED_SEED)
    w = PRIOR_W
    run = lambda order: ba_refine_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['start'][0], None, sc['intr'][0], w, iters=20,
                                                 order=order)
    return sc, w, {o: run(o) for o in ('sums', 'fwd', 'bwd')}, pose_only_reference_link(sc, 20)


def pose_dist(a, b):
    return float(np.linalg.norm(lie.se3_log(lie.se3_mul(lie.se3_inv(a), b))))


# ------------------------------------------------------------------------------------------------ 1. Schur against the dense system
def _dense_system(r, w):
    """The joint Gauss-Newton system assembled explicitly from stacked residual rows: unknowns [xi (6, body frame); rho_i of every
    pixel with a prior], rows sqrt(c) [J_cam A, jd e_i] per valid pixel and component, and sqrt(w) [0, e_i] per prior."""
    idx = np.flatnonzero(r['prior'].ravel())
    n = idx.size
    col = {p: 6 + k for k, p in enumerate(idx)}
    rows, rhs = [], []
    flat = lambda a: a.reshape(-1, *a.shape[2:])
    c, ju, jv, jdu, jdv, ru, rv = (flat(r[k]) for k in ('c', 'ju', 'jv', 'jdu', 'jdv', 'ru', 'rv'))
    rho, rho0, valid = r['rho'].ravel(), r['rho0'].ravel(), r['valid'].ravel()
    for p in idx:
        if valid[p]:
            for j, jd, res in ((ju[p], jdu[p], ru[p]), (jv[p], jdv[p], rv[p])):
                row = np.zeros(6 + n)
                row[:6] = math.sqrt(c[p]) * (j @ r['A'])
                row[col[p]] = math.sqrt(c[p]) * jd
                rows.append(row)
                rhs.append(math.sqrt(c[p]) * res)
        row = np.zeros(6 + n)
        row[col[p]] = math.sqrt(w)
        rows.append(row)
        rhs.append(math.sqrt(w) * (rho[p] - rho0[p]))
    Jb, rb = np.array(rows), np.array(rhs)
    return Jb.T @ Jb, Jb.T @ rb


def test_schur_sums_are_the_schur_complement_of_the_dense_system():
    """7 x 9 with the mount, a user mask and every clause dropping pixels, at a perturbed rho, under Cauchy(1.0), w = 1: S and gs of the
    restatement against the Schur complement of the explicitly assembled (6 + n) x (6 + n) system, and S^-1 against the pose block of
    that matrix's inverse.  Bound: 64 eps cond |value| with cond the condition number of the dense matrix (asserted below 1e9; measured
    1.4e3) and |value| the largest entry of the compared array."""
    sc = noisy_prior(make_scene(1, 7, 9, seed=107, noise=0.3), seed=1)
    start = right_perturb(sc['motion'][0], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    w = 1.0          # a weak prior: at fx = 4.3 the depth columns are of the size of 1 px per 1/m, so here the elimination matters
    rng = np.random.default_rng(4)
    rho = (1.0 / sc['depth'][0].astype(np.float64)) * (1.0 + 0.03 * rng.standard_normal((7, 9)))
    r = ba_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], start, MOUNT, sc['intr'][0], w, rho, robust.Cauchy(1.0))
    assert (r['rejects'] > 0).all() and 2 * r['count'] >= 63 and (~np.asarray(sc['mask'][0])).any()
    Mx, rhs = _dense_system(r, w)
    n = Mx.shape[0] - 6
    assert n == 63
    cond = np.linalg.cond(Mx)
    eps = np.finfo(np.float64).eps
    Sd = Mx[:6, :6] - Mx[:6, 6:] @ np.linalg.solve(Mx[6:, 6:], Mx[6:, :6])
    gd = rhs[:6] - Mx[:6, 6:] @ np.linalg.solve(Mx[6:, 6:], rhs[6:])
    inv = np.linalg.inv(Mx)[:6, :6]
    Si = np.linalg.inv(r['S'])
    errs = [np.abs(r['S'] - Sd).max() / np.abs(Sd).max(), np.abs(r['g'] - gd).max() / np.abs(gd).max(), np.abs(Si - inv).max() / np.abs(inv).max()]
    print('cond %.3e, bound %.3e; relative errors: S %.3e, gs %.3e, S^-1 %.3e' % (cond, 64 * eps * cond, *errs))
    assert cond < 1e9
    assert max(errs) <= 64 * eps * cond
    assert np.abs(r['S'] - r['Hpp']).max() > 1e-2 * np.abs(r['Hpp']).max()          # the elimination matters


# ------------------------------------------------------------------------------------------------ 2. gradient against central differences
@pytest.mark.parametrize('kernel', [None, robust.Cauchy(1.0)], ids=['none', 'cauchy'])
def test_full_gradient_matches_central_differences(kernel):
    """2 [g_p; g_d] = d cost / d [xi; rho] of the joint cost, in the six pose directions and for single pixels' rho (interior and
    border).  As section 3.23's gradient test: the quotient D(h) is held to |D(2h) - D(h)| (three times its Richardson truncation
    estimate) plus its rounding, 64 eps cost / h, a bound asserted below 1e-4 of the largest gradient entry of its block; the valid
    set is the same over the stencil (asserted)."""
    sc = noisy_prior(make_scene(1, 24, 40, seed=3, noise=0.3, intr0=(40.0, 40.0, 19.5, 11.5), low_depth=False, flow_dtype=np.float64), seed=2)
    start = right_perturb(sc['motion'][0], [0.01, -0.02, 0.015, 0.004, -0.003, 0.005])
    w = PRIOR_W
    rng = np.random.default_rng(6)
    rho = (1.0 / sc['depth'][0].astype(np.float64)) * (1.0 + 0.02 * rng.standard_normal((24, 40)))
    ev = lambda X, rh: ba_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], X, MOUNT, sc['intr'][0], w, rh, kernel)
    ref = ev(start, rho)
    assert ref['count'] > 800 and np.linalg.norm(ref['gp']) > 1.0
    eps = np.finfo(np.float64).eps

    def check(name, move, h, want, scale):
        D = []
        for step in (h, 2 * h):
            p, m = ev(*move(step)), ev(*move(-step))
            assert np.array_equal(p['valid'], ref['valid']) and np.array_equal(m['valid'], ref['valid'])
            D.append((p['cost'] - m['cost']) / (2 * step))
        tol = abs(D[1] - D[0]) + 64 * eps * ref['cost'] / h
        print('%s: D(h) %.12e  2g %.12e  diff %.3e  tol %.3e' % (name, D[0], 2 * want, abs(D[0] - 2 * want), tol))
        assert abs(D[0] - 2 * want) <= tol
        assert tol < 1e-4 * scale

    for k in range(6):
        e = np.zeros(6)
        e[k] = 1.0
        check('pose %d' % k, lambda s, e=e: (right_perturb(start, s * e), rho), 1e-4, ref['gp'][k], np.abs(2 * ref['gp']).max())
    valid = ref['valid']
    pixels = [(12, 20), (5, 31), (0, 0), (23, 39), (0, 17), (11, 0)]
    pixels = [p for p in pixels if valid[p]]
    assert len(pixels) >= 4 and any(p[0] in (0, 23) or p[1] in (0, 39) for p in pixels)
    gscale = np.abs(2 * ref['gd'][valid]).max()
    for p in pixels:
        def move(s, p=p):
            rh = rho.copy()
            rh[p] += s
            return start, rh
        check('rho %s' % (p,), move, 2e-5, ref['gd'][p], gscale)
    assert np.abs(ref['gd'][valid]).min() > 0


# ------------------------------------------------------------------------------------------------ 3. the two limits
@pytest.mark.parametrize('H,W,seed', [(7, 9, 107), (24, 40, 124)])
def test_marginalised_information_lies_below_H_and_tends_to_it(H, W, seed):
    """H - S is positive semi-definite (H: section 3.23's restatement at the same pose, on the same depth map), its smallest eigenvalue
    held to minus the rounding bound of the sums, 6 x 2^-52 (K + n) max(Habs + Sabs); S -> H for w = 1e300 to that bound entry by
    entry.  (At rho = rho0 the two restatements differ by 1/(1/z) against z, one more rounding per term.)"""
    sc = noisy_prior(make_scene(1, H, W, seed=seed, noise=0.3), seed=3)
    start = right_perturb(sc['motion'][0], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    args = (sc['depth'][0], sc['flow'][0], sc['mask'][0], start, MOUNT, sc['intr'][0])
    h = reproj_reference_link(*args, kernel=robust.Huber(1.0))
    for w in (PRIOR_W, 1.0):
        r = ba_reference_link(*args, w, None, robust.Huber(1.0))
        assert r['count'] == h['count'] > 20
        bound = U * (K_ROUND + r['count']) * (h['Habs'] + r['Sabs'])
        ev = np.linalg.eigvalsh(h['H'] - r['S'])
        print('%dx%d w %.0f: eig(H - S) %.3e .. %.3e, bound %.3e; S/H diagonal %s' % (H, W, w, ev[0], ev[-1], 6 * bound.max(), np.diag(r['S']) / np.diag(h['H'])))
        assert ev[0] >= -6 * bound.max()
        assert ev[-1] > 1e3 * 6 * bound.max()                  # ... and the difference is not rounding
        assert np.linalg.eigvalsh(r['S'])[0] > 0
    r = ba_reference_link(*args, 1e300, None, robust.Huber(1.0))
    bound = U * (K_ROUND + r['count']) * (h['Habs'] + r['Sabs'])
    assert (np.abs(r['S'] - h['H']) <= bound).all() and (np.abs(r['g'] - h['g']) <= U * (K_ROUND + r['count']) * (h['gabs'] + r['gabs'])).all()


# ------------------------------------------------------------------------------------------------ 4. the planted scene
@pytest.mark.parametrize('H,W', [(24, 40), (72, 96)])
def test_joint_refinement_beats_pose_only_on_the_planted_scene(H, W):
    """sigma_rho = 0.02 /m, 0.3 px of flow noise, start 0.08 away, 20 evaluations (seed 0 settles at both sizes): the restatement's joint
    pose is strictly closer to the truth than its pose-only pose, and its inverse-depth RMS error strictly below the prior's.
    Measured here: 24 x 40 pose-only 9.41e-3, joint 7.89e-3 (1.2 x), rho RMS 2.000e-2 -> 1.906e-2, last step 5.5e-10;
    72 x 96 pose-only 1.561e-2, joint 1.43e-3 (11.0 x), rho RMS 1.995e-2 -> 1.601e-2, last step 5.0e-10."""
    sc, w, ref, pose_only = planted_case(H, W)
    r = ref['sums']
    truth = sc['motion'][0]
    e_pose, e_joint = pose_dist(truth, pose_only['motion']), pose_dist(truth, r['motion'])
    d = lie.se3_log(lie.se3_mul(lie.se3_inv(truth), r['motion']))
    rho0 = 1.0 / sc['depth'][0].astype(np.float64)
    rms = lambda x: float(np.sqrt(np.mean((x - sc['rho_true'][0]) ** 2)))
    print('%dx%d: pose-only %.3e, joint %.3e (transl. %.2e / rot. %.2e), %.1f x; rho RMS %.3e -> %.3e; last step %.1e, accepted %d rejected %d' % (
        H, W, e_pose, e_joint, np.linalg.norm(d[:3]), np.linalg.norm(d[3:]), e_pose / e_joint, rms(rho0), rms(r['rho']), r['last_step'],
        r['accepted'], r['rejected']))
    assert r['status'] == OK and pose_only['status'] == OK and r['accepted'] + r['rejected'] == 19
    assert e_joint < e_pose
    assert rms(r['rho']) < rms(rho0)


# ------------------------------------------------------------------------------------------------ 5. host-side checks
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    from islam_amd import _lib
    assert _lib.DENSE_REPROJ_BADPRIOR == BADPRIOR
    one = 1        # any non-NULL address: a refused call never reads it
    assert lib.islam_dense_ba_scratch_bytes(0, 4, 4, 0) == 0
    b0, b1 = lib.islam_dense_ba_scratch_bytes(3, 5, 7, 0), lib.islam_dense_ba_scratch_bytes(3, 5, 7, 20)
    assert b0 >= 8 * 3 * _lib.DENSE_REPROJ_NBLK * _lib.DENSE_REPROJ_NSUM and b1 >= b0 + 8 * 3 * (7 + 6) + 4 * 3 + 2 * 8 * 3 * 5 * 7

    def normal(B=1, H=2, W=2, kind=0, delta=1.0, depth=one, out=one, scratch=one, prior=one):
        return lib.islam_dense_ba_normal(depth, one, None, one, None, one, prior, None, kind, delta, out, one, one, one, one, one, scratch, B, H, W, None)

    def refine(B=1, H=2, W=2, kind=0, delta=1.0, iters=3, status=one, trace=None, cap=0, damping=1e-4, prior=one, rho=one):
        return lib.islam_dense_ba_refine(one, one, None, one, None, one, prior, kind, delta, iters, damping, 16.0, one, rho, one, one, one, one, one,
                                         one, one, one, one, status, trace, cap, one, B, H, W, None)

    for call, name in ((normal, b'islam_dense_ba_normal'), (refine, b'islam_dense_ba_refine')):
        for kw, what in ((dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
                         (dict(kind=3), b'robust kind'), (dict(kind=-1), b'robust kind'), (dict(kind=1, delta=0.0), b'delta'),
                         (dict(delta=-2.0), b'delta'), (dict(delta=float('nan')), b'delta'), (dict(prior=None), b'prior_weight')):
            assert call(**kw) == -1, kw
            msg = lib.islam_last_error()
            assert name in msg and what in msg, (kw, msg)
    for kw in (dict(depth=None), dict(out=None), dict(scratch=None)):
        assert normal(**kw) == -1 and b'islam_dense_ba_normal: NULL' in lib.islam_last_error()
    for kw, what in ((dict(iters=0), b'iters'), (dict(iters=-4), b'iters'), (dict(status=None), b'NULL'), (dict(cap=4), b'trace'),
                     (dict(damping=-1.0), b'damping'), (dict(rho=None), b'out_inv_depth')):
        assert refine(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_dense_ba_refine' in msg and what in msg, (kw, msg)


def _cpu_loss(sc):
    from islam_amd import lietensor as pp
    from islam_amd.dense_ba import DenseReprojectionLoss
    fx, fy, cx, cy = sc['intr'][0]
    return DenseReprojectionLoss(torch.from_numpy(sc['depth']), torch.from_numpy(sc['flow']), fx, fy, cx, cy, torch.from_numpy(sc['mask']),
                                 pp.SE3(torch.from_numpy(MOUNT)), device='cpu')


def test_ops_refuse_cpu_tensors():
    from islam_amd import ops
    sc = make_scene(2, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (t(sc['depth']), t(sc['flow']), t(sc['mask']), t(sc['motion']), t(sc['intr']))
    with pytest.raises(RuntimeError):
        ops.dense_ba_normal(*args, 2500.0)
    with pytest.raises(RuntimeError):
        ops.dense_ba_refine(*args, 2500.0, iters=3)
    with pytest.raises(RuntimeError):
        _cpu_loss(sc).refine_joint(t(sc['motion']), 0.02)


def test_python_argument_errors():
    from islam_amd.dense_ba import DenseReprojectionLoss
    sc = make_scene(2, 7, 9, seed=1)
    loss, motion = _cpu_loss(sc), torch.from_numpy(sc['motion'])
    for bad in (0.0, -0.02, float('nan'), float('inf'), torch.tensor([0.02, 0.0]), torch.tensor([0.02, 0.02, 0.02]), torch.ones(2, 2)):
        with pytest.raises(ValueError, match='sigma_inv_depth'):
            loss.refine_joint(motion, bad)
        with pytest.raises(ValueError, match='sigma_inv_depth'):
            loss.information(motion, sigma_inv_depth=bad)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='sigma_px'):
            loss.refine_joint(motion, 0.02, sigma_px=bad)
        with pytest.raises(ValueError, match='sigma_px'):
            loss.information(motion, sigma_px=bad, sigma_inv_depth=0.02)
    with pytest.raises(ValueError, match='2 motions|motions for'):
        loss.refine_joint(motion[:1], 0.02)
    assert DenseReprojectionLoss.sigma_inv_depth_from_disparity(0.5, 320.0, 0.25) == 0.5 / (320.0 * 0.25)
    for bad in ((0.0, 320.0, 0.25), (0.5, -1.0, 0.25), (0.5, 320.0, 0.0)):
        with pytest.raises(ValueError):
            DenseReprojectionLoss.sigma_inv_depth_from_disparity(*bad)


def test_information_takes_the_old_path_without_a_depth_sigma(monkeypatch):
    """information(sigma_inv_depth=None) calls ops.dense_reproj_normal and nothing of the joint path; with a value it calls
    ops.dense_ba_normal with w = (sigma_px / sigma_inv_depth)^2 and returns S / sigma_px^2."""
    from islam_amd import ops
    sc = make_scene(2, 7, 9, seed=1)
    loss, motion = _cpu_loss(sc), torch.from_numpy(sc['motion'])
    Hm = torch.arange(72, dtype=torch.float64).reshape(2, 6, 6)
    cost, count = torch.tensor([30.0, 50.0], dtype=torch.float64), torch.tensor([13.0, 28.0], dtype=torch.float64)
    calls = []

    def old(depth, flow, mask, mo, intr, rgb2imu=None, kernel=None):
        calls.append(('old', kernel))
        return ops.DenseReprojNormal(Hm, None, cost, None, count, None)

    def new(depth, flow, mask, mo, intr, w, inv_depth=None, rgb2imu=None, kernel=None):
        calls.append(('new', w, inv_depth, kernel))
        return ops.DenseBANormal(2 * Hm, None, 3 * cost, None, count, None)

    monkeypatch.setattr(ops, 'dense_reproj_normal', old)
    monkeypatch.setattr(ops, 'dense_ba_normal', new)
    assert torch.equal(loss.information(motion, sigma_px=0.5), Hm / 0.25) and torch.equal(loss.information(motion, 0.5, None, None), Hm / 0.25)
    assert torch.equal(loss.information(motion, sigma_px='residual'), Hm / (cost / (2 * count - 6)).view(-1, 1, 1))
    assert [c[0] for c in calls] == ['old'] * 3
    del calls[:]
    kern = robust.Huber(1.0)
    assert torch.equal(loss.information(motion, sigma_px=0.5, kernel=kern, sigma_inv_depth=0.02), 2 * Hm / 0.25)
    assert calls == [('new', (0.5 / 0.02) ** 2, None, kern)]
    del calls[:]
    got = loss.information(motion, sigma_px='residual', sigma_inv_depth=torch.tensor([0.02, 0.04], dtype=torch.float64))
    assert torch.equal(got, 2 * Hm / (3 * cost / (2 * count - 6)).view(-1, 1, 1))
    assert calls[0][0] == 'new' and torch.equal(calls[0][1], (1.0 / torch.tensor([0.02, 0.04], dtype=torch.float64)) ** 2)


def test_dense_ba_kernels_do_not_spill(lib):
    """Thirty fp64 accumulators, two poses and the per-pixel Schur terms: none of the new kernels may have a private segment or a
    spilled VGPR."""
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = {n: blk for n, blk in _kernels().items() if 'dense_ba' in n}
    assert len(ks) == 3 and all(any(want in n for n in ks) for want in ('dense_ba_partial_kernel', 'dense_ba_final_kernel', 'dense_ba_gather_kernel'))
    for n, blk in ks.items():
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, n
