"""Joint (pose, inverse depth) dense bundle adjustment (include/islam_hip.h, islam_dense_ba_normal / _refine):
everything about the float64 numpy restatement of the per-pixel Schur sums and of the joint Levenberg-Marquardt (ba_reference_link and
ba_refine_reference_link in tests/dense_reproj_f64.py) that can be checked without a GPU -- the Schur complement against the explicitly
assembled dense system, the full gradient against central differences, the two limits (H - S >= 0, S -> H), the planted refinement --
and the host-side argument errors.  (The kernels' register metadata: tests/test_dense_reproj_cpu.py.)"""
import math

import numpy as np
import pytest
import torch

from islam_amd import robust
from oracle import lie
from tests.dense_reproj_f64 import (BADPRIOR, K_ROUND, MOUNT, OK, PRIOR_W, U, ba_reference_link, make_scene, noisy_prior, planted_case, pose_dist,
                                    reproj_reference_link, right_perturb)


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
    assert _lib.DENSE_REPROJ_BADPRIOR == BADPRIOR == 3
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

