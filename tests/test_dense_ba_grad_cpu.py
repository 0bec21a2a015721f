"""The gradient of the joint (pose, inverse depth) refinement in depth and flow (include/islam_hip.h, islam_dense_ba_ift_weights and
islam_dense_ba_vjp): everything about the float64 numpy restatement the GPU tests compare against
(tests/dense_ba_grad_f64.py) that can be checked without a GPU -- the gradient of Phi = lambda^T G against central differences, the
per-pixel elimination against a dense solve of the explicitly assembled system, the implicit gradient against refining again on moved
data (exact in a zero-residual scene, its Gauss-Newton error measured in a noisy one), the status rule -- and the host side: argument
errors, the three kernels' register metadata, and refine_joint's differentiable= switch."""
import inspect
import os

import numpy as np
import pytest
import torch

from islam_amd import robust
from tests.dense_ba_grad_f64 import (ba_adjoint_reference_link, ba_implicit_gradient, ba_implicit_gradient_batch, ba_phi,
                                     ba_vjp_reference_link)
from tests.dense_reproj_f64 import (MOUNT, OK, PRIOR_W, ba_reference_link, ba_refine_reference_link, link_front, make_scene, noisy_prior,
                                    planted_case, planted_scene, right_perturb, tangent_from_pose_grad)
from tests.test_dense_ba_joint_cpu import _dense_system

EPS = np.finfo(np.float64).eps
START = [0.01, -0.008, 0.012, 0.006, -0.005, 0.007]


# ------------------------------------------------------------------------------------------------ 1. Phi against central differences
KERNELS = {'none': (None, 0.3, 1e-3), 'cauchy': (robust.Cauchy(1.0), 0.3, 1e-3), 'huber': (robust.Huber(1.0), 0.7, 1e-5)}      # kernel, flow noise, step


def _small_scene(noise):
    """7 x 9 with the mount, the user mask and every clause active, float64 flow and depth, and an inverse-depth state 3 % off the prior."""
    sc = noisy_prior(make_scene(1, 7, 9, seed=107, noise=noise, low_depth=False, flow_dtype=np.float64), seed=1)
    sc['depth'] = sc['depth'].astype(np.float64)
    sc['start'] = right_perturb(sc['motion'][0], START)
    sc['rho'] = (1.0 / sc['depth'][0]) * (1.0 + 0.03 * np.random.default_rng(4).standard_normal((7, 9)))
    return sc


@pytest.mark.parametrize('kind', list(KERNELS))
def test_gradient_of_phi_matches_central_differences(kind):
    """dPhi along a direction in depth or flow, Phi = lam_p^T g_p + sum lam_d g_d from ba_reference_link's gradient blocks at a fixed
    state and a fixed lambda (the adjoint of a random v), against the restatement's gradient dotted with the direction: dense random
    directions in flow and in depth, and single pixels (an interior and a border one, both valid: both flow components and the depth;
    one the user mask drops: the depth, the only thing of it Phi sees).  As section 3.24's test: the quotient D(h) is held to
    |D(2h) - D(h)| (three times its Richardson truncation estimate) plus its rounding, 64 eps sum|term of Phi| / h, a bound asserted
    below 1e-4 of the value; the valid set, and under Huber the branch of every pixel, is the same over the stencil (asserted)."""
    kernel, noise, h = KERNELS[kind]
    sc = _small_scene(noise)
    z0, f0, mask, intr, w = sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['intr'][0], PRIOR_W
    rng = np.random.default_rng(12)
    v_p, v_d = rng.standard_normal(6), rng.standard_normal((7, 9))
    adj = ba_adjoint_reference_link(z0, f0, mask, sc['start'], MOUNT, intr, w, sc['rho'], v_p, v_d, kernel)
    ref = ba_vjp_reference_link(z0, f0, mask, sc['start'], MOUNT, intr, w, sc['rho'], adj['lam_p'], v_d, kernel)
    assert np.array_equal(ref['lam_d'], adj['lam_d']) and ref['prior'].all()
    valid = ref['valid']
    assert 2 * valid.sum() >= 63 and not mask.all()
    if kind == 'huber':
        d2 = kernel.delta ** 2
        beyond = int((ref['s'][valid] > d2).sum())
        print('huber: %d of %d pixels beyond delta' % (beyond, valid.sum()))
        assert 0 < beyond < valid.sum()
    zero_z, zero_f = np.zeros((7, 9)), np.zeros((2, 7, 9))
    dirs = [('dense flow', zero_z, rng.standard_normal((2, 7, 9))), ('dense depth', rng.standard_normal((7, 9)), zero_f)]
    interior = next((y, x) for y in (3, 2, 4) for x in (4, 3, 5) if valid[y, x])
    border = next((y, x) for y in range(7) for x in range(9) if valid[y, x] and (y in (0, 6) or x in (0, 8)))
    masked = next((y, x) for y in range(7) for x in range(9) if not mask[y, x])
    assert not valid[masked]
    for name, (y, x) in (('interior', interior), ('border', border), ('masked', masked)):
        dz = zero_z.copy()
        dz[y, x] = 1.0
        dirs.append(('%s pixel (%d,%d) depth' % (name, y, x), dz, zero_f))
        for k in range(2 if name != 'masked' else 0):
            df = zero_f.copy()
            df[k, y, x] = 1.0
            dirs.append(('%s pixel (%d,%d) flow %d' % (name, y, x, k), zero_z, df))
    assert not ref['grad_flow'][:, masked[0], masked[1]].any()
    phi = lambda z, f: ba_phi(z, f, mask, sc['start'], MOUNT, intr, w, sc['rho'], adj['lam_p'], adj['lam_d'], kernel)
    for name, dz, df in dirs:
        want = float((ref['grad_depth'] * dz).sum() + (ref['grad_flow'] * df).sum())
        D, mag = [], 0.0
        for step in (h, 2 * h):
            vals = []
            for sign in (1.0, -1.0):
                val, mag, vset, s = phi(z0 + sign * step * dz, f0 + sign * step * df)
                assert np.array_equal(vset, valid)
                if kind == 'huber':
                    assert np.array_equal(s[valid] > d2, ref['s'][valid] > d2) and np.abs(s[valid] / d2 - 1.0).min() > 1e-6
                vals.append(val)
            D.append((vals[0] - vals[1]) / (2 * step))
        tol = abs(D[1] - D[0]) + 64 * EPS * mag / h
        print('%-7s %-30s D(h) %.12e  grad %.12e  diff %.3e  tol %.3e' % (kind, name, D[0], want, abs(D[0] - want), tol))
        assert abs(D[0] - want) <= tol
        assert tol < 1e-4 * abs(want)


# ------------------------------------------------------------------------------------------------ 2. the elimination
def test_elimination_matches_a_dense_solve_of_the_full_system():
    """The scene of section 3.25's test (1) (7 x 9, the mount, a user mask, every clause dropping pixels, a perturbed rho, Cauchy(1.0),
    w = 1): [lam_p; lam_d] from the per-pixel elimination against -H_full^-1 v with the explicitly assembled (6 + 63) x (6 + 63)
    Gauss-Newton matrix of that test and a random v = [v_p; v_d].  Bound: 64 eps cond |value|, cond the condition number of the dense
    matrix (asserted below 1e9) and |value| the largest entry of the solution."""
    sc = noisy_prior(make_scene(1, 7, 9, seed=107, noise=0.3), seed=1)
    start = right_perturb(sc['motion'][0], START)
    w = 1.0
    rho = (1.0 / sc['depth'][0].astype(np.float64)) * (1.0 + 0.03 * np.random.default_rng(4).standard_normal((7, 9)))
    args = (sc['depth'][0], sc['flow'][0], sc['mask'][0], start, MOUNT, sc['intr'][0], w, rho)
    r = ba_reference_link(*args, robust.Cauchy(1.0))
    Mx, _ = _dense_system(r, w)
    assert Mx.shape == (69, 69) and r['prior'].all() and 0 < r['count'] < 63
    v = np.random.default_rng(21).standard_normal(69)
    want = -np.linalg.solve(Mx, v)
    adj = ba_adjoint_reference_link(*args, v[:6], v[6:].reshape(7, 9), robust.Cauchy(1.0))
    got = np.concatenate([adj['lam_p'], adj['lam_d'].ravel()])
    cond = np.linalg.cond(Mx)
    err = np.abs(got - want).max() / np.abs(want).max()
    print('cond %.3e, bound %.3e; relative error of [lam_p; lam_d] %.3e (pose block %.3e)' % (
        cond, 64 * EPS * cond, err, np.abs(got[:6] - want[:6]).max() / np.abs(want[:6]).max()))
    assert cond < 1e9
    assert err <= 64 * EPS * cond
    assert np.abs(adj['u_cam']).max() > 0 and np.abs(adj['lam_d'][~r['valid']] + v[6:].reshape(7, 9)[~r['valid']] / w).max() <= 4 * EPS * np.abs(v).max()


# ------------------------------------------------------------------------------------------------ 3. the implicit gradient, exact case
REFINE_AGAIN = 8          # evaluations of a re-refinement from T* (see test_implicit_gradient_matches_refining_again)


def _exact_scene():
    """planted_scene without flow noise and without prior noise, its float32 depth taken as the truth and the flow recomputed from it in
    float64: r = 0 and rho* = rho0 at the optimum, so the Gauss-Newton matrix is the exact Hessian there."""
    sc = planted_scene(24, 40, 0, sigma_rho=0.0, noise=0.0)
    z = sc['depth'][0].astype(np.float64)
    f = link_front(z, np.zeros((2, 24, 40)), np.ones((24, 40), bool), sc['motion'][0], None, sc['intr'][0])
    assert f['valid'].all()
    return z, np.stack([f['ru'], f['rv']]), sc['intr'][0], sc['start'][0]


def _smooth(what):
    v, u = np.meshgrid(np.arange(24.0), np.arange(40.0), indexing='ij')
    if what == 'flow':
        return np.zeros((24, 40)), np.stack([np.sin(0.2 * u + 0.1 * v), np.cos(0.15 * v - 0.1 * u)])
    return 0.5 + 0.4 * np.sin(0.15 * u - 0.2 * v), np.zeros((2, 24, 40))


def _refine_quotient(z0, f0, mask, intr, w, star, a, b, dz, df, eps, iters):
    """D(eps), D(2 eps) of L = a . motion + sum b rho* over re-refinements from ``star`` on data moved by +-eps, +-2 eps along (dz, df),
    the largest last step of the four runs, and whether every run kept ``star``'s valid set."""
    D, last = [], 0.0
    for step in (eps, 2 * eps):
        vals = []
        for sign in (1.0, -1.0):
            run = ba_refine_reference_link(z0 + sign * step * dz, f0 + sign * step * df, mask, star['motion'], None, intr, w, iters=iters)
            assert run['status'] == OK and np.array_equal(run['valid'], star['valid'])
            last = max(last, run['last_step'])
            vals.append(float(a @ run['motion']) + float((b * run['rho']).sum()))
        D.append((vals[0] - vals[1]) / (2 * step))
    return D, last


@pytest.mark.parametrize('loss', ['pose', 'depths'])
@pytest.mark.parametrize('what', ['flow', 'depth'])
def test_implicit_gradient_matches_refining_again(what, loss):
    """A zero-residual scene, L = a . motion + sum b_i rho*_i with fixed random a and b ('pose': b = 0, the path that skips the reduction
    of u_cam; 'depths': a = 0): the restatement's implicit gradient dotted with a smooth direction in flow or in depth, against the
    quotient of L over joint re-refinements from T* on data moved by +-eps = 1e-3 along it.  The bound takes section 3.24's form:
    |D(2 eps) - D(eps)| (Richardson) plus 10 x the re-refinement's last step over eps, the step (the larger of |delta| and max |delta
    rho|) weighed with |a| + sum|b|, what a state error of that size can move L by; it is asserted below 1e-3 of the value.  The
    re-refinements take REFINE_AGAIN = 8 evaluations: a run restarts its inverse depths from the moved prior, so it needs a few more
    than section 3.24's six, and with more the rejected trials only raise the damping and the reported last step stops saying how
    far the run stands from its optimum."""
    z0, f0, intr, start = _exact_scene()
    mask, w = np.ones((24, 40), bool), PRIOR_W
    star = ba_refine_reference_link(z0, f0, mask, start, None, intr, w, iters=20)
    at = ba_reference_link(z0, f0, mask, star['motion'], None, intr, w, star['rho'])
    assert star['status'] == OK and at['cost'] < 1e-16 and at['count'] == 960 and np.abs(star['rho'] * z0 - 1).max() < 1e-9
    rng = np.random.default_rng(31)
    a, b = rng.standard_normal(7), rng.standard_normal((24, 40))
    if loss == 'pose':
        b = np.zeros((24, 40))
    else:
        a = np.zeros(7)
    g = ba_implicit_gradient(z0, f0, mask, star['motion'], None, intr, w, star['rho'], a, None if loss == 'pose' else b)
    assert (loss == 'pose') == (not g['u_cam'].any())
    dz, df = _smooth(what)
    want = float((g['grad_depth'] * dz).sum() + (g['grad_flow'] * df).sum())
    eps = 1e-3
    D, last = _refine_quotient(z0, f0, mask, intr, w, star, a, b, dz, df, eps, REFINE_AGAIN)
    tol = abs(D[1] - D[0]) + 10 * last * (np.abs(a).sum() + np.abs(b).sum()) / eps
    print('%s, loss on %s: D(eps) %.12e  predicted %.12e  diff %.3e = %.2e of the value, tol %.3e (last step %.3e)' % (
        what, loss, D[0], want, abs(D[0] - want), abs(D[0] - want) / abs(want), tol, last))
    assert abs(D[0] - want) <= tol
    assert tol < 1e-3 * abs(want)


# ------------------------------------------------------------------------------------------------ 4. tangent conversion and status
def test_status_rule_and_pixels_without_a_prior():
    """Three links: a marked link and a link with an indefinite S get exact zeros and lam_p = 0, and the third link's values are those of
    a call on it alone; lam_p solves S lam_p = -(v_p - A^T u_cam) with v_p the tangent conversion of the gradient on [t, q]; pixels
    without a prior (0, NaN, -1) get a zero depth gradient whatever arrives on them; a masked-out pixel with a prior gets
    dL/ddepth = -v_d / z^2 to rounding (rho* = rho0 = 1/z there) and no flow gradient."""
    sc = noisy_prior(make_scene(3, 7, 9, seed=107, noise=0.3), seed=7)
    no_prior = {(2, 5): 0.0, (3, 1): np.nan, (1, 7): -1.0}
    for p, val in no_prior.items():
        sc['depth'][:, p[0], p[1]] = val
    start = right_perturb(sc['motion'], START)
    w = np.array([PRIOR_W, 400.0, 100.0])
    rng = np.random.default_rng(9)
    with np.errstate(divide='ignore', invalid='ignore'):
        rho0 = 1.0 / sc['depth'].astype(np.float64)
    have = np.isfinite(rho0) & (rho0 > 0)
    rho = np.where(have, rho0 * (1.0 + 0.03 * rng.standard_normal(rho0.shape)), 0.0)
    rho = np.where(sc['mask'], rho, np.where(have, rho0, 0.0))          # a masked-out pixel sits at its prior, as after a refinement
    grad7, v_d = rng.standard_normal((3, 7)), rng.standard_normal((3, 7, 9))
    S = np.stack([ba_reference_link(sc['depth'][b], sc['flow'][b], sc['mask'][b], start[b], MOUNT, sc['intr'][b], w[b], rho[b])['S'] for b in range(3)])
    args = (sc['depth'], sc['flow'], sc['mask'], start, MOUNT, sc['intr'], w, rho, grad7, v_d)
    healthy, st = ba_implicit_gradient_batch(*args, S)
    assert st.tolist() == [0, 0, 0]
    bad = S.copy()
    bad[1, 2, 2] = -bad[1, 2, 2]
    for name, out in (('marked', ba_implicit_gradient_batch(*args, S, status=[0, 1, 0])), ('indefinite', ba_implicit_gradient_batch(*args, bad)),
                      ('bad prior', ba_implicit_gradient_batch(*args[:6], np.array([PRIOR_W, 0.0, 100.0]), *args[7:], S))):
        res, status = out
        assert status.tolist() == [0, dict(marked=1, indefinite=2)[name] if name != 'bad prior' else 3, 0], name
        assert not res[1]['grad_depth'].any() and not res[1]['grad_flow'].any() and not res[1]['lam_p'].any(), name
        for b in (0, 2):
            assert np.array_equal(res[b]['grad_depth'], healthy[b]['grad_depth']) and np.array_equal(res[b]['grad_flow'], healthy[b]['grad_flow']), name
    for b, g in enumerate(healthy):
        v_p = tangent_from_pose_grad(start[b], grad7[b])
        res = g['S'] @ g['lam_p'] + v_p - g['A'].T @ g['u_cam']
        assert np.abs(res).max() <= 64 * EPS * np.linalg.cond(g['S']) * np.abs(v_p).max()
        assert g['grad_depth'].any() and g['grad_flow'].any()
        for p in no_prior:
            assert g['grad_depth'][p] == 0 and not g['grad_flow'][:, p[0], p[1]].any() and not g['prior'][p]
        out = ~sc['mask'][b] & g['prior']
        assert out.any() and not g['valid'][out].any() and not g['grad_flow'][:, out].any()
        z = sc['depth'][b].astype(np.float64)[out]
        want = -v_d[b][out] / z ** 2
        assert np.abs(g['grad_depth'][out] - want).max() <= 8 * EPS * np.abs(want).max()


# ------------------------------------------------------------------------------------------------ 5. the Gauss-Newton error, measured
GN_DEVIATION = {}


@pytest.mark.parametrize('H,W', [(24, 40), (72, 96)])
def test_gauss_newton_error_on_the_noisy_planted_scene(H, W):
    """Measured, not asserted.  The planted scene of section 3.25 (0.3 px of flow noise, sigma_rho = 0.02 /m): the residuals at the
    optimum are not zero, so H_full differs from the exact Hessian by terms proportional to them.  The relative deviation of the implicit
    gradient from the quotient of L over re-refinements (+-eps = 1e-3 along the smooth flow and depth directions, 12 evaluations each;
    20 evaluations or eps = 1e-4 give the same four digits), for a loss on the pose and for one on the inverse depths.  Measured here
    (|implicit - quotient| / |quotient|), loss on the pose / on the inverse depths:
    24 x 40: flow direction 8.1e-2 / 2.2e-2, depth direction 7.5e-2 / 3.1e-2;  72 x 96: flow 5.1e-2 / 1.9e-1, depth 3.0e-2 / 1.0e-1.
    That is the size the neglected term has per pixel: r . d2r/drho2 = |r| (2/rho) |jd| against h_dd = |jd|^2 + w, about 0.3 x 10 x 7 /
    275 = 8 % at 24 x 40 (fx = 24, |t| = 0.3 m) and 0.3 x 10 x 17 / 525 = 10 % at 72 x 96.  The test asserts only that both sides are
    finite and that the deviation is recorded; a bound, if one is wanted later, is to be taken from these numbers with a stated
    margin."""
    sc, w, ref, _ = planted_case(H, W)
    star = ref['sums']
    z0, f0, mask, intr = sc['depth'][0].astype(np.float64), sc['flow'][0].astype(np.float64), sc['mask'][0], sc['intr'][0]
    rng = np.random.default_rng(31)
    v, u = np.meshgrid(np.arange(float(H)), np.arange(float(W)), indexing='ij')
    dirs = {'flow': (np.zeros((H, W)), np.stack([np.sin(0.2 * u + 0.1 * v), np.cos(0.15 * v - 0.1 * u)])),
            'depth': (0.5 + 0.4 * np.sin(0.15 * u - 0.2 * v), np.zeros((2, H, W)))}
    for loss in ('pose', 'depths'):
        a = rng.standard_normal(7) if loss == 'pose' else np.zeros(7)
        b = np.zeros((H, W)) if loss == 'pose' else rng.standard_normal((H, W))
        g = ba_implicit_gradient(z0, f0, mask, star['motion'], None, intr, w, star['rho'], a, None if loss == 'pose' else b)
        for what, (dz, df) in dirs.items():
            want = float((g['grad_depth'] * dz).sum() + (g['grad_flow'] * df).sum())
            D, last = _refine_quotient(z0, f0, mask, intr, w, star, a, b, dz, df, 1e-3, 12)
            dev = abs(want - D[0]) / abs(D[0])
            GN_DEVIATION[(H, W, what, loss)] = dev
            print('%dx%d %s, loss on %s: implicit %.9e  quotient %.9e (Richardson %.1e, last step %.1e)  relative deviation %.3e' % (
                H, W, what, loss, want, D[0], abs(D[1] - D[0]), last, dev))
            assert np.isfinite(want) and np.isfinite(D[0]) and np.isfinite(dev)
    assert len([k for k in GN_DEVIATION if k[:2] == (H, W)]) == 4


# ------------------------------------------------------------------------------------------------ 6. host-side checks
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'islam_hip.h')).read()
    for name in ('islam_dense_ba_adjoint_scratch_bytes', 'islam_dense_ba_ift_weights', 'islam_dense_ba_vjp'):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None and name in header
    assert callable(ops.dense_ba_ift_weights) and callable(ops.dense_ba_vjp) and issubclass(ops._DenseBARefine, torch.autograd.Function)
    assert lib.islam_abi_version() == 1


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    from islam_amd import _lib
    one = 1        # any non-NULL address: a refused call never reads it
    assert lib.islam_dense_ba_adjoint_scratch_bytes(0) == 0 and lib.islam_dense_ba_adjoint_scratch_bytes(-2) == 0
    assert lib.islam_dense_ba_adjoint_scratch_bytes(3) >= 8 * 3 * _lib.DENSE_REPROJ_NBLK * 6

    def ift(B=1, H=2, W=2, kind=0, delta=1.0, depth=one, flow=one, motion=one, intr=one, prior=one, rho=one, S=one, grad=one, scratch=one,
            lam=one, status=one):
        return lib.islam_dense_ba_ift_weights(depth, flow, None, motion, None, intr, prior, rho, kind, delta, S, grad, None, None, scratch, B, H, W,
                                              lam, status, None)

    def vjp(B=1, H=2, W=2, kind=0, delta=1.0, depth=one, flow=one, motion=one, intr=one, prior=one, rho=one, lam=one, gd=one, gf=one):
        return lib.islam_dense_ba_vjp(depth, flow, None, motion, None, intr, prior, rho, kind, delta, lam, None, None, gd, gf, B, H, W, None)

    common = ((dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
              (dict(kind=3), b'robust kind'), (dict(kind=-1), b'robust kind'), (dict(kind=1, delta=0.0), b'delta'), (dict(delta=-2.0), b'delta'),
              (dict(delta=float('nan')), b'delta'), (dict(depth=None), b'NULL'), (dict(flow=None), b'NULL'), (dict(motion=None), b'NULL'),
              (dict(intr=None), b'NULL'), (dict(prior=None), b'prior_weight'), (dict(rho=None), b'inv_depth'), (dict(lam=None), b'lambda_p'))
    for call, name, more in ((ift, b'islam_dense_ba_ift_weights', ((dict(S=None), b'NULL'), (dict(grad=None), b'grad_motion'),
                                                                  (dict(scratch=None), b'scratch'), (dict(status=None), b'status_out'))),
                             (vjp, b'islam_dense_ba_vjp', ((dict(gd=None), b'grad_depth'), (dict(gf=None), b'grad_flow')))):
        for kw, what in common + more:
            assert call(**kw) == -1, (name, kw)
            msg = lib.islam_last_error()
            assert name in msg and what in msg, (kw, msg)


def _cpu_loss(sc, leaf=False):
    from islam_amd import lietensor as pp
    from islam_amd.dense_ba import DenseReprojectionLoss
    fx, fy, cx, cy = sc['intr'][0]
    depth, flow = torch.from_numpy(sc['depth']).requires_grad_(leaf), torch.from_numpy(sc['flow']).requires_grad_(leaf)
    return DenseReprojectionLoss(depth, flow, fx, fy, cx, cy, torch.from_numpy(sc['mask']), pp.SE3(torch.from_numpy(MOUNT)), device='cpu')


def test_ops_refuse_cpu_tensors():
    from islam_amd import ops
    sc = make_scene(2, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (t(sc['depth']), t(sc['flow']), t(sc['mask']), t(sc['motion']), t(sc['intr']), 225.0, torch.ones(2, 7, 9, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.dense_ba_ift_weights(*args, torch.eye(6, dtype=torch.float64).expand(2, 6, 6), torch.zeros(2, 7, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.dense_ba_vjp(*args, torch.zeros(2, 6, dtype=torch.float64))
    loss = _cpu_loss(sc, leaf=True)
    assert loss.z.requires_grad and loss.flow.requires_grad          # the stored tensors keep their graph
    with pytest.raises(RuntimeError):
        loss.refine_joint(t(sc['motion']), 0.02, differentiable=True)


def test_new_kernels_do_not_spill(lib):
    """The three kernels of section 3.26 are in the library, once each, without a private segment and without a spilled VGPR."""
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = _kernels()
    for want in ('joint_adj_partial_kernel', 'joint_adj_solve_kernel', 'joint_adj_vjp_kernel'):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        blk = ks[found[0]]
        print('%s: %d VGPRs, %d SGPRs, %d B of LDS' % (want, _field(blk, 'vgpr_count'), _field(blk, 'sgpr_count'), _field(blk, 'group_segment_fixed_size')))
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, want


def test_refine_joint_switch(monkeypatch):
    """refine_joint accepts differentiable=; with False (the default) it makes today's one ops call, ops.dense_ba_refine with today's
    arguments, and nothing of the differentiable path; with True it goes through ops._DenseBARefine.apply with the stored tensors."""
    from islam_amd import ops
    from islam_amd.dense_ba import DenseReprojectionLoss
    assert inspect.signature(DenseReprojectionLoss.refine_joint).parameters['differentiable'].default is False
    sc = make_scene(2, 7, 9, seed=1)
    loss, motion = _cpu_loss(sc), torch.from_numpy(sc['motion'])
    rho = torch.full((2, 7, 9), 0.25, dtype=torch.float64)
    rho[0, 0, 0] = 0.0
    fields = [motion, rho] + [None] * 11
    calls = []

    def plain(depth, flow, mask, mo, intr, w, rgb2imu=None, kernel=None, iters=20, damping=1e-4, min_count=16, trace_cap=0):
        calls.append(('plain', depth, flow, mask, w, rgb2imu, kernel, iters, damping, min_count, trace_cap))
        return ops.DenseBARefined(*fields)

    class Fn:
        @staticmethod
        def apply(*a):
            calls.append(('fn',) + a)
            return tuple(fields)

    monkeypatch.setattr(ops, 'dense_ba_refine', plain)
    monkeypatch.setattr(ops, '_DenseBARefine', Fn)
    for name in ('dense_ba_ift_weights', 'dense_ba_vjp'):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail('the default path must not touch the gradient ops'))
    kern = robust.Huber(1.0)
    for kw in ({}, dict(differentiable=False)):
        out = loss.refine_joint(motion, 0.02, sigma_px=0.5, iters=7, kernel=kern, damping=1e-3, min_count=5, trace_cap=2, **kw)
        assert len(calls) == 1 and calls[0][0] == 'plain'
        _, depth, flow, mask, w, mount, kernel, iters, damping, min_count, trace_cap = calls.pop()
        assert depth is loss.z and flow is loss.flow and mask is loss.mask and mount is loss.rgb2imu_pose and kernel is kern
        assert (w, iters, damping, min_count, trace_cap) == ((0.5 / 0.02) ** 2, 7, 1e-3, 5, 2)
        assert out.depth[0, 0, 0] == loss.z[0, 0, 0] and out.depth[1, 2, 3] == 4.0 and out.depth.dtype == loss.z.dtype
    out = loss.refine_joint(motion, 0.02, sigma_px=0.5, iters=7, kernel=kern, differentiable=True)
    assert len(calls) == 1 and calls[0][0] == 'fn' and calls[0][1] is loss.z and calls[0][2] is loss.flow and calls[0][6] == (0.5 / 0.02) ** 2
    assert calls[0][8] is kern and calls[0][9] == 7 and out.depth[1, 2, 3] == 4.0
