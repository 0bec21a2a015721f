"""The gradient of the refined dense-reprojection pose in depth and flow (include/islam_hip.h, islam_dense_reproj_vjp and
islam_dense_reproj_ift_weights): everything about the float64 numpy restatement the GPU tests compare against
(vjp_reference_link in tests/dense_reproj_f64.py) that can be checked without a GPU -- the vector-Jacobian product against central
differences of w^T g, the implicit gradient against re-refining on perturbed data, the conversion of a gradient on [t, q] to the
right tangent -- and the host-side argument errors.  (The kernels' register metadata: tests/test_dense_reproj_cpu.py.)"""
import os

import numpy as np
import pytest
import torch

from islam_amd import robust
from oracle import lie
from tests.dense_reproj_f64 import make_scene, refine_reference_link, reproj_reference_link, right_perturb, tangent_from_pose_grad, vjp_reference_link

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ the VJP against central differences
W_TEST = np.array([0.7, -0.4, 0.9, -1.3, 0.8, 0.5])
KERNELS = {'none': (None, 0.3, 1e-3), 'cauchy': (robust.Cauchy(1.0), 0.3, 1e-3), 'huber': (robust.Huber(1.0), 0.7, 1e-5)}      # kernel, flow noise, step


def _smooth_scene(noise):
    """The scene of test_gradient_matches_central_differences: 24 x 40, float64 flow, every pixel well inside the clauses."""
    sc = make_scene(1, 24, 40, seed=3, noise=noise, intr0=(40.0, 40.0, 19.5, 11.5), low_depth=False, flow_dtype=np.float64)
    sc['depth'] = sc['depth'].astype(np.float64)
    sc['start'] = right_perturb(sc['motion'][0], [0.01, -0.02, 0.015, 0.004, -0.003, 0.005])
    return sc


def _phi(sc, depth, flow, kernel, w=W_TEST):
    r = reproj_reference_link(depth, flow, sc['mask'][0], sc['start'], sc['rgb2imu'], sc['intr'][0], kernel)
    return float(w @ r['g']), float(np.abs(w) @ r['gabs']), r['valid']


def _directions(sc, ref):
    """(name, direction in depth, direction in flow): a dense random one in each, and single pixels (an interior one and one on the
    image border, both valid)."""
    rng = np.random.default_rng(11)
    H, W = ref['valid'].shape
    zero_z, zero_f = np.zeros((H, W)), np.zeros((2, H, W))
    out = [('dense depth', rng.standard_normal((H, W)), zero_f), ('dense flow', zero_z, rng.standard_normal((2, H, W)))]
    border = next((0, x) for x in range(W) if ref['valid'][0, x])
    for name, (y, x) in (('interior', (11, 17)), ('border', border)):
        assert ref['valid'][y, x]
        dz = zero_z.copy()
        dz[y, x] = 1.0
        out.append(('%s pixel (%d,%d) depth' % (name, y, x), dz, zero_f))
        for k in range(2):
            df = zero_f.copy()
            df[k, y, x] = 1.0
            out.append(('%s pixel (%d,%d) flow %d' % (name, y, x, k), zero_z, df))
    return out


@pytest.mark.parametrize('kind', list(KERNELS))
def test_vjp_matches_central_differences(kind):
    """d(w^T g) along a direction in depth or flow: the difference quotient D(h) of w^T g from reproj_reference_link against the
    restatement's gradient dotted with the direction.  D(h) has truncation error (D(2h) - D(h)) / 3 + O(h^4) (Richardson); the check
    holds the difference to three times that estimate plus the quotient's rounding, 64 eps sum|term of w^T g| / h, as
    test_gradient_matches_central_differences does, and the bound is asserted below 1e-4 of the value, so a wrong sign or a missing
    term shows.  The valid set (and under Huber the branch of every pixel) is the same over the stencil (asserted)."""
    kernel, noise, h = KERNELS[kind]
    sc = _smooth_scene(noise)
    z0, f0 = sc['depth'][0], sc['flow'][0]
    ref = vjp_reference_link(z0, f0, sc['mask'][0], sc['start'], sc['rgb2imu'], sc['intr'][0], W_TEST, kernel)
    assert ref['valid'].sum() > 800
    if kind == 'huber':
        d2 = kernel.delta ** 2
        frac = np.mean(ref['s'][ref['valid']] > d2)
        print('huber: %.1f %% of the pixels beyond delta' % (100 * frac))
        assert 0.1 <= frac <= 0.9
    for name, dz, df in _directions(sc, ref):
        want = float((ref['grad_depth'] * dz).sum() + (ref['grad_flow'] * df).sum())
        D, mag = [], 0.0
        for step in (h, 2 * h):
            vals = []
            for sign in (1.0, -1.0):
                phi, mag, valid = _phi(sc, z0 + sign * step * dz, f0 + sign * step * df, kernel)
                assert np.array_equal(valid, ref['valid'])
                if kind == 'huber':
                    s = vjp_reference_link(z0 + sign * step * dz, f0 + sign * step * df, sc['mask'][0], sc['start'], sc['rgb2imu'], sc['intr'][0],
                                           W_TEST, kernel)['s'][valid]
                    assert np.array_equal(s > d2, ref['s'][valid] > d2) and np.abs(s / d2 - 1.0).min() > 1e-6
                vals.append(phi)
            D.append((vals[0] - vals[1]) / (2 * step))
        tol = abs(D[1] - D[0]) + 64 * EPS * mag / h
        print('%-7s %-28s D(h) %.12e  vjp %.12e  diff %.3e  tol %.3e' % (kind, name, D[0], want, abs(D[0] - want), tol))
        assert abs(D[0] - want) <= tol
        assert tol < 1e-4 * abs(want)


def test_dJ_dz_term_is_load_bearing():
    """With 0.3 px of noise the depth gradient without the dq/dz term is off by far more than the tolerance of the test above: the
    term cannot be dropped unnoticed."""
    kernel, noise, h = KERNELS['none']
    sc = _smooth_scene(noise)
    z0, f0 = sc['depth'][0], sc['flow'][0]
    ref = vjp_reference_link(z0, f0, sc['mask'][0], sc['start'], sc['rgb2imu'], sc['intr'][0], W_TEST, kernel)
    name, dz, df = _directions(sc, ref)[0]
    full, without = float((ref['grad_depth'] * dz).sum()), float(((ref['grad_depth'] - ref['depth_dJ']) * dz).sum())
    D = [(_phi(sc, z0 + k * h * dz, f0, kernel)[0] - _phi(sc, z0 - k * h * dz, f0, kernel)[0]) / (2 * k * h) for k in (1, 2)]
    tol = abs(D[1] - D[0]) + 64 * EPS * _phi(sc, z0, f0, kernel)[1] / h
    print('full %.9e  without dJ/dz %.9e  D(h) %.9e  tol %.3e' % (full, without, D[0], tol))
    assert abs(D[0] - full) <= tol
    assert abs(full - without) > tol and abs(D[0] - without) > tol


# ------------------------------------------------------------------------------------------------ the implicit gradient
def _dist6(a, b):
    return lie.se3_log(lie.se3_mul(lie.se3_inv(a), b))


@pytest.mark.parametrize('what', ['flow', 'depth'])
def test_implicit_gradient_matches_refining_again(what):
    """A zero-residual scene (float64 flow, no noise), where H is the exact Hessian: the pose the LM restatement converges to on data
    moved by +-eps along a smooth direction, against xi = -H^-1 (dg/dtheta . direction) with dg/dtheta from the restatement (w = e_k
    gives row k).  The difference quotient of Log(T*^-1 T*_eps) is held to its Richardson estimate plus 10 x the refinement's last
    step over eps (how far a run may stop from its optimum), and that bound is asserted below 1e-3 of the value.  The runs from T* take
    six evaluations: they stall after three or four (the accept test cannot see a cost decrease below its rounding, a step of about
    1e-12 here), and every further rejected trial only raises the damping, which shrinks the reported last step below the distance
    to the optimum it stands for (at twelve evaluations: damping 1e3, last step 4e-15, undamped step 3e-12)."""
    sc = make_scene(1, 24, 40, seed=5, intr0=(40.0, 40.0, 19.5, 11.5), low_depth=False, flow_dtype=np.float64)
    z0, f0, mask, mount, intr = sc['depth'][0].astype(np.float64), sc['flow'][0], sc['mask'][0], sc['rgb2imu'], sc['intr'][0]
    start = right_perturb(sc['motion'][0], [0.004, -0.003, 0.005, 0.002, -0.001, 0.002])
    first = refine_reference_link(z0, f0, mask, start, mount, intr, iters=12)
    star = first['motion']
    at = reproj_reference_link(z0, f0, mask, star, mount, intr)
    assert first['status'] == 0 and at['cost'] < 1e-18 and at['count'] > 800
    v, u = np.meshgrid(np.arange(24.0), np.arange(40.0), indexing='ij')
    if what == 'flow':
        dz, df, eps = np.zeros((24, 40)), np.stack([np.sin(0.2 * u + 0.1 * v), np.cos(0.15 * v - 0.1 * u)]), 1e-3
    else:
        dz, df, eps = 0.5 + 0.4 * np.sin(0.15 * u - 0.2 * v), np.zeros((2, 24, 40)), 1e-3
    G = np.zeros(6)
    for k in range(6):
        r = vjp_reference_link(z0, f0, mask, star, mount, intr, np.eye(6)[k])
        G[k] = (r['grad_depth'] * dz).sum() + (r['grad_flow'] * df).sum()
    want = -np.linalg.solve(at['H'], G)
    D, last = [], 0.0
    for step in (eps, 2 * eps):
        ends = []
        for sign in (1.0, -1.0):
            run = refine_reference_link(z0 + sign * step * dz, f0 + sign * step * df, mask, star, mount, intr, iters=6)
            moved = reproj_reference_link(z0 + sign * step * dz, f0 + sign * step * df, mask, run['motion'], mount, intr)
            assert run['status'] == 0 and np.array_equal(moved['valid'], at['valid'])
            last = max(last, run['last_step'])
            ends.append(_dist6(star, run['motion']))
        D.append((ends[0] - ends[1]) / (2 * step))
    tol = np.abs(D[1] - D[0]).max() + 10 * last / eps
    print('%s: xi/eps %s\n   predicted %s\n   diff %.3e tol %.3e (last step %.3e)' % (what, D[0], want, np.abs(D[0] - want).max(), tol, last))
    assert np.abs(D[0] - want).max() <= tol
    assert tol < 1e-3 * np.abs(want).max()


def test_tangent_conversion_matches_central_differences():
    """v from a gradient on [t, q] against central differences of L(motion Exp(xi)), L = coeff . [t, q] (linear in the seven numbers,
    so its gradient on them is coeff)."""
    rng = np.random.default_rng(4)
    for _ in range(4):
        motion = lie.se3_exp(np.concatenate([rng.uniform(-1, 1, 3), rng.uniform(-1.5, 1.5, 3)]))
        coeff = rng.standard_normal(7)
        v = tangent_from_pose_grad(motion, coeff)
        h = 1e-5
        for k in range(6):
            D = []
            for step in (h, 2 * h):
                e = np.zeros(6)
                e[k] = step
                D.append(float(coeff @ (right_perturb(motion, e) - right_perturb(motion, -e))) / (2 * step))
            tol = abs(D[1] - D[0]) + 64 * EPS * float(np.abs(coeff) @ np.abs(motion)) / h
            assert abs(D[0] - v[k]) <= tol and tol < 1e-6 * np.abs(v).max(), (k, D, v[k], tol)


# ------------------------------------------------------------------------------------------------ the library without a GPU
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib, ops
    for name in ('islam_dense_reproj_vjp', 'islam_dense_reproj_ift_weights'):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        assert name in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'islam_hip.h')).read()
    assert callable(ops.dense_reproj_vjp) and callable(ops.dense_reproj_ift_weights)
    assert lib.islam_abi_version() == 1


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    one = 1        # any non-NULL address: a refused call never reads it

    def vjp(B=1, H=2, W=2, kind=0, delta=1.0, depth=one, flow=one, motion=one, intr=one, w=one, gd=one, gf=one):
        return lib.islam_dense_reproj_vjp(depth, flow, None, motion, None, intr, B, H, W, kind, delta, w, None, gd, gf, None)

    def ift(B=1, Hm=one, motion=one, grad=one, w=one, status=one):
        return lib.islam_dense_reproj_ift_weights(Hm, motion, grad, None, B, w, status, None)

    for kw, what in ((dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
                     (dict(kind=3), b'robust kind'), (dict(kind=-1), b'robust kind'), (dict(kind=1, delta=0.0), b'delta'),
                     (dict(kind=2, delta=-2.0), b'delta'), (dict(delta=float('nan')), b'delta'), (dict(depth=None), b'NULL'),
                     (dict(flow=None), b'NULL'), (dict(motion=None), b'NULL'), (dict(intr=None), b'NULL'), (dict(w=None), b'NULL'),
                     (dict(gd=None), b'NULL'), (dict(gf=None), b'NULL')):
        assert vjp(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_dense_reproj_vjp' in msg and what in msg, (kw, msg)
    for kw, what in ((dict(B=0), b'bad shape'), (dict(B=-3), b'bad shape'), (dict(Hm=None), b'NULL'), (dict(motion=None), b'NULL'),
                     (dict(grad=None), b'NULL'), (dict(w=None), b'NULL'), (dict(status=None), b'NULL')):
        assert ift(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_dense_reproj_ift_weights' in msg and what in msg, (kw, msg)


def test_ops_refuse_cpu_tensors():
    from islam_amd import lietensor as pp
    from islam_amd import ops
    from islam_amd.dense_ba import DenseReprojectionLoss
    sc = make_scene(1, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (t(sc['depth']), t(sc['flow']), t(sc['mask']), t(sc['motion']), t(sc['intr']))
    with pytest.raises(RuntimeError):
        ops.dense_reproj_vjp(*args, torch.zeros(1, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.dense_reproj_ift_weights(torch.eye(6, dtype=torch.float64)[None], t(sc['motion']), torch.zeros(1, 7, dtype=torch.float64))
    fx, fy, cx, cy = sc['intr'][0]
    loss = DenseReprojectionLoss(t(sc['depth']).requires_grad_(), t(sc['flow']).requires_grad_(), fx, fy, cx, cy, t(sc['mask']),
                                 pp.SE3(t(sc['rgb2imu'])), device='cpu')
    assert loss.z.requires_grad and loss.flow.requires_grad          # the stored tensors keep their graph
    with pytest.raises(RuntimeError):
        loss.refine(pp.SE3(t(sc['motion'])), iters=3, differentiable=True)

