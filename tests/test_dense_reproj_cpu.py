"""Dense reprojection normal equations (include/islam_hip.h, "dense reprojection"): everything about the
float64 numpy restatement (tests/dense_reproj_f64.py) and the library that can be checked without a GPU -- the convention (gradient
against central differences, the quadratic form, the mount conjugation), PvgoInfo.from_dense_reproj, the host-side argument errors
and the register metadata of the whole dense reprojection kernel family."""
import os

import numpy as np
import pytest
import torch

from islam_amd import robust
from islam_amd.information import PvgoInfo
from oracle import lie
from tests.dense_reproj_f64 import (MOUNT, OK, S_L1, make_scene, refine_reference_link, reproj_reference, reproj_reference_link, right_perturb,
                                    scene_args)


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


# every kernel of the family (dense_reproj.hip, dense_ba.hip)
FAMILY_KERNELS = ('dense_reproj_partial_kernel', 'dense_reproj_final_kernel', 'reproj_vjp_kernel', 'reproj_ift_kernel', 'dense_ba_partial_kernel',
                  'dense_ba_final_kernel', 'dense_ba_gather_kernel', 'joint_adj_partial_kernel', 'joint_adj_solve_kernel', 'joint_adj_vjp_kernel')


def test_dense_family_kernels_do_not_spill(lib):
    """Thirty fp64 accumulators plus the pose (two poses and the per-pixel Schur terms in the joint kernel) are tight: the library holds
    exactly the ten kernels of the family, and none of them may have a private segment or a spilled VGPR."""
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = {n: blk for n, blk in _kernels().items() if any(part in n for part in ('dense_reproj', 'dense_ba', 'reproj_vjp', 'reproj_ift', 'joint_adj'))}
    assert len(ks) == len(FAMILY_KERNELS) and all(sum(want in n for n in ks) == 1 for want in FAMILY_KERNELS), sorted(ks)
    for n, blk in ks.items():
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, n
