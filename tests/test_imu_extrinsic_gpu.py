"""GPU tests of the camera-IMU extrinsic-rotation solve (islam_imu_extrinsic_rot_solve through islam_amd.ops and
IMUModule.estimate_extrinsic_rotation).

Reference: extrinsic_reference below, a float64 numpy restatement written pair by pair from the definition in include/islam_hip.h
(canonical quaternions, M_i = L(qb_i) - R(qc_i), A = sum w rho M^T M, numpy.linalg.eigh, the same K Huber rounds).  Planted truth:
camera rotations Exp(N(0, sigma^2 I)), body rotations q_true (x) qc_i (x) q_true^-1 with q_true = Exp((1.1, -0.7, 0.4)), a random half
of the body quaternions negated (the canonicalisation must make that invisible).

Tolerances are measured, not fixed.  For every case two angles are taken first: the restatement's to the planted q_true, and the one
between the restatement summed forwards and summed backwards (the sensitivity to the summation order).  The library is held, against
the planted truth and against the restatement, to 10 x the larger of the two, with a floor of 16 * 2^-52 * l3 / (l1 - l0): the
first-order eigenvector perturbation bound for sixteen roundings of |A|.  Eigenvalues against eigh: 1e-9 l3, the float64 bound of
tests/test_imu_cov_gpu.py for accumulated matrices.  The residuals against the restatement's: the same angle bound.  All angles are
rotation angles, 2 atan2(|vec|, |w|) of the relative quaternion.  The partial-sum kernel's reach is 1024 pairs, hence the 1024 and 1025 cases."""
import functools

import numpy as np
import pytest
import torch

from tests.test_imu_align_gpu import _mat_to_quat, make_stream
from tests.test_imu_cov_gpu import _rounded

pytestmark = pytest.mark.gpu

REACH = 1024                                          # pairs one workgroup of the partial-sum kernel sums (csrc/imu_terms.h)
EPS = 2.0 ** -52


def qexp(v):
    """Exp of rotation vectors (..., 3) -> xyzw (..., 4)"""
    v = np.asarray(v, np.float64)
    t = np.linalg.norm(v, axis=-1, keepdims=True)
    k = np.where(t > 1e-8, np.sin(0.5 * t) / np.where(t > 1e-8, t, 1.0), 0.5 - t * t / 48.0)
    return np.concatenate([k * v, np.cos(0.5 * t)], -1)


def qmul(a, b):
    ax, ay, az, aw = np.moveaxis(np.asarray(a, np.float64), -1, 0)
    bx, by, bz, bw = np.moveaxis(np.asarray(b, np.float64), -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def qinv(a):
    return np.asarray(a, np.float64) * np.array([-1.0, -1.0, -1.0, 1.0])


def qangle(a, b):
    """the rotation angle between two unit quaternions (the sign of either does not matter)"""
    e = qmul(qinv(a), b)
    return 2.0 * np.arctan2(np.linalg.norm(e[..., :3], axis=-1), np.abs(e[..., 3]))


Q_TRUE = qexp(np.array([1.1, -0.7, 0.4]))


@functools.lru_cache(maxsize=None)
def planted(n, sigma=0.05, noise=0.0, outliers=False, axis=None):
    """(qb (n, 4), qc (n, 4)) of the planted mount.  noise: rotation noise (rad) on every body rotation; outliers: every tenth body
    rotation corrupted by Exp(N(0, 0.05^2)); axis: all camera rotations about this one axis."""
    rng = np.random.default_rng(5 + n)
    if axis is None:
        qc = qexp(rng.normal(0.0, sigma, (n, 3)))
    else:
        a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
        qc = qexp(rng.normal(0.0, sigma, (n, 1)) * a[None, :])
    qb = qmul(qmul(Q_TRUE, qc), qinv(Q_TRUE))
    if noise:
        qb = qmul(qb, qexp(rng.normal(0.0, noise, (n, 3))))
    if outliers:
        qb[::10] = qmul(qb[::10], qexp(rng.normal(0.0, 0.05, (len(qb[::10]), 3))))
    flip = rng.permutation(n) < n // 2                # a random half of the body quaternions negated
    qb[flip] = -qb[flip]
    qb.setflags(write=False)
    qc.setflags(write=False)
    return qb, qc


def _canon(q):
    q = np.asarray(q, np.float64)
    with np.errstate(all='ignore'):
        n = np.sqrt(q @ q)
        if not (n > 0 and np.isfinite(n)):
            return None
        q = q / n
    return -q if q[3] < 0 else q


def _lmat(a):
    x, y, z, w = a
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def _rmat(a):
    x, y, z, w = a
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def _theta(b, c, q):
    e = qmul(qinv(b), qmul(qmul(q, c), qinv(q)))
    return 2.0 * np.arctan2(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]), abs(e[3]))


def extrinsic_reference(rot_imu, rot_cam, weight=None, delta=None, rounds=4, backward=False):
    """(q (4), eig (4) ascending, res (n), excluded) from the definition, pair by pair, float64; (zeros, zeros, zeros, excluded) when no
    pair takes part.  backward: the sum runs from the last pair to the first."""
    n = len(rot_imu)
    pairs = [(_canon(rot_imu[i]), _canon(rot_cam[i])) for i in range(n)]
    K = int(rounds) if delta else 0
    q, lam, bad = np.zeros(4), np.zeros(4), 0
    for r in range(K + 1):
        A, bad, part = np.zeros((4, 4)), 0, 0
        for i in (range(n - 1, -1, -1) if backward else range(n)):
            w = 1.0 if weight is None else weight[i]
            if w == 0:
                continue
            b, c = pairs[i]
            if b is None or c is None or not np.isfinite(w) or w < 0:
                bad += 1
                continue
            rho = 1.0
            if r > 0:
                th = _theta(b, c, q)
                rho = min(1.0, delta / th) if th > 0 else 1.0
            M = _lmat(b) - _rmat(c)
            A += w * rho * (M.T @ M)
            part += 1
        if part == 0:
            return np.zeros(4), np.zeros(4), np.zeros(n), bad
        lam, V = np.linalg.eigh(A)
        q = V[:, 0] / np.linalg.norm(V[:, 0])
        q = -q if q[3] < 0 else q
    res = np.array([np.nan if b is None or c is None else _theta(b, c, q) for b, c in pairs])
    return q, lam, res, bad


def extrinsic_reference_vec(rot_imu, rot_cam):
    """The same sum for valid pairs of unit weight, all pairs at once (numpy's order of summation): (q, eig, res)."""
    def canon(q):
        q = np.asarray(q, np.float64)
        q = q / np.sqrt(np.sum(q * q, -1, keepdims=True))
        return np.where(q[:, 3:4] < 0, -q, q)
    b, c = canon(rot_imu), canon(rot_cam)
    d, s, m = b[:, 3] - c[:, 3], b[:, :3] + c[:, :3], b[:, :3] - c[:, :3]
    M = np.stack([np.stack([d, -s[:, 2], s[:, 1], m[:, 0]], -1), np.stack([s[:, 2], d, -s[:, 0], m[:, 1]], -1),
                  np.stack([-s[:, 1], s[:, 0], d, m[:, 2]], -1), np.stack([-m[:, 0], -m[:, 1], -m[:, 2], d], -1)], 1)
    A = np.einsum('nki,nkj->ij', M, M)
    lam, V = np.linalg.eigh(0.5 * (A + A.T))
    q = V[:, 0] / np.linalg.norm(V[:, 0])
    q = -q if q[3] < 0 else q
    return q, lam, qangle(b, qmul(qmul(q, c), qinv(q)))


def angle_floor(lam):
    """16 roundings of |A| against the gap of the smallest eigenvalue: the first-order eigenvector perturbation bound"""
    gap = lam[1] - lam[0]
    return 16.0 * EPS * lam[3] / gap if gap > 0 else np.inf


@functools.lru_cache(maxsize=None)
def measured(n, dtype_name='float64', sigma=0.05, noise=0.0, outliers=False, delta=None, rounds=4, wseed=None):
    """The restatement on a planted case (inputs rounded to the I/O dtype) and the measured bound:
    dict(q, eig, res, bad, e_ref, e_ord, bound, weight).  Over 10 000 pairs the vectorised restatement is used, forwards and on the
    reversed arrays; its different order of summation is inside the bound."""
    qb, qc = planted(n, sigma, noise, outliers)
    qb, qc = _rounded(qb, np.dtype(dtype_name).type), _rounded(qc, np.dtype(dtype_name).type)
    w = None if wseed is None else np.random.default_rng(wseed).uniform(0.2, 3.0, n)
    if n > 10000:
        assert w is None and not delta
        q, lam, res = extrinsic_reference_vec(qb, qc)
        qr, bad = extrinsic_reference_vec(qb[::-1], qc[::-1])[0], 0
    else:
        q, lam, res, bad = extrinsic_reference(qb, qc, w, delta, rounds)
        qr = extrinsic_reference(qb, qc, w, delta, rounds, backward=True)[0]
    e_ref, e_ord = float(qangle(q, Q_TRUE)), float(qangle(q, qr))
    return dict(qb=qb, qc=qc, q=q, eig=lam, res=res, bad=bad, e_ref=e_ref, e_ord=e_ord, weight=w,
                bound=max(10.0 * max(e_ref, e_ord), angle_floor(lam)))


def _t(cuda, a, dtype=np.float64):
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), dtype=td, device=cuda)


def _solve(cuda, qb, qc, dtype=np.float64, weight=None, delta=None, rounds=4):
    """ops.imu_extrinsic_rot_solve -> (q, eig, res, excluded) as numpy"""
    from islam_amd import ops
    q, eig, res, bad = ops.imu_extrinsic_rot_solve(_t(cuda, qb, dtype), _t(cuda, qc, dtype), None if weight is None else _t(cuda, weight),
                                                   delta, rounds)
    for t, k in ((q, 4), (eig, 4), (res, len(qb))):
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (k,)
    return q.cpu().numpy(), eig.cpu().numpy(), res.cpu().numpy(), bad


def _check(tag, got, ref):
    """library against the planted truth and against the restatement, under the measured bound; prints every figure first"""
    q, eig, res, bad = got
    e_lib, par = float(qangle(q, Q_TRUE)), float(qangle(q, ref['q']))
    e_eig = float(np.abs(eig - ref['eig']).max())
    e_res = float(np.abs(res - ref['res']).max())
    print('%s: restatement vs planted %.3g, forward vs backward %.3g, bound %.3g (floor %.3g); library vs planted %.3g, vs restatement %.3g, '
          'residuals %.3g, eigenvalues %.3g of l3 = %.3g, l1 / l3 = %.3g'
          % (tag, ref['e_ref'], ref['e_ord'], ref['bound'], angle_floor(ref['eig']), e_lib, par, e_res, e_eig / ref['eig'][3], ref['eig'][3],
             ref['eig'][1] / ref['eig'][3]))
    assert bad == ref['bad']
    assert abs(np.linalg.norm(q) - 1.0) <= 4 * EPS and q[3] >= 0
    assert np.all(np.diff(eig) >= 0)
    assert e_lib <= ref['bound'] and par <= ref['bound']
    assert e_eig <= 1e-9 * ref['eig'][3]
    assert e_res <= ref['bound']


# ------------------------------------------------------------------------------------------------ 1. parity and recovery
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('n', [2, 3, 65, 257, REACH, REACH + 1, 5000, 70001])
def test_against_the_restatement_and_the_planted_truth(cuda, n, dtype):
    ref = measured(n, np.dtype(dtype).name)
    got = _solve(cuda, ref['qb'], ref['qc'], dtype)
    _check('%d %s' % (n, np.dtype(dtype).name), got, ref)
    again = _solve(cuda, ref['qb'], ref['qc'], dtype)     # a second call: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and again[3] == got[3] == 0


def test_one_pair_alone(cuda):
    """One pair leaves a two-dimensional null space: l1 - l0 <= 1e-9 l3, no error, and no claim on q.  Every vector of that null space
    turns qc into qb exactly, so the residual is rounding: the null SPACE is separated from the rest by l2 - l1 (= l3 here), so the
    returned vector lies in it to 16 eps l3 / (l2 - l1) by the same perturbation bound, a rotation angle is twice a quaternion angle,
    and the residual's own three quaternion products add 16 eps more: 48 eps l3 / (l2 - l1), or 10 x the restatement's residual."""
    qb, qc = planted(1)
    q, eig, res, bad = _solve(cuda, qb, qc)
    _, lam, res_ref, _ = extrinsic_reference(qb, qc)
    bound = max(10.0 * res_ref[0], 48.0 * EPS * lam[3] / (lam[2] - lam[1]))
    print('one pair: eig %s, (l1 - l0) / l3 = %.3g, residual %.3g (restatement %.3g, bound %.3g)' % (eig, (eig[1] - eig[0]) / eig[3], res[0],
                                                                                                    res_ref[0], bound))
    assert bad == 0 and eig[1] - eig[0] <= 1e-9 * eig[3]
    assert np.abs(eig - lam).max() <= 1e-9 * lam[3]
    assert res[0] <= bound


# ------------------------------------------------------------------------------------------------ 2. degeneracy
def _one_axis_module(cuda):
    """A module whose gyro turns about one axis only, and the camera rotations that go with its motion rows under the planted mount"""
    from islam_amd.imu_integrator import IMUModule
    rng = np.random.default_rng(11)
    S, per = 120, 10
    t = np.arange(S) * 0.005
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    gyro = (0.8 * np.sin(1.3 * t + 0.2) + 0.5)[:, None] * axis[None, :]
    acc = np.array([0.0, 0.0, 9.81]) + rng.normal(0, 0.1, (S, 3))
    imu = IMUModule(acc, gyro, np.full(S, 0.005), rgb2imu_sync=np.arange(0, S, per), device='cuda:0', denoise_accel=False, denoise_gyro=False,
                    dtype=torch.float64)
    return imu, 0, S // per - 1


def test_rotations_about_one_axis(cuda):
    qb, qc = planted(50, axis=(0.3, -0.5, 0.8))
    q, eig, res, bad = _solve(cuda, qb, qc)
    lam = extrinsic_reference(qb, qc)[1]
    print('one axis, 50 pairs: eig %s (eigh %s), (l1 - l0) / l3 = %.3g' % (eig, lam, (eig[1] - eig[0]) / eig[3]))
    assert bad == 0 and (eig[1] - eig[0]) / eig[3] <= 1e-9          # no error: the eigenvalues carry the degeneracy
    assert np.abs(eig - lam).max() <= 1e-9 * lam[3]
    # the module: min_gap turns the same diagnosis into a ValueError, on one-axis data only
    imu, st, end = _one_axis_module(cuda)
    dr = imu.integrate(st, end, motion_mode=True)[1].tensor().numpy()
    cam = qmul(qmul(qinv(Q_TRUE), dr), Q_TRUE)
    q1, eig1, _ = imu.estimate_extrinsic_rotation(st, end, cam)
    print('one-axis module: (l1 - l0) / l3 = %.3g' % float((eig1[1] - eig1[0]) / eig1[3]))
    with pytest.raises(ValueError, match='one axis'):
        imu.estimate_extrinsic_rotation(st, end, cam, min_gap=1e-6)
    imu3, st3, end3, cam3, _ = _planted_module()
    q3, eig3, _ = imu3.estimate_extrinsic_rotation(st3, end3, cam3, min_gap=1e-6)
    assert float((eig3[1] - eig3[0]) / eig3[3]) >= 1e-6


# ------------------------------------------------------------------------------------------------ 3. Huber rounds
HUBER = dict(sigma=0.05, noise=2e-4, outliers=True)


@pytest.mark.parametrize('K', [1, 2, 4])
def test_huber_rounds(cuda, K):
    ref = measured(300, delta=1e-3, rounds=K, **HUBER)
    got = _solve(cuda, ref['qb'], ref['qc'], delta=1e-3, rounds=K)
    _check('huber K=%d' % K, got, ref)


def test_huber_gain_and_delta_zero(cuda):
    plain, robust = measured(300, **HUBER), measured(300, delta=1e-3, rounds=4, **HUBER)
    print('restatement vs planted: %.3g plain, %.3g after 4 rounds' % (plain['e_ref'], robust['e_ref']))
    assert 10.0 * robust['e_ref'] <= plain['e_ref']
    lib0, lib4 = _solve(cuda, plain['qb'], plain['qc']), _solve(cuda, plain['qb'], plain['qc'], delta=1e-3, rounds=4)
    print('library vs planted: %.3g plain, %.3g after 4 rounds' % (qangle(lib0[0], Q_TRUE), qangle(lib4[0], Q_TRUE)))
    # delta = 0 with rounds = 4: the bits of rounds = 0
    a, b = _solve(cuda, plain['qb'], plain['qc'], delta=0.0, rounds=4), _solve(cuda, plain['qb'], plain['qc'], delta=None, rounds=0)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and all(np.array_equal(x, y) for x, y in zip(a[:3], lib0[:3]))


# ------------------------------------------------------------------------------------------------ 4. weights and exclusion
def test_weights_and_exclusion(cuda):
    from islam_amd import _lib, ops
    ref = measured(70, wseed=3)
    qb, qc, n = ref['qb'], ref['qc'], 70
    _check('70 weights', _solve(cuda, qb, qc, weight=ref['weight']), ref)
    # weight 0 on two pairs, with and without NaN behind them: the same bits, nothing counted
    w0 = np.ones(n)
    w0[[19, 20]] = 0.0
    qbn, qcn = qb.copy(), qc.copy()
    qbn[19, 1] = np.nan
    qcn[20, 3] = np.nan
    clean, dirty = _solve(cuda, qb, qc, weight=w0), _solve(cuda, qbn, qcn, weight=w0)
    assert clean[3] == 0 and dirty[3] == 0
    assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1])
    keep = np.ones(n, bool)
    keep[[19, 20]] = False
    assert np.array_equal(clean[2][keep], dirty[2][keep]) and np.isnan(dirty[2][[19, 20]]).all() and np.isfinite(clean[2]).all()
    want = extrinsic_reference(qb, qc, w0)
    print('zero weights: library vs restatement %.3g, residuals of the two idle pairs %s (restatement %s)'
          % (qangle(clean[0], want[0]), clean[2][[19, 20]], want[2][[19, 20]]))
    assert qangle(clean[0], want[0]) <= ref['bound'] and np.abs(clean[2] - want[2]).max() <= ref['bound']
    # the same NaN under weight 1 (pair 19): excluded and counted, q is the bits of the zero-weight call, its residual is NaN
    w1 = np.ones(n)
    w1[20] = 0.0
    got = _solve(cuda, qbn, qcn, weight=w1)
    assert got[3] == 1 and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1]) and np.isnan(got[2][19])
    assert extrinsic_reference(qbn, qcn, w1)[3] == 1
    # a zero quaternion and a negative weight: each counted, and neither takes part
    qcz = qc.copy()
    qcz[19] = 0.0
    wn = np.ones(n)
    wn[20] = -1.0
    z, neg, both = _solve(cuda, qb, qcz), _solve(cuda, qb, qc, weight=wn), _solve(cuda, qb, qcz, weight=wn)
    assert (z[3], neg[3], both[3]) == (1, 1, 2) and np.array_equal(both[0], clean[0]) and np.array_equal(both[1], clean[1])
    assert np.isnan(z[2][19]) and np.isfinite(neg[2]).all()
    # no pair takes part (all weights zero, rows == 0): ISLAM_ENOTPD with the entry point's name; at the C level zeros are written
    with pytest.raises(_lib.IslamHipError) as ei:
        _solve(cuda, qb, qc, weight=np.zeros(n))
    assert ei.value.code == -3 and 'islam_imu_extrinsic_rot_solve' in str(ei.value)
    with pytest.raises(_lib.IslamHipError) as ei:
        ops.imu_extrinsic_rot_solve(_t(cuda, np.zeros((0, 4))), _t(cuda, np.zeros((0, 4))))
    assert ei.value.code == -3 and 'islam_imu_extrinsic_rot_solve' in str(ei.value)
    for rows, wz in ((n, np.zeros(n)), (0, None)):
        out = torch.full((8 + rows,), 7.0, dtype=torch.float64, device=cuda)
        scratch = torch.empty(_lib.lib().islam_imu_extrinsic_rot_solve_scratch_bytes(rows), dtype=torch.uint8, device=cuda)
        a, b = _t(cuda, qb[:rows]), _t(cuda, qc[:rows])
        rc = _lib.lib().islam_imu_extrinsic_rot_solve(_lib.ptr(a), _lib.ptr(b), _lib.ptr(None if wz is None else _t(cuda, wz)), rows, 1e-3, 2,
                                                      _lib.ptr(out[0:4]), _lib.ptr(out[4:8]), _lib.ptr(out[8:]) if rows else None,
                                                      _lib.ptr(scratch), 1, _lib.stream_ptr(cuda))
        assert rc == -3 and not out.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ 5. IMUModule
def _planted_module():
    """A module over a planted stream with a ragged rgb2imu_sync and a non-identity initial rotation; the camera rotations are the
    planted body rotations conjugated by q_true^-1."""
    from islam_amd.imu_integrator import IMUModule
    counts = (5, 9, 12, 3, 10, 10, 7, 25, 10, 6, 11, 10, 4, 10, 8, 10)
    s = make_stream(counts, 1.0, np.zeros(3), seed=5, tail=1)
    imu = IMUModule(s['acc'], s['gyro'], s['dt'], accel_bias=torch.zeros(3), gyro_bias=torch.zeros(3), gravity=9.79,
                    rgb2imu_sync=s['seg'], device='cuda:0', denoise_accel=False, denoise_gyro=False, dtype=torch.float64,
                    init={'rot': _mat_to_quat(s['R'][0]), 'pos': s['p'][0], 'vel': s['v'][0]})
    st, end = 2, 15
    rel = np.stack([_mat_to_quat(s['R'][i].T @ s['R'][i + 1]) for i in range(st, end)])
    cam = qmul(qmul(qinv(Q_TRUE), rel), Q_TRUE)
    return imu, st, end, cam, (s, rel)


def test_imu_module(cuda):
    """The module's DR_i come from the shipped HIP integrator (a quaternion chain), not from the numpy chain the camera rotations were
    planted with, so the summation-order margin does not apply to it: the bound is the larger of the measured bound and 1e-9, the
    float64 tolerance the project holds that integrator's derived rows to (tests/test_imu_cov_gpu.py, tests/test_imu_bias_jac_gpu.py);
    a wrong frame, order of the product or sign is of order 1."""
    imu, st, end, cam, (s, rel) = _planted_module()
    quat = np.stack([_mat_to_quat(R) for R in s['R']])
    init = {'rot': quat[st], 'pos': s['p'][st], 'vel': s['v'][st]}
    others = lambda: (imu.estimate_gyro_bias(st, end, rel), imu.integrate(st, end, init), imu.integrate(st, end, init, motion_mode=True),
                      imu.estimate_gravity_accel_bias(st, end, quat[st:end + 1], s['p'][st:end + 1]))
    before = others()
    attrs = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(imu).items()}
    q, eig, res = imu.estimate_extrinsic_rotation(st, end, cam)
    for k, v in vars(imu).items():
        assert torch.equal(v, attrs[k]) if torch.is_tensor(v) else (v is attrs[k] or np.array_equal(v, attrs[k])), k
    assert set(vars(imu)) == set(attrs)
    for t, k in ((q, 4), (eig, 4), (res, end - st)):
        assert t.dtype == torch.float64 and t.device.type == 'cpu' and tuple(t.shape) == (k,)
    qr, lam, _, _ = extrinsic_reference(rel, cam)
    e_ref, e_ord = float(qangle(qr, Q_TRUE)), float(qangle(qr, extrinsic_reference(rel, cam, backward=True)[0]))
    bound = max(10.0 * max(e_ref, e_ord), angle_floor(lam), 1e-9)
    e_lib = float(qangle(q.numpy(), Q_TRUE))
    print('module: restatement vs planted %.3g, forward vs backward %.3g, module vs planted %.3g, bound %.3g, largest residual %.3g, eig %s'
          % (e_ref, e_ord, e_lib, bound, float(res.max()), eig.numpy()))
    assert e_lib <= bound and float(res.max()) <= bound
    assert np.abs(eig.numpy() - lam).max() <= 1e-9 * lam[3]
    # SO3 input, weights and the Huber rounds pass through
    from islam_amd import lietensor as pp
    w = np.ones(end - st)
    w[3] = 0.0
    q2, _, res2 = imu.estimate_extrinsic_rotation(st, end, pp.SO3(torch.tensor(cam)), weight=w, delta=1e-3, rounds=2)
    assert float(qangle(q2.numpy(), Q_TRUE)) <= bound and np.isfinite(res2.numpy()).all()
    # the other entry points give what they gave before
    after = others()
    assert torch.equal(before[0][0], after[0][0]) and torch.equal(before[0][1], after[0][1])
    for a, b in zip(before[1:3], after[1:3]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].tensor(), b[1].tensor()) and torch.equal(a[3], b[3])
    assert all(torch.equal(a, b) for a, b in zip(before[3], after[3]))
