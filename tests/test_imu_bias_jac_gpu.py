"""GPU tests of the pre-integration bias Jacobians (islam_imu_preint_bias_jac), the first-order bias correction
(islam_imu_bias_correct) and the closed-form gyro-bias solve (islam_imu_gyro_bias_solve) through islam_amd.ops and IMUModule.

Reference: jac_reference below, a float64 numpy restatement of the recurrence include/islam_hip.h defines, one sample after the
other; integrate_reference is the plain numpy integrator of the same discretisation (gravity 0, start-body frame) and
solve_reference the same normal equations in numpy.  Error measure of a Jacobian: every entry against the largest absolute entry of
its own 3x3 block in the reference, bound 1e-9 -- the float64 tolerance of tests/test_imu_cov_gpu.py, whose join depth and
arithmetic are the same; a block that is zero in the reference must be exactly zero."""
import numpy as np
import pytest
import torch

from islam_amd import synthetic
from tests.test_imu_cov_gpu import _exp_jr, _hat, _quat_to_mat, _ragged, _rounded

pytestmark = pytest.mark.gpu

TOL = 1e-9


def jac_reference(dt, gyro, acc, seg, motion, init_jac=None):
    """J <- A J - [Bg | Ba] sample by sample (float64), A, Bg, Ba as in cov_reference.  motion: nframes rows, every frame from J = 0,
    DR = I; else nframes + 1 rows, row 0 = init_jac (its (dphi, b_a) block dropped), row k over all samples [seg[0], seg[k])."""
    dt, gyro, acc = np.asarray(dt, np.float64), np.asarray(gyro, np.float64), np.asarray(acc, np.float64)
    n = len(seg) - 1
    out = np.zeros((n if motion else n + 1, 9, 6))
    J = np.zeros((9, 6))
    if init_jac is not None and not motion:
        J = np.array(init_jac, dtype=np.float64)
        J[0:3, 3:6] = 0.0
    DR = np.eye(3)
    if not motion:
        out[0] = J
    I3 = np.eye(3)
    for i in range(n):
        if motion:
            J, DR = np.zeros((9, 6)), np.eye(3)
        for j in range(int(seg[i]), int(seg[i + 1])):
            d = dt[j]
            dr, Jr = _exp_jr(gyro[j] * d)
            Ra = DR @ _hat(acc[j])
            A = np.zeros((9, 9))
            A[0:3, 0:3] = dr.T
            A[3:6, 0:3] = -Ra * d
            A[6:9, 0:3] = -0.5 * Ra * d * d
            A[3:6, 3:6] = I3
            A[6:9, 3:6] = I3 * d
            A[6:9, 6:9] = I3
            B = np.zeros((9, 6))
            B[0:3, 0:3] = Jr * d
            B[3:6, 3:6] = DR * d
            B[6:9, 3:6] = 0.5 * DR * d * d
            J = A @ J - B
            DR = DR @ dr
        out[i + (0 if motion else 1)] = J
    return out


def integrate_reference(dt, gyro, acc):
    """(DR, dv, dp) of one interval in the body frame of its start, gravity 0: the discretisation of the integrator that ships
    (a rotated by the rotation in front of the sample; p += v d + a d^2 / 2, v += a d, DR <- DR Exp(w d))."""
    DR, v, p = np.eye(3), np.zeros(3), np.zeros(3)
    for j in range(len(dt)):
        d = dt[j]
        ra = DR @ acc[j]
        p = p + v * d + 0.5 * ra * d * d
        v = v + ra * d
        DR = DR @ _exp_jr(gyro[j] * d)[0]
    return DR, v, p


def log_so3(R):
    c = np.clip(0.5 * (np.trace(R) - 1.0), -1.0, 1.0)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    return v if s < 1e-12 else v * (np.arctan2(s, c) / s)


def solve_reference(jac, R_imu, R_ref, weight=None):
    """argmin sum_i w_i |Log(R_imu_i^T R_ref_i) - J_phig,i x|^2 by the normal equations (numpy float64): (x, H)."""
    H, g = np.zeros((3, 3)), np.zeros(3)
    for i in range(len(jac)):
        w = 1.0 if weight is None else weight[i]
        Jp = jac[i][0:3, 0:3]
        H += w * Jp.T @ Jp
        g += w * Jp.T @ log_so3(R_imu[i].T @ R_ref[i])
    return np.linalg.solve(H, g), H


def block_error(J, ref):
    """max over entries of |J - ref| / (largest |entry| of the entry's own 3x3 block in ref); inf if a block that is zero in ref is not
    exactly zero in J."""
    J, ref = np.asarray(J), np.asarray(ref)
    worst = 0.0
    for r in range(3):
        for c in range(2):
            a, b = J[..., 3 * r:3 * r + 3, 3 * c:3 * c + 3], ref[..., 3 * r:3 * r + 3, 3 * c:3 * c + 3]
            scale = np.abs(b).max(axis=(-1, -2))
            err = np.abs(a - b).max(axis=(-1, -2))
            if np.any(err[scale == 0] != 0):
                return np.inf
            k = scale > 0
            if k.any():
                worst = max(worst, float((err[k] / scale[k]).max()))
    return worst


def _t(cuda, a, dtype=np.float64):
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), dtype=td, device=cuda)


def _run(cuda, dt, gyro, acc, seg, motion, dtype=np.float64, init_jac=None):
    from islam_amd import ops
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    ij = None if init_jac is None else torch.tensor(init_jac, dtype=torch.float64, device=cuda)
    out = ops.imu_preint_bias_jac(_t(cuda, dt, dtype), _t(cuda, gyro, dtype), _t(cuda, acc, dtype), torch.tensor(seg, device=cuda), seg, motion, ij)
    assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (len(seg) - (1 if motion else 0), 9, 6)
    return out.cpu().numpy()


def _check(out, want):
    e = block_error(out, want)
    assert e <= TOL, e
    assert not out[:, 0:3, 3:6].any()                 # the (dphi, b_a) block is exactly zero
    return e


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('motion', [False, True])
@pytest.mark.parametrize('frames,per', [(1, 1), (3, 10), (64, 10), (65, 7), (4, 200)])
def test_against_the_restatement(cuda, dtype, motion, frames, per):
    tr = synthetic.car_trajectory(frames + 1, imu_per_frame=per, seed=frames + per)
    seg = tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0]
    assert len(seg) == frames + 1
    r = lambda a: _rounded(a, dtype)
    out = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, dtype)
    e = _check(out, jac_reference(r(tr['imu_dts']), r(tr['gyros']), r(tr['accels']), seg, motion))
    print('bias jac (%d, %d) %s %s: %.3g' % (frames, per, 'motion' if motion else 'world', np.dtype(dtype).name, e))
    assert np.array_equal(out, _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, dtype))       # a second call: the same bits


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_ragged_and_empty_intervals(cuda, dtype):
    counts, seg, dt, gyro, acc = _ragged()
    r = lambda a: _rounded(a, dtype)
    for motion in (False, True):
        out = _run(cuda, dt, gyro, acc, seg, motion, dtype)
        _check(out, jac_reference(r(dt), r(gyro), r(acc), seg, motion))
        for i, c in enumerate(counts):
            if c == 0:
                if motion:
                    assert not out[i].any()
                else:
                    assert np.array_equal(out[i + 1], out[i])
    # a stream that starts with frames without samples: they repeat row 0
    seg2 = np.concatenate([[0, 0, 0], seg])
    J0 = _init_jac(3)
    out = _run(cuda, dt, gyro, acc, seg2, False, dtype, init_jac=J0)
    want0 = J0.copy()
    want0[0:3, 3:6] = 0.0
    assert np.array_equal(out[0], want0) and np.array_equal(out[1], want0) and np.array_equal(out[2], want0)
    _check(out, jac_reference(r(dt), r(gyro), r(acc), seg2, False, J0))
    # no frames at all: world mode returns init_jac alone, motion mode nothing
    assert np.array_equal(_run(cuda, dt, gyro, acc, np.array([0]), False, dtype, init_jac=J0), want0[None])
    assert not _run(cuda, dt, gyro, acc, np.array([0]), False, dtype).any()
    assert _run(cuda, dt, gyro, acc, np.array([0]), True, dtype).shape == (0, 9, 6)


def _init_jac(seed):
    """A random 9x6 start, its (dphi, b_a) block NOT zero: the kernel must ignore it."""
    return np.random.default_rng(seed).normal(0, 1.0, (9, 6)) * np.array([0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.01, 0.01, 0.01])[:, None]


def test_full_size_5000_frames(cuda):
    """5000 frame intervals / 50 001 samples: three scan levels in world mode; a second call is bit-equal (no atomics, fixed order)."""
    tr = synthetic.car_trajectory(5001)
    seg = tr['rgb2imu_sync']
    assert len(seg) == 5001 and len(tr['imu_dts']) == 50001
    for motion in (False, True):
        out = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion)
        assert np.array_equal(out, _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion))
        e = _check(out, jac_reference(tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion))
        print('bias jac 5000 frames %s: %.3g' % ('motion' if motion else 'world', e))


def _ragged_blocks():
    rng = np.random.default_rng(5)
    n = 1301
    counts = rng.integers(1, 6, n)
    counts[rng.random(n) < 0.2] = 0
    for i, c in ((0, 0), (63, 0), (64, 0), (65, 3), (127, 2), (128, 0), (1279, 0), (1280, 0), (1300, 0)):
        counts[i] = c
    seg = np.concatenate([[0], np.cumsum(counts)])
    S = int(seg[-1])
    dt, gyro = rng.uniform(0.004, 0.012, S), rng.normal(0, 0.5, (S, 3))
    acc = rng.normal(0, 1.0, (S, 3)) + np.array([0, 0, 9.81])
    return counts, seg, dt, gyro, acc


def test_ragged_frames_across_the_scan_blocks(cuda):
    """Frames without samples at the borders of the 64-frame scan blocks, a last block that is not full, two scan levels."""
    counts, seg, dt, gyro, acc = _ragged_blocks()
    J0 = _init_jac(9)
    out = _run(cuda, dt, gyro, acc, seg, False, init_jac=J0)
    _check(out, jac_reference(dt, gyro, acc, seg, False, J0))
    for i in np.nonzero(counts == 0)[0]:
        assert np.array_equal(out[i + 1], out[i])
    assert np.array_equal(out, _run(cuda, dt, gyro, acc, seg, False, init_jac=J0))
    out = _run(cuda, dt, gyro, acc, seg, True)
    _check(out, jac_reference(dt, gyro, acc, seg, True))
    assert not out[counts == 0].any()


# ------------------------------------------------------------------------------------------------ 2. init_jac
@pytest.mark.parametrize('frames,per', [(9, 10), (200, 7)])
def test_init_jac_is_transported_and_windows_split(cuda, frames, per):
    """World rows from a random init_jac; and a window split in two: the second call's elements live in the body frame at the split,
    so it is handed diag(I, W^T, W^T) J_m and its rows are turned back by diag(I, W, W), W = the rotation accumulated over the first
    half -- taken from the forward (world rows of ops.imu_preint from the identity)."""
    from islam_amd import ops
    tr = synthetic.car_trajectory(frames + 1, imu_per_frame=per, seed=11)
    seg = tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0]
    S = int(seg[-1])
    dt, gyro, acc = tr['imu_dts'][:S], tr['gyros'][:S] * 5.0, tr['accels'][:S]          # (five times the car's rates: W is far from I)
    J0 = _init_jac(frames)
    out = _run(cuda, dt, gyro, acc, seg, False, init_jac=J0)
    _check(out, jac_reference(dt, gyro, acc, seg, False, J0))
    m = frames // 2
    sm = int(seg[m])
    first = _run(cuda, dt[:sm], gyro[:sm], acc[:sm], seg[:m + 1], False, init_jac=J0)
    assert block_error(first, out[:m + 1]) <= TOL
    z3, q0 = _t(cuda, np.zeros(3)), _t(cuda, np.array([0.0, 0.0, 0.0, 1.0]))
    segh = np.ascontiguousarray(seg[:m + 1], dtype=np.int64)
    rot = ops.imu_preint(_t(cuda, dt[:sm]), _t(cuda, gyro[:sm]), _t(cuda, acc[:sm]), torch.tensor(segh, device=cuda), segh, z3, q0, z3, 0.0, False)[1]
    W = _quat_to_mat(rot.cpu().numpy()[-1])
    T = np.zeros((9, 9))
    T[0:3, 0:3] = np.eye(3)
    T[3:6, 3:6] = T[6:9, 6:9] = W
    second = _run(cuda, dt[sm:], gyro[sm:], acc[sm:], seg[m:] - sm, False, init_jac=T.T @ first[-1])
    joined = np.einsum('ab,kbc->kac', T, second)
    assert block_error(joined, out[m:]) <= TOL


# ------------------------------------------------------------------------------------------------ 3. the integrator that ships
@pytest.mark.parametrize('per', [10, 70])
def test_consistent_with_the_integrator(cuda, per):
    """J_b = -sum_s d out / d sample_s of ops.imu_preint(motion_mode=True) (one frame, identity initial rotation, gravity 0), from
    islam_imu_preint_bwd with nine unit cotangents as tests/test_imu_cov_gpu.py::test_consistent_with_the_integrator takes them; its
    rotation rows are LEFT tangents, dphi_right = DR^T dphi_left.  Bound 1e-6 of the block's largest entry (that test's bound): both
    sides are the same first-order quantity, a convention error is of order |w d| ~ 1e-3 or larger."""
    from islam_amd import ops
    tr = synthetic.car_trajectory(2, imu_per_frame=per, seed=per)
    seg = np.ascontiguousarray(tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0], dtype=np.int64)
    S = int(seg[-1])
    dt = _t(cuda, tr['imu_dts'][:S])
    gyro, acc = _t(cuda, tr['gyros'][:S]).requires_grad_(True), _t(cuda, tr['accels'][:S]).requires_grad_(True)
    z3, q0 = _t(cuda, np.zeros(3)), _t(cuda, np.array([0.0, 0.0, 0.0, 1.0]))
    pos, rot, vel = ops.imu_preint(dt, gyro, acc, torch.tensor(seg, device=cuda), seg, z3, q0, z3, 0.0, True)
    DR = _quat_to_mat(rot.detach().cpu().numpy()[0])
    Jg, Ja = np.zeros((9, S, 3)), np.zeros((9, S, 3))
    for blk, o in enumerate((rot, vel, pos)):
        for k in range(3):
            g = torch.zeros_like(o)
            g[0, k] = 1.0
            gg, ga = torch.autograd.grad(o, (gyro, acc), grad_outputs=g, retain_graph=True)
            Jg[3 * blk + k], Ja[3 * blk + k] = gg.cpu().numpy(), ga.cpu().numpy()
    Jg[0:3] = np.einsum('ji,jsk->isk', DR, Jg[0:3])       # DR^T . (left tangent rows)
    Ja[0:3] = np.einsum('ji,jsk->isk', DR, Ja[0:3])
    want = -np.concatenate([Jg.sum(1), Ja.sum(1)], 1)
    out = _run(cuda, tr['imu_dts'][:S], tr['gyros'][:S], tr['accels'][:S], seg, True)[0]
    # the backward's (dphi, b_a) block is zero up to its own rounding; everything else to 1e-6 of its block
    assert np.abs(want[0:3, 3:6]).max() <= 1e-12
    want[0:3, 3:6] = 0.0
    e = block_error(out, want)
    print('bias jac vs -sum of the sample gradients (%d samples): %.3g' % (S, e))
    assert e <= 1e-6


# ------------------------------------------------------------------------------------------------ 4. the correction
def _random_stream(seed, frames, per):
    rng = np.random.default_rng(seed)
    S = frames * per
    seg = np.arange(frames + 1, dtype=np.int64) * per
    return seg, rng.uniform(0.004, 0.012, S), rng.normal(0, 0.5, (S, 3)), rng.normal(0, 1.0, (S, 3)) + np.array([0, 0, 9.81])


def _body_increments(cuda, dt, gyro, acc, seg, init_rot):
    """Motion rows of the shipped integrator (gravity 0) brought into the start-body frame of every frame, as include/islam_hip.h asks:
    vel_i, pos_i rotated by R0_i^T, R0_i = world-mode rotation row i of the same stream."""
    from islam_amd import ops
    z3, q0 = _t(cuda, np.zeros(3)), _t(cuda, init_rot)
    a = (_t(cuda, dt), _t(cuda, gyro), _t(cuda, acc), torch.tensor(seg, device=cuda), seg, z3, q0, z3, 0.0)
    pos, rot, vel = ops.imu_preint(*a, True)
    R0 = np.stack([_quat_to_mat(q) for q in ops.imu_preint(*a, False)[1].cpu().numpy()[:-1]])
    vb = np.einsum('kji,kj->ki', R0, vel.cpu().numpy())
    pb = np.einsum('kji,kj->ki', R0, pos.cpu().numpy())
    return rot.cpu().numpy(), vb, pb


def _inc_errors(a, b):
    """(rotation angle, |dv|, |dp|) differences of two sets of increments, the largest over the rows"""
    ang = max(np.linalg.norm(log_so3(_quat_to_mat(p).T @ _quat_to_mat(q))) for p, q in zip(a[0], b[0]))
    return np.array([ang, np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max()])


@pytest.mark.parametrize('init_rot', [[0.0, 0.0, 0.0, 1.0], [0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214]])
def test_bias_correct_is_second_order(cuda, init_rot):
    """The stream is re-integrated (float64, the shipped integrator, gravity 0) with the biases b and b / 2 subtracted; the increments of
    the unbiased stream corrected to first order miss them by O(|b|^2): the error ratio between b and b / 2 is 4 up to the third-order
    term, which is of relative size |b_g| T ~ 2e-3 here (bound 3 .. 5, for the rotation, the velocity and the position).  The
    uncorrected error is first order, its ratio r0 ~ 2: if the correction removes the whole first-order term, each halving of b gains
    r / r0 on it, so at b the corrected error must be below the uncorrected one by at least that factor (computed, not fixed).
    |b_g| = 0.02 rad/s and |b_a| = 0.2 m/s^2 over 0.16 s frames move the increments by 3.5e-3 rad, 2.8e-2 m/s, 2.4e-3 m; the numpy
    restatement leaves 3.6e-8 rad, 3.6e-5 m/s, 2.1e-6 m after the correction at b and 9.1e-9, 9.1e-6, 5.1e-7 at b / 2 (ratios 4.000,
    4.001, 4.001), eight orders and more above the rounding of increments of size 1.7 m/s and 0.15 m.  With a non-identity init_rot the motion rows are rotated into the
    start-body frame of their frame first (include/islam_hip.h)."""
    from islam_amd import ops
    seg, dt, gyro, acc = _random_stream(21, 6, 20)
    init_rot = np.array(init_rot)
    bg, ba = np.array([0.012, -0.016, 0.0]), np.array([0.12, 0.0, -0.16])
    assert abs(np.linalg.norm(bg) - 0.02) < 1e-12 and abs(np.linalg.norm(ba) - 0.2) < 1e-12
    base = _body_increments(cuda, dt, gyro, acc, seg, init_rot)
    jac = ops.imu_preint_bias_jac(_t(cuda, dt), _t(cuda, gyro), _t(cuda, acc), torch.tensor(seg, device=cuda), seg, True)
    err, raw = [], []
    for s in (1.0, 0.5):
        truth = _body_increments(cuda, dt, gyro - s * bg, acc - s * ba, seg, init_rot)
        got = ops.imu_bias_correct(jac, _t(cuda, base[0]), _t(cuda, base[1]), _t(cuda, base[2]), s * bg, s * ba)
        err.append(_inc_errors([g.cpu().numpy() for g in got], truth))
        raw.append(_inc_errors(base, truth))
    r, r0 = err[0] / err[1], raw[0] / raw[1]
    print('bias correct: corrected', err, 'uncorrected', raw, 'ratios', r, r0)
    assert np.all(err[1] > 1e-12)                     # far above rounding: the ratios mean something
    assert np.all(r > 3.0) and np.all(r < 5.0)
    assert np.all(raw[0] / err[0] >= r / r0)
    # float32 I/O: the same correction at b, from increments rounded to float32 and rounded once more on the way out
    got = ops.imu_bias_correct(jac, _t(cuda, base[0]), _t(cuda, base[1]), _t(cuda, base[2]), bg, ba)
    got32 =ops.imu_bias_correct(jac, _t(cuda, base[0], np.float32), _t(cuda, base[1], np.float32), _t(cuda, base[2], np.float32), bg, ba)
    for a, b in zip(got32, got):
        assert a.dtype == torch.float32 and torch.allclose(a.double(), b, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ 5. the gyro-bias solve
def _motion_rots(cuda, dt, gyro, acc, seg):
    from islam_amd import ops
    z3, q0 = _t(cuda, np.zeros(3)), _t(cuda, np.array([0.0, 0.0, 0.0, 1.0]))
    return ops.imu_preint(_t(cuda, dt), _t(cuda, gyro), _t(cuda, acc), torch.tensor(seg, device=cuda), seg, z3, q0, z3, 0.0, True)[1]


def _solve_stream(frames=60):
    tr = synthetic.car_trajectory(frames + 1, seed=17)
    seg = np.ascontiguousarray(tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0], dtype=np.int64)
    S = int(seg[-1])
    # the car's own rates are ~1e-2 rad/s, and with w = 0 the problem is exactly linear: a steady turn is added so that the second-order
    # term the test measures stands well above rounding
    gyro = tr['gyros'][:S] + np.array([0.3, -0.2, 0.5])
    return seg, tr['imu_dts'][:S], gyro, tr['accels'][:S]


GN_CONSTANT = 3e-4


def _solve_once(cuda, dt, gyro, acc, seg, ref):
    """(estimate, H, rows, rot, jac) of one solve of the stream `gyro` against the trusted rotations `ref`"""
    from islam_amd import ops
    jac = ops.imu_preint_bias_jac(_t(cuda, dt), _t(cuda, gyro), _t(cuda, acc), torch.tensor(seg, device=cuda), seg, True)
    rot = _motion_rots(cuda, dt, gyro, acc, seg)
    dbg, H, bad = ops.imu_gyro_bias_solve(jac, rot, ref)
    again = ops.imu_gyro_bias_solve(jac, rot, ref)
    assert torch.equal(dbg, again[0]) and torch.equal(H, again[1]) and bad == 0 and again[2] == 0          # repeat calls: the same bits
    return dbg.cpu().numpy(), H.cpu().numpy(), rot, jac


def test_gyro_bias_solve(cuda):
    """rot_ref from the clean stream, rot_imu from the stream with the gyro bias b added (60 frames of synthetic.car_trajectory plus a
    steady turn).  One solve misses b by O(|b|^2): ratio 3 .. 5 between |b| = 0.02 rad/s and b / 2 (the numpy restatement -- jac_reference,
    integrate_reference, solve_reference -- gives 1.735e-7 and 4.337e-8 rad/s: 4.00).
    A second Gauss-Newton round (subtract the estimate, re-integrate, solve again) leaves less than GN_CONSTANT * (first-round error)^2.
    It is run at |b| = 0.5 rad/s, where the second-round error stands above rounding (at 0.02 rad/s it is 2e-17, i.e. rounding).  The
    restatement on the CPU gives there e1 = 1.085e-4, e2 = 3.33e-12, e2 / e1^2 = 2.831e-4 s/rad, and the same 2.83e-4 at |b| = 0.1, 0.2
    and 1 rad/s: it is the constant of the quadratic convergence on this stream.  GN_CONSTANT is that figure rounded up to 3e-4: the
    GPU's different rounding moves e2 by ~1e-16, four orders below the 6 % of room."""
    seg, dt, gyro, acc = _solve_stream()
    ref = _motion_rots(cuda, dt, gyro, acc, seg)
    b = np.array([0.012, -0.016, 0.0])
    e1 = []
    for s in (1.0, 0.5):
        x1, Hn, rot, jac = _solve_once(cuda, dt, gyro + s * b, acc, seg, ref)
        e1.append(np.linalg.norm(x1 - s * b))
        assert np.array_equal(Hn, Hn.T) and np.linalg.eigvalsh(Hn).min() > 0
    # against the numpy normal equations on the same rows
    xr, Hr = solve_reference(jac.cpu().numpy(), [_quat_to_mat(q) for q in rot.cpu().numpy()], [_quat_to_mat(q) for q in ref.cpu().numpy()])
    assert np.abs(x1 - xr).max() <= 1e-9 * np.abs(xr).max() and np.abs(Hn - Hr).max() <= 1e-9 * np.abs(Hr).max()
    print('gyro bias solve: e1(b) %.4g e1(b/2) %.4g ratio %.4g' % (e1[0], e1[1], e1[0] / e1[1]))
    assert 3.0 < e1[0] / e1[1] < 5.0
    big = 25.0 * b
    x1 = _solve_once(cuda, dt, gyro + big, acc, seg, ref)[0]
    x2 = _solve_once(cuda, dt, gyro + big - x1, acc, seg, ref)[0]
    f1, f2 = np.linalg.norm(x1 - big), np.linalg.norm(x1 + x2 - big)
    print('gyro bias solve, |b| = 0.5: first round %.4g, second round %.4g = %.4g e1^2' % (f1, f2, f2 / f1 ** 2))
    assert f2 < GN_CONSTANT * f1 ** 2


def test_gyro_bias_solve_weights(cuda):
    """Rows of weight zero take no part, exactly as if they were not there: a corrupted rot_ref (a wrong rotation, a NaN) behind a zero
    weight gives the bits of the solve on the remaining rows alone.  All weights zero: ISLAM_ENOTPD and a zero estimate.  A corrupted
    row that does count is excluded and counted when its residual is not finite."""
    from islam_amd import _lib, ops
    seg, dt, gyro, acc = _solve_stream()
    ref = _motion_rots(cuda, dt, gyro, acc, seg)
    g1 = gyro + np.array([0.012, -0.016, 0.0])
    jac = ops.imu_preint_bias_jac(_t(cuda, dt), _t(cuda, g1), _t(cuda, acc), torch.tensor(seg, device=cuda), seg, True)
    rot = _motion_rots(cuda, dt, g1, acc, seg)
    n = len(seg) - 1
    bad_rows = np.array([0, 5, 17, 18, 40, n - 1])
    keep = np.setdiff1d(np.arange(n), bad_rows)
    kd = torch.tensor(keep, device=cuda)
    clean = ops.imu_gyro_bias_solve(jac[kd].contiguous(), rot[kd].contiguous(), ref[kd].contiguous())
    w = np.ones(n)
    w[bad_rows] = 0.0
    corrupt = ref.clone()
    corrupt[bad_rows[0]] = torch.tensor([0.5, 0.5, 0.5, 0.5], dtype=torch.float64, device=cuda)
    corrupt[bad_rows[1]] = float('nan')
    corrupt[bad_rows[2:]] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=cuda)
    got = ops.imu_gyro_bias_solve(jac, rot, corrupt, _t(cuda, w))
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1], clean[1]) and got[2] == 0
    # weights that are not all ones, against numpy
    w2 = np.random.default_rng(1).uniform(0.2, 3.0, n)
    x, H, _ = ops.imu_gyro_bias_solve(jac, rot, ref, _t(cuda, w2))
    xr, Hr = solve_reference(jac.cpu().numpy(), [_quat_to_mat(q) for q in rot.cpu().numpy()], [_quat_to_mat(q) for q in ref.cpu().numpy()], w2)
    assert np.abs(x.cpu().numpy() - xr).max() <= 1e-9 * np.abs(xr).max() and np.abs(H.cpu().numpy() - Hr).max() <= 1e-9 * np.abs(Hr).max()
    # a NaN row that counts is excluded and counted; the answer is the one without it
    one = np.ones(n)
    one[bad_rows[[0] + list(range(2, len(bad_rows)))]] = 0.0
    got = ops.imu_gyro_bias_solve(jac, rot, corrupt, _t(cuda, one))
    assert got[2] == 1 and torch.equal(got[0], clean[0])
    # all weights zero
    with pytest.raises(_lib.IslamHipError) as ei:
        ops.imu_gyro_bias_solve(jac, rot, ref, _t(cuda, np.zeros(n)))
    assert ei.value.code == -3 and 'islam_imu_gyro_bias_solve' in str(ei.value)
    out = torch.full((12,), 7.0, dtype=torch.float64, device=cuda)
    scratch = torch.empty(_lib.lib().islam_imu_gyro_bias_solve_scratch_bytes(n), dtype=torch.uint8, device=cuda)
    rc = _lib.lib().islam_imu_gyro_bias_solve(_lib.ptr(jac), _lib.ptr(rot), _lib.ptr(ref), _lib.ptr(_t(cuda, np.zeros(n))), n, _lib.ptr(out[0:3]),
                                             _lib.ptr(out[3:12]), _lib.ptr(scratch), 1, _lib.stream_ptr(cuda))
    assert rc == -3 and not out.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ 6. IMUModule
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_imu_module(cuda, dtype):
    from islam_amd import ops
    from islam_amd.imu_integrator import IMUModule
    tr = synthetic.car_trajectory(41, seed=3)
    bias = np.array([0.004, -0.002, 0.003])
    kw = dict(init=tr['init'], gravity=tr['gravity'], rgb2imu_sync=tr['rgb2imu_sync'], device='cuda:0', denoise_accel=False,
              denoise_gyro=False, dtype=dtype)
    st, end = 8, 16
    init = dict(pos=tr['init']['pos'], rot=tr['init']['rot'], vel=tr['init']['vel'])
    for prop_cov in (False, True):
        imu = IMUModule(tr['accels'], tr['gyros'], tr['imu_dts'], prop_cov=prop_cov, bias_jac=True, **kw)
        plain = IMUModule(tr['accels'], tr['gyros'], tr['imu_dts'], prop_cov=prop_cov, **kw)
        assert imu.last_bias_jac is None and plain.bias_jac is False
        b0 = int(tr['rgb2imu_sync'][st])
        seg = np.ascontiguousarray(tr['rgb2imu_sync'][st:end + 1] - b0, dtype=np.int64)
        sl = slice(b0, int(tr['rgb2imu_sync'][end]) + 1)
        want = {}
        for motion in (False, True):
            want[motion] = ops.imu_preint_bias_jac(imu.dts[sl, 0].contiguous(), imu.gyros[sl].contiguous(), imu.accels[sl].contiguous(),
                                                   torch.tensor(seg, device=cuda), seg, motion).to(dtype).cpu()
            got, ref = imu.integrate(st, end, init, motion_mode=motion), plain.integrate(st, end, init, motion_mode=motion)
            _same_tuple(got, ref, prop_cov)
            J = imu.last_bias_jac
            assert J.dtype == dtype and J.device.type == 'cpu' and tuple(J.shape) == (end - st + (0 if motion else 1), 9, 6)
            assert torch.equal(J, want[motion])
        both, refb = imu.integrate_both(st, end, init), plain.integrate_both(st, end, init)
        for g, r in zip(both, refb):
            _same_tuple(g, r, prop_cov)
        assert isinstance(imu.last_bias_jac, tuple) and torch.equal(imu.last_bias_jac[0], want[False]) and torch.equal(imu.last_bias_jac[1], want[True])
        assert plain.last_bias_jac is None
    # estimate_gyro_bias: the stream carries `bias`; the trusted rotations come from the clean stream
    clean = IMUModule(tr['accels'], tr['gyros'], tr['imu_dts'], **kw)
    ref_rots = clean.integrate(st, end, init, motion_mode=True)[1]
    start = np.array([0.001, 0.0, -0.001])
    imu = IMUModule(tr['accels'], tr['gyros'] + bias, tr['imu_dts'], gyro_bias=torch.tensor(start), bias_jac=True, **kw)
    before = (imu.gyro_bias.clone(), imu.gyros.clone(), imu.last_bias_jac, imu.optm_bias)
    est, H = imu.estimate_gyro_bias(st, end, ref_rots)
    assert torch.equal(imu.gyro_bias, before[0]) and torch.equal(imu.gyros, before[1]) and imu.last_bias_jac is before[2] and imu.optm_bias == before[3]
    assert est.dtype == torch.float64 and est.device.type == 'cpu' and tuple(H.shape) == (3, 3)
    # float64: the second-order term, at most |db| |db| T = 4e-3 * 4e-4.  float32: the ten quaternion products of a frame and the two
    # stored rotations round at 6e-8 per component, ~1e-6 rad on a residual, over T = 0.1 s: 1e-5 rad/s per row; five times that.
    tol = 2e-6 if dtype == torch.float64 else 5e-5
    print('estimate_gyro_bias %s: error %.3g' % (dtype, np.abs(est.numpy() - bias).max()))
    assert np.abs(est.numpy() - bias).max() <= tol
    est2, _ = imu.estimate_gyro_bias(st, end, ref_rots.tensor(), weight=np.ones(end - st))
    assert torch.equal(est, est2)


def _same_tuple(got, ref, prop_cov):
    assert len(got) == 4 and torch.equal(got[0], ref[0]) and torch.equal(got[1].tensor(), ref[1].tensor()) and torch.equal(got[3], ref[3])
    if prop_cov:
        assert torch.equal(got[2], ref[2])
    else:
        assert got[2] == [] and ref[2] == []
