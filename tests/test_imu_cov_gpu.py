"""GPU tests of the pre-integration covariance (islam_imu_preint_cov through islam_amd.ops, IMUModule(prop_cov=True)).

Reference: cov_reference below, a float64 numpy restatement of the recurrence include/islam_hip.h defines, one sample after the
other.  Error measure: for every entry |S - Sref|_ab <= 1e-9 sqrt(Sref_aa Sref_bb) (the Cauchy-Schwarz scale: rotation and
position variances differ by eleven orders of magnitude); 1e-9 is the project's float64 covariance tolerance
(tests/test_marginals_gpu.py).  The sequential float64 recurrence differs from the same recurrence in long double by 5.6e-13 of this
measure on the 5000-frame trajectory (50 000 samples, world rows), and a per-frame-then-compose association by 1.5e-13: the
reference sits three orders inside the bound whatever the association.  Entries whose scale is zero must be exactly zero."""
import numpy as np
import pytest
import torch

from islam_amd import synthetic

pytestmark = pytest.mark.gpu

GYRO_COV, ACC_COV = (1.6968e-4) ** 2, (2.0e-3) ** 2
TOL = 1e-9


def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _exp_jr(th):
    """Exp(th) and the right Jacobian Jr(th) of SO(3)."""
    t2 = float(th @ th)
    t = np.sqrt(t2)
    K = _hat(th)
    if t > 1e-5:
        A, B, C = np.sin(t) / t, 2.0 * np.sin(0.5 * t) ** 2 / t2, (t - np.sin(t)) / (t2 * t)
    else:
        A, B, C = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
    K2 = K @ K
    return np.eye(3) + A * K + B * K2, np.eye(3) - B * K + C * K2


def cov_reference(dt, gyro, acc, seg, gyro_cov, acc_cov, motion, init_cov=None):
    """Sigma <- A Sigma A^T + Bg diag(sg) Bg^T + Ba diag(sa) Ba^T sample by sample (float64).  gyro_cov / acc_cov: a scalar, three
    values or an (S, 3) array.  motion: nframes rows, every frame from Sigma = 0, DR = I; else nframes + 1 rows, row 0 = init_cov,
    row k over all samples [seg[0], seg[k]) with DR accumulated since seg[0]."""
    dt, gyro, acc = np.asarray(dt, np.float64), np.asarray(gyro, np.float64), np.asarray(acc, np.float64)
    S = len(dt)
    sg = np.broadcast_to(np.asarray(gyro_cov, np.float64), (S, 3))
    sa = np.broadcast_to(np.asarray(acc_cov, np.float64), (S, 3))
    n = len(seg) - 1
    out = np.zeros((n if motion else n + 1, 9, 9))
    Sig = np.zeros((9, 9)) if init_cov is None or motion else np.array(init_cov, dtype=np.float64)
    DR = np.eye(3)
    if not motion:
        out[0] = Sig
    I3 = np.eye(3)
    for i in range(n):
        if motion:
            Sig, DR = np.zeros((9, 9)), np.eye(3)
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
            Bg = np.zeros((9, 3))
            Bg[0:3] = Jr * d
            Ba = np.zeros((9, 3))
            Ba[3:6] = DR * d
            Ba[6:9] = 0.5 * DR * d * d
            Sig = A @ Sig @ A.T + (Bg * sg[j]) @ Bg.T + (Ba * sa[j]) @ Ba.T
            DR = DR @ dr
        out[i + (0 if motion else 1)] = Sig
    return out


def cs_error(S, ref):
    """max over entries of |S - ref| / sqrt(ref_aa ref_bb); entries with a zero scale must be exactly zero (inf otherwise)."""
    S, ref = np.asarray(S), np.asarray(ref)
    dg = np.sqrt(np.maximum(np.diagonal(ref, axis1=-2, axis2=-1), 0.0))
    scale = dg[..., :, None] * dg[..., None, :]
    err = np.abs(S - ref)
    if np.any(err[scale == 0] != 0):
        return np.inf
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0), initial=0.0))


def _check_rows(out):
    """Exactly symmetric, positive semi-definite after scaling to unit diagonal."""
    assert np.array_equal(out, np.swapaxes(out, -1, -2))
    for S in out:
        d = np.diag(S)
        if not d.all():
            assert not S[d == 0].any() and not S[:, d == 0].any()
        k = d > 0
        if k.any():
            s = 1.0 / np.sqrt(d[k])
            assert np.linalg.eigvalsh(S[np.ix_(k, k)] * s[:, None] * s[None, :]).min() >= -TOL


def _run(cuda, dt, gyro, acc, seg, motion, dtype=np.float64, gyro_cov=GYRO_COV, acc_cov=ACC_COV, init_cov=None, per_sample=None):
    from islam_amd import ops
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=dtype), dtype=td, device=cuda)
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    ic = None if init_cov is None else torch.tensor(init_cov, dtype=torch.float64, device=cuda)
    gs, as_ = (None, None) if per_sample is None else (t(per_sample[0]), t(per_sample[1]))
    out = ops.imu_preint_cov(t(dt), t(gyro), t(acc), torch.tensor(seg, device=cuda), seg, gyro_cov, acc_cov, motion, ic, gs, as_)
    assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (len(seg) - (1 if motion else 0), 9, 9)
    return out.cpu().numpy()


def _rounded(a, dtype):
    return np.asarray(a, dtype=dtype).astype(np.float64)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('motion', [False, True])
@pytest.mark.parametrize('frames,per', [(2, 10), (9, 10), (9, 1), (33, 7), (5, 70), (4, 200)])
def test_against_the_restatement(cuda, dtype, motion, frames, per):
    tr = synthetic.car_trajectory(frames, imu_per_frame=per, seed=frames + per)
    seg = tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0]
    out = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, dtype)
    want = cov_reference(_rounded(tr['imu_dts'], dtype), _rounded(tr['gyros'], dtype), _rounded(tr['accels'], dtype), seg, GYRO_COV, ACC_COV, motion)
    e = cs_error(out, want)
    print('cov (%d, %d) %s %s: %.3g' % (frames, per, 'motion' if motion else 'world', np.dtype(dtype).name, e))
    assert e <= TOL
    _check_rows(out)
    if dtype == np.float32:
        # the float32 module returns the float64 rows of the kernel cast to float32
        from islam_amd.imu_integrator import IMUModule
        imu = IMUModule(tr['accels'], tr['gyros'], tr['imu_dts'], init=tr['init'], gravity=tr['gravity'], rgb2imu_sync=tr['rgb2imu_sync'],
                        device='cuda:0', denoise_accel=False, denoise_gyro=False, dtype=torch.float32, prop_cov=True)
        covs = imu.integrate(0, frames - 1, tr['init'], motion_mode=motion)[2]
        assert covs.dtype == torch.float32 and torch.equal(covs, torch.from_numpy(out).to(torch.float32))


def _ragged():
    rng = np.random.default_rng(0)
    counts = np.array([3, 0, 11, 1, 0, 0, 25, 2])
    seg = np.concatenate([[0], np.cumsum(counts)])
    S = int(seg[-1])
    dt = rng.uniform(0.004, 0.012, S)
    gyro = rng.normal(0, 0.5, (S, 3))
    gyro[0] = 0.0                       # theta == 0 -> Taylor branch of Jr
    gyro[5] = [400.0, -250.0, 90.0]     # |theta| > pi
    acc = rng.normal(0, 1.0, (S, 3)) + np.array([0, 0, 9.81])
    return counts, seg, dt, gyro, acc


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_ragged_and_empty_intervals(cuda, dtype):
    counts, seg, dt, gyro, acc = _ragged()
    r = lambda a: _rounded(a, dtype)
    for motion in (False, True):
        out = _run(cuda, dt, gyro, acc, seg, motion, dtype)
        want = cov_reference(r(dt), r(gyro), r(acc), seg, GYRO_COV, ACC_COV, motion)
        assert cs_error(out, want) <= TOL
        _check_rows(out)
        for i, c in enumerate(counts):
            if c == 0:
                if motion:
                    assert not out[i].any()
                else:
                    assert np.array_equal(out[i + 1], out[i])
    # a stream that starts with frames without samples: they repeat row 0
    seg2 = np.concatenate([[0, 0, 0], seg])
    S0 = _spd(3)
    out = _run(cuda, dt, gyro, acc, seg2, False, dtype, init_cov=S0)
    assert np.array_equal(out[0], S0) and np.array_equal(out[1], S0) and np.array_equal(out[2], S0)
    assert cs_error(out, cov_reference(r(dt), r(gyro), r(acc), seg2, GYRO_COV, ACC_COV, False, S0)) <= TOL
    # no frames at all: world mode returns init_cov alone, motion mode nothing
    assert np.array_equal(_run(cuda, dt, gyro, acc, np.array([0]), False, dtype, init_cov=S0), S0[None])
    assert _run(cuda, dt, gyro, acc, np.array([0]), True, dtype).shape == (0, 9, 9)


def _spd(seed):
    L = np.random.default_rng(seed).normal(0, 1e-3, (9, 9))
    S = L @ L.T
    return 0.5 * (S + S.T)


def test_full_size_5000_frames(cuda):
    """5000 frame intervals / 50 001 samples: three scan levels in world mode; a second call is bit-equal (no atomics, fixed order)."""
    tr = synthetic.car_trajectory(5001)
    seg = tr['rgb2imu_sync']
    assert len(seg) == 5001 and len(tr['imu_dts']) == 50001
    for motion in (False, True):
        out = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion)
        again = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion)
        assert np.array_equal(out, again)
        want = cov_reference(tr['imu_dts'], tr['gyros'], tr['accels'], seg, GYRO_COV, ACC_COV, motion)
        e = cs_error(out, want)
        print('cov 5000 frames %s: %.3g' % ('motion' if motion else 'world', e))
        assert e <= TOL
        _check_rows(out)


def test_ragged_frames_across_the_scan_blocks(cuda):
    """Frames without samples at the borders of the 64-frame scan blocks, a last block that is not full, two scan levels."""
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
    S0 = _spd(9)
    out = _run(cuda, dt, gyro, acc, seg, False, init_cov=S0)
    assert cs_error(out, cov_reference(dt, gyro, acc, seg, GYRO_COV, ACC_COV, False, S0)) <= TOL
    _check_rows(out)
    for i in np.nonzero(counts == 0)[0]:
        assert np.array_equal(out[i + 1], out[i])
    out = _run(cuda, dt, gyro, acc, seg, True)
    assert cs_error(out, cov_reference(dt, gyro, acc, seg, GYRO_COV, ACC_COV, True)) <= TOL
    assert not out[counts == 0].any()


@pytest.mark.parametrize('frames,per', [(9, 10), (200, 7)])
def test_initial_covariance_is_transported(cuda, frames, per):
    """sigma = 0: world row k is Phi_k Sigma_0 Phi_k^T."""
    tr = synthetic.car_trajectory(frames, imu_per_frame=per, seed=11)
    seg = tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0]
    S0 = _spd(frames)
    out = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, False, gyro_cov=0.0, acc_cov=0.0, init_cov=S0)
    want = cov_reference(tr['imu_dts'], tr['gyros'], tr['accels'], seg, 0.0, 0.0, False, S0)
    assert np.array_equal(out[0], S0)
    assert cs_error(out, want) <= TOL
    _check_rows(out)
    # motion rows ignore it, and without noise they are zero
    assert not _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, True, gyro_cov=0.0, acc_cov=0.0).any()


@pytest.mark.parametrize('motion', [False, True])
def test_linear_in_the_variances(cuda, motion):
    """Scaling both variances by c scales the rows by c.  c = 4 scales every intermediate exactly: bit-equal.  A general c rounds the
    variances and every sum differently, and entries that are small by cancellation carry the rounding of their large terms: the
    difference is measured against the Cauchy-Schwarz scale, rtol 1e-12 (4500 float64 roundings; a row is < 30 dependent joins)."""
    tr = synthetic.car_trajectory(33, imu_per_frame=7, seed=2)
    seg = tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0]
    g3, a3 = np.array([1.0, 2.0, 0.5]) * GYRO_COV, np.array([0.7, 1.0, 3.0]) * ACC_COV
    base = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, gyro_cov=g3, acc_cov=a3)
    x4 = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, gyro_cov=4.0 * g3, acc_cov=4.0 * a3)
    np.testing.assert_allclose(x4, 4.0 * base, rtol=1e-12, atol=0.0)
    c = 3.7
    xc = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, gyro_cov=c * g3, acc_cov=c * a3)
    assert cs_error(xc, c * base) <= 1e-12
    # and the three variances of a sensor are not mixed up
    assert cs_error(base, cov_reference(tr['imu_dts'], tr['gyros'], tr['accels'], seg, g3, a3, motion)) <= TOL


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('motion', [False, True])
def test_per_sample_variances(cuda, dtype, motion):
    tr = synthetic.car_trajectory(9, imu_per_frame=10, seed=4)
    seg = tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0]
    S = len(tr['imu_dts'])
    const = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, dtype)
    arr = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, dtype, gyro_cov=1.0, acc_cov=1.0,
               per_sample=(np.full((S, 3), GYRO_COV), np.full((S, 3), ACC_COV)))
    if dtype == np.float64:
        assert cs_error(arr, const) <= TOL
    else:       # the arrays are float32 like the samples: the constants rounded to float32 are what the kernel sees
        want = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, dtype, gyro_cov=float(np.float32(GYRO_COV)),
                    acc_cov=float(np.float32(ACC_COV)))
        assert cs_error(arr, want) <= TOL
    # arrays that do vary
    rng = np.random.default_rng(8)
    gs, as_ = GYRO_COV * rng.uniform(0.5, 2.0, (S, 3)), ACC_COV * rng.uniform(0.5, 2.0, (S, 3))
    out = _run(cuda, tr['imu_dts'], tr['gyros'], tr['accels'], seg, motion, dtype, per_sample=(gs, as_))
    r = lambda a: _rounded(a, dtype)
    assert cs_error(out, cov_reference(r(tr['imu_dts']), r(tr['gyros']), r(tr['accels']), seg, r(gs), r(as_), motion)) <= TOL


def _quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize('per', [10, 70])
def test_consistent_with_the_integrator(cuda, per):
    """The covariance is J diag(sigma) J^T of the integrator that ships: one frame, identity initial rotation, gravity 0 (the forward
    subtracts gravity in a gyro-dependent body frame, which is not part of this error model).  J = the Jacobian of
    ops.imu_preint(motion_mode=True)'s (rot, vel, pos) w.r.t. every gyro / accelerometer sample, from islam_imu_preint_bwd with nine
    unit cotangents; its rotation rows are LEFT tangents, dphi_right = DR^T dphi_left.  Bound 1e-6 of the Cauchy-Schwarz scale: the
    two are the same first-order quantity (differences: rounding), while a convention error (Jl for Jr, a sign, a frame) is of order
    |w d| ~ 1e-3 or larger."""
    from islam_amd import ops
    tr = synthetic.car_trajectory(2, imu_per_frame=per, seed=per)
    seg = np.ascontiguousarray(tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0], dtype=np.int64)
    S = int(seg[-1])
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=cuda)
    dt = t(tr['imu_dts'][:S])
    gyro, acc = t(tr['gyros'][:S]).requires_grad_(True), t(tr['accels'][:S]).requires_grad_(True)
    z3, q0 = t(np.zeros(3)), t(np.array([0.0, 0.0, 0.0, 1.0]))
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
    g3, a3 = np.array([1.0, 2.0, 0.5]) * GYRO_COV, np.array([0.7, 1.0, 3.0]) * ACC_COV
    SJ = np.einsum('asi,i,bsi->ab', Jg, g3, Jg) + np.einsum('asi,i,bsi->ab', Ja, a3, Ja)
    out = _run(cuda, tr['imu_dts'][:S], tr['gyros'][:S], tr['accels'][:S], seg, True, gyro_cov=g3, acc_cov=a3)
    e = cs_error(out[0], SJ)
    print('cov vs J sigma J^T (%d samples): %.3g' % (S, e))
    assert e <= 1e-6


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_imu_module(cuda, dtype):
    from islam_amd.imu_integrator import IMUModule
    tr = synthetic.car_trajectory(41, seed=3)
    kw = dict(init=tr['init'], gravity=tr['gravity'], rgb2imu_sync=tr['rgb2imu_sync'], device='cuda:0', denoise_accel=False,
              denoise_gyro=False, dtype=dtype)
    imu = IMUModule(tr['accels'], tr['gyros'], tr['imu_dts'], prop_cov=True, **kw)
    st, end = 8, 16
    init = dict(pos=tr['init']['pos'], rot=tr['init']['rot'], vel=tr['init']['vel'])
    S0 = _spd(1)
    w, m = imu.integrate_both(st, end, init, init_cov=S0)
    rw = imu.integrate(st, end, init, motion_mode=False, init_cov=S0)
    rm = imu.integrate(st, end, init, motion_mode=True)
    for got, ref, rows in ((w, rw, end - st + 1), (m, rm, end - st)):
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].tensor(), ref[1].tensor()) and torch.equal(got[3], ref[3])
        assert torch.equal(got[2], ref[2])
        assert tuple(got[2].shape) == (rows, 9, 9) and got[2].device.type == 'cpu' and got[2].dtype == dtype
    assert torch.equal(w[2][0], torch.from_numpy(S0).to(dtype))
    b0 = int(tr['rgb2imu_sync'][st])
    seg = tr['rgb2imu_sync'][st:end + 1] - b0
    sl = slice(b0, int(tr['rgb2imu_sync'][end]) + 1)
    npd = np.float64 if dtype == torch.float64 else np.float32
    r = lambda a: _rounded(a[sl], npd)
    want = cov_reference(r(tr['imu_dts']), r(tr['gyros']), r(tr['accels']), seg, GYRO_COV, ACC_COV, False, S0)
    tol = TOL if dtype == torch.float64 else 4 * np.finfo(np.float32).eps         # the float32 module rounds the rows once
    assert cs_error(w[2].double().numpy(), want) <= tol
    # the default stays what the reference returns
    plain = IMUModule(tr['accels'], tr['gyros'], tr['imu_dts'], **kw)
    assert plain.integrate(st, end, init)[2] == [] and plain.integrate_both(st, end, init)[0][2] == []
    ref = plain.integrate(st, end, init)
    assert torch.equal(ref[0], rw[0]) and torch.equal(ref[3], rw[3])
