"""GPU tests of the gravity / accelerometer-bias / velocity solve (islam_imu_gravity_bias_solve through islam_amd.ops and
IMUModule.estimate_gravity_accel_bias).

Reference: align_reference below, a float64 numpy restatement written pair by pair from the definition in include/islam_hip.h, solved
by numpy.linalg.solve on the normal equations, with the same four gravity-norm rounds.  Planted truth: planted_stream propagates a world
trajectory with the shipped discretisation (p += v d + (R a + g) d^2 / 2, v += (R a + g) d, R <- R Exp(w d)); the increments come from
integrate_reference on the samples a + b_planted.  In this discretisation (P_i) and (V_i) hold exactly and the increments are linear in the
accelerometer bias, so g, b_planted and every v_i are recovered to rounding times conditioning.

Tolerances are measured, not fixed: for every stream the restatement's own error against the planted truth is taken first; the library
is held to 10 x that against the planted truth and against the restatement, with a floor of 1e-12 relative to |g| resp. max |b| (resp.
max |v|) -- the margin covers a different summation order.  H against the restatement: 1e-9 sqrt(H_aa H_bb) per entry, the float64
bound of tests/test_imu_cov_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests.test_imu_bias_jac_gpu import integrate_reference, jac_reference
from tests.test_imu_cov_gpu import ACC_COV, GYRO_COV, _exp_jr, _quat_to_mat, _rounded

pytestmark = pytest.mark.gpu

G_PLANTED = np.array([0.9, -1.7, -9.6])              # |g| = 9.79, tilted against every axis
B_PLANTED = np.array([0.12, -0.05, 0.08])
RAGGED12 = (3, 11, 1, 6, 140, 2, 9, 5, 10, 4, 7, 8)   # 12 frames, one long one
SHAPES = {'4x7': ((7,) * 4, 1.0), '12xragged': (RAGGED12, 1.0), '70x10': ((10,) * 70, 1.0), '300x10': ((10,) * 300, 0.5),
          '1100x4': ((4,) * 1100, 0.5)}
# P = 1024 and P = 1025 pairs: the last size the solve kernel sums by itself and the first with a partial-sum launch (csrc/imu_terms.h)
REACH_SHAPES = {'1025x4': ((4,) * 1025, 0.5), '1026x4': ((4,) * 1026, 0.5)}


def _mat_to_quat(R):
    """xyzw of a rotation matrix (w >= 0 branch is enough here: the planted rotations stay below pi)."""
    w = 0.5 * np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 0.0))
    assert w > 0.1
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def make_stream(counts, amp=1.0, bias=B_PLANTED, seed=0, tail=0):
    """Samples of a planted trajectory: dt ~ 5 ms, a sinusoidal gyro of amplitude `amp` rad/s, a smooth specific force.  Returns the
    measured samples (the accelerometer carries `bias`), the frame offsets and the world states (R, p, v) at every frame border.
    `tail` extra samples follow the last frame (IMUModule slices one sample past the last border)."""
    rng = np.random.default_rng(seed)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S = int(seg[-1]) + tail
    dt = rng.uniform(0.0045, 0.0055, S)
    t = np.cumsum(dt) - dt
    gyro = amp * np.stack([np.sin(1.3 * t + 0.2), np.sin(0.7 * t + 1.1), np.sin(2.1 * t + 0.5)], 1)
    acc = np.stack([1.5 * np.sin(0.9 * t), 0.8 * np.cos(1.7 * t + 0.3), 9.6 + 0.5 * np.sin(0.4 * t)], 1) + rng.normal(0, 0.2, (S, 3))
    R, p, v = _exp_jr(np.array([0.3, -0.5, 0.8]))[0], np.array([1.0, -2.0, 0.5]), np.array([0.7, 0.2, -0.1])
    Rs, ps, vs = [], [], []
    for j in range(int(seg[-1])):
        if j in seg[:-1]:
            for _ in range(int(np.sum(seg[:-1] == j))):
                Rs.append(R); ps.append(p); vs.append(v)
        d = dt[j]
        a = R @ acc[j] + G_PLANTED
        p = p + v * d + 0.5 * a * d * d
        v = v + a * d
        R = R @ _exp_jr(gyro[j] * d)[0]
    Rs.append(R); ps.append(p); vs.append(v)
    return dict(seg=seg, dt=dt, gyro=gyro, acc=acc + np.asarray(bias), R=np.stack(Rs), p=np.stack(ps), v=np.stack(vs))


@functools.lru_cache(maxsize=None)
def planted_stream(name, bias=True):
    """The solve's inputs for one of SHAPES or REACH_SHAPES, in float64: quaternions and positions of the poses, durations, increments in the
    start-body frame, bias Jacobians; and the planted g, b, v."""
    counts, amp = SHAPES[name] if name in SHAPES else REACH_SHAPES[name]
    s = make_stream(counts, amp, B_PLANTED if bias else np.zeros(3), seed=len(counts))
    seg, n = s['seg'], len(counts)
    d, dv, dp = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        sl = slice(int(seg[i]), int(seg[i + 1]))
        d[i] = s['dt'][sl].sum()
        _, dv[i], dp[i] = integrate_reference(s['dt'][sl], s['gyro'][sl], s['acc'][sl])
    jac = jac_reference(s['dt'], s['gyro'], s['acc'], seg, True)
    out = dict(s, quat=np.stack([_mat_to_quat(R) for R in s['R']]), d=d, dv=dv, dp=dp, jac=jac, g=G_PLANTED,
               b=B_PLANTED if bias else np.zeros(3))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def align_reference(quat, p, d, dv, dp, jac=None, cov=None, weight=None, gravity_norm=None):
    """(x (6), H (6, 6), vel (n + 1, 3), excluded) from the definition, pair by pair, float64."""
    quat, p, d, dv, dp = (np.asarray(a, np.float64) for a in (quat, p, d, dv, dp))
    n = len(d)
    nu = 6 if jac is not None else 3
    R = [_quat_to_mat(q) for q in quat]
    H, c, bad = np.zeros((6, 6)), np.zeros(6), 0
    I3 = np.eye(3)
    with np.errstate(all='ignore'):
        for i in range(n - 1):
            w = 1.0 if weight is None else weight[i]
            if w == 0:
                continue
            A = np.zeros((3, 6))
            A[:, 0:3] = -0.5 * (d[i] + d[i + 1]) * I3
            if jac is not None:
                Jv0, Jp0, Jp1 = jac[i][3:6, 3:6], jac[i][6:9, 3:6], jac[i + 1][6:9, 3:6]
                A[:, 3:6] = R[i] @ Jp0 / d[i] - R[i + 1] @ Jp1 / d[i + 1] - R[i] @ Jv0
            r = (p[i + 1] - p[i]) / d[i] - (p[i + 2] - p[i + 1]) / d[i + 1] + R[i + 1] @ dp[i + 1] / d[i + 1] - R[i] @ dp[i] / d[i] + R[i] @ dv[i]
            ok = np.isfinite(w) and d[i] > 0 and d[i + 1] > 0 and np.isfinite(A).all() and np.isfinite(r).all()
            L = I3
            if ok and cov is not None:
                S0, S1 = cov[i], cov[i + 1]
                C = R[i + 1] @ S1[6:9, 6:9] @ R[i + 1].T / d[i + 1] ** 2 + \
                    R[i] @ (S0[6:9, 6:9] / d[i] ** 2 - (S0[6:9, 3:6] + S0[3:6, 6:9]) / d[i] + S0[3:6, 3:6]) @ R[i].T
                try:
                    L = np.linalg.cholesky(0.5 * (C + C.T))
                except np.linalg.LinAlgError:
                    ok = False
            if not ok:
                bad += 1
                continue
            Aw, rw = np.linalg.solve(L, A), np.linalg.solve(L, r)
            H += w * Aw.T @ Aw
            c += w * Aw.T @ rw
    x = np.zeros(6)
    x[:nu] = np.linalg.solve(H[:nu, :nu], c[:nu])
    if gravity_norm:
        G = float(gravity_norm)
        gh = x[0:3] / np.linalg.norm(x[0:3])
        for _ in range(4):
            e = np.zeros(3)
            e[int(np.argmin(np.abs(gh)))] = 1.0            # (argmin takes the lowest index on a tie)
            b1 = e - (e @ gh) * gh
            b1 /= np.linalg.norm(b1)
            b2 = np.cross(gh, b1)
            B = np.zeros((nu, nu - 1))
            B[0:3, 0], B[0:3, 1] = b1, b2
            B[3:, 2:] = np.eye(nu - 3)
            x0 = np.zeros(nu)
            x0[0:3] = G * gh
            z = np.linalg.solve(B.T @ H[:nu, :nu] @ B, B.T @ (c[:nu] - H[:nu, :nu] @ x0))
            gn = x0[0:3] + b1 * z[0] + b2 * z[1]
            gh = gn / np.linalg.norm(gn)
        x[0:3] = G * gh
        x[3:nu] = z[2:]
    g, b = x[0:3], x[3:6]
    vel = np.full((n + 1, 3), np.nan)
    for i in range(n + 1):
        k = i if i < n and d[i] > 0 else (i - 1 if i > 0 and d[i - 1] > 0 else -1)
        if k < 0:
            continue
        ddp = dp[k] + (jac[k][6:9, 3:6] @ b if jac is not None else 0.0)
        vel[i] = (p[k + 1] - p[k] - 0.5 * g * d[k] ** 2 - R[k] @ ddp) / d[k]
        if k != i:
            vel[i] = vel[i] + g * d[k] + R[k] @ (dv[k] + (jac[k][3:6, 3:6] @ b if jac is not None else 0.0))
    return x, H, vel, bad


def errors(x, vel, st):
    """(|g - g_planted|, |b - b_planted|, |v - v_planted|), the largest component each"""
    return np.array([np.abs(x[0:3] - st['g']).max(), np.abs(x[3:6] - st['b']).max(), np.abs(vel - st['v']).max()])


def bounds(ref_err, st):
    """10 x the restatement's own error, floor 1e-12 of |g|, max |b| (|g| where nothing is planted in b), max |v|"""
    scale = np.array([np.linalg.norm(st['g']), np.abs(st['b']).max() or np.linalg.norm(st['g']), np.abs(st['v']).max()])
    return np.maximum(10.0 * ref_err, 1e-12 * scale)


def h_error(H, ref):
    dg = np.sqrt(np.diag(ref))
    scale = dg[:, None] * dg[None, :]
    err = np.abs(H - ref)
    if np.any(err[scale == 0] != 0):
        return np.inf
    return float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)))


def _t(cuda, a, dtype=np.float64):
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), dtype=td, device=cuda)


def _solve(cuda, st, dtype=np.float64, jac=True, cov=None, weight=None, gravity_norm=None, dp=None, d=None):
    """ops.imu_gravity_bias_solve on a planted stream -> (x, H, vel, excluded) as numpy"""
    from islam_amd import ops
    a = (_t(cuda, st['quat'], dtype), _t(cuda, st['p'], dtype), _t(cuda, st['d'] if d is None else d, dtype), _t(cuda, st['dv'], dtype),
         _t(cuda, st['dp'] if dp is None else dp, dtype))
    g, b, H, vel, bad = ops.imu_gravity_bias_solve(*a, _t(cuda, st['jac']) if jac else None, None if cov is None else _t(cuda, cov),
                                                   None if weight is None else _t(cuda, weight), gravity_norm)
    n = len(st['d'])
    assert g.is_cuda and g.dtype == torch.float64 and tuple(H.shape) == (6, 6) and tuple(vel.shape) == (n + 1, 3)
    return np.concatenate([g.cpu().numpy(), b.cpu().numpy()]), H.cpu().numpy(), vel.cpu().numpy(), bad


def _reference(st, dtype=np.float64, jac=True, cov=None, weight=None, gravity_norm=None):
    r = lambda a: _rounded(a, dtype)
    return align_reference(r(st['quat']), r(st['p']), r(st['d']), r(st['dv']), r(st['dp']), st['jac'] if jac else None, cov, weight, gravity_norm)


def _check(tag, got, ref, st, h_tol=1e-9):
    """library against the planted truth and against the restatement, under the measured bounds; prints every figure first"""
    x, H, vel, bad = got
    xr, Hr, velr, badr = ref
    e_ref, e_lib = errors(xr, velr, st), errors(x, vel, st)
    tol = bounds(e_ref, st)
    par = np.array([np.abs(x[0:3] - xr[0:3]).max(), np.abs(x[3:6] - xr[3:6]).max(), np.abs(vel - velr).max()])
    he = h_error(H, Hr)
    print('%s: restatement vs planted %s, library vs planted %s, library vs restatement %s, bound %s, H %.3g, cond(H) %.3g'
          % (tag, e_ref, e_lib, par, tol, he, np.linalg.cond(Hr[:3, :3] if not Hr[3, 3] else Hr)))
    assert bad == badr
    assert np.all(e_lib <= tol), (e_lib, tol)
    assert np.all(par <= tol), (par, tol)
    assert he <= h_tol and np.array_equal(H, H.T)


# ------------------------------------------------------------------------------------------------ 1. parity and recovery
@pytest.mark.parametrize('name,dtype', [(n, d) for n in SHAPES for d in (np.float64, np.float32)] + [(n, np.float64) for n in REACH_SHAPES])
def test_against_the_restatement_and_the_planted_truth(cuda, name, dtype):
    st = planted_stream(name)
    got = _solve(cuda, st, dtype)
    _check('%s %s' % (name, np.dtype(dtype).name), got, _reference(st, dtype), st)
    again = _solve(cuda, st, dtype)                       # a second call: the same bits, velocities included
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and again[3] == got[3] == 0


@pytest.mark.parametrize('name', ['4x7', '70x10', '1100x4'])
def test_without_jacobians(cuda, name):
    """No Jacobians: three unknowns, b exactly 0.0.  The stream carries no accelerometer bias, so g and the velocities are still the
    planted ones and the measured bound means what it means elsewhere."""
    st = planted_stream(name, bias=False)
    got = _solve(cuda, st, jac=False)
    assert np.array_equal(got[0][3:6], np.zeros(3)) and not np.signbit(got[0][3:6]).any()
    assert not got[1][3:6, :].any() and not got[1][:, 3:6].any()
    _check('%s no jac' % name, got, _reference(st, jac=False), st)


# ------------------------------------------------------------------------------------------------ 2. covariances
def _motion_cov(cuda, st, dtype=np.float64):
    from islam_amd import ops
    seg = np.ascontiguousarray(st['seg'], dtype=np.int64)
    S = int(seg[-1])
    return ops.imu_preint_cov(_t(cuda, st['dt'][:S], dtype), _t(cuda, st['gyro'][:S], dtype), _t(cuda, st['acc'][:S], dtype),
                              torch.tensor(seg, device=cuda), seg, GYRO_COV, ACC_COV, True).cpu().numpy()


@pytest.mark.parametrize('name,dtype', [('12xragged', np.float64), ('70x10', np.float32), ('300x10', np.float64), ('1100x4', np.float64)])
def test_with_covariances(cuda, name, dtype):
    """cov from ops.imu_preint_cov (motion rows): parity with the restatement's whitened solve, H = sum A^T C^-1 A; the planted values
    are still recovered (the equations are consistent, whatever the weights).  All S_i scaled by 4: x unchanged to 1e-12 relative, H
    divided by 4 to rounding (1e-12 of sqrt(H_aa H_bb): the scaling by 4 itself is exact, the Cholesky factors differ by rounding)."""
    st = planted_stream(name)
    cov = _motion_cov(cuda, st, dtype)
    got = _solve(cuda, st, dtype, cov=cov)
    _check('%s %s cov' % (name, np.dtype(dtype).name), got, _reference(st, dtype, cov=cov), st)
    x4, H4, vel4, bad4 = _solve(cuda, st, dtype, cov=4.0 * cov)
    print('cov x 4: x moves by %.3g relative, H / 4 by %.3g' % (np.abs(x4 - got[0]).max() / np.abs(got[0]).max(), h_error(4.0 * H4, got[1])))
    assert bad4 == 0 and np.abs(x4 - got[0]).max() <= 1e-12 * np.abs(got[0]).max()
    assert h_error(4.0 * H4, got[1]) <= 1e-12


# ------------------------------------------------------------------------------------------------ 3. gravity of known magnitude
# ('4x7', False): three pairs and three unknowns, the 2 x 2 projected system: the rounds' loops over "the rest of M" run zero times
@pytest.mark.parametrize('name,jac', [('4x7', True), ('4x7', False), ('70x10', True), ('70x10', False), ('1100x4', True)])
def test_gravity_norm(cuda, name, jac):
    st = planted_stream(name, bias=jac)
    G = float(np.linalg.norm(G_PLANTED))
    got = _solve(cuda, st, jac=jac, gravity_norm=G)
    print('|g| - G = %.3g' % (np.linalg.norm(got[0][0:3]) - G))
    # g = G gh: gh is normalised (two roundings of its norm), scaled (half of one) and its norm is taken here (two more): 8 eps
    assert abs(np.linalg.norm(got[0][0:3]) - G) <= 8 * np.finfo(np.float64).eps * G
    _check('%s norm' % name, got, _reference(st, jac=jac, gravity_norm=G), st)
    # a wrong magnitude (1 % off): the norm is still G, and the result is the restatement's (same bound; the planted values are not
    # what this problem's minimum is, so only the parity is asked)
    Gw = 1.01 * G
    x, H, vel, bad = _solve(cuda, st, jac=jac, gravity_norm=Gw)
    xr, Hr, velr, _ = _reference(st, jac=jac, gravity_norm=Gw)
    tol = bounds(errors(*_reference(st, jac=jac, gravity_norm=G)[0:3:2], st), st)
    par = np.array([np.abs(x[0:3] - xr[0:3]).max(), np.abs(x[3:6] - xr[3:6]).max(), np.abs(vel - velr).max()])
    print('wrong G: library vs restatement %s, bound %s' % (par, tol))
    assert bad == 0 and abs(np.linalg.norm(x[0:3]) - Gw) <= 8 * np.finfo(np.float64).eps * Gw
    assert np.all(par <= tol)
    if not jac:
        assert np.array_equal(x[3:6], np.zeros(3))


# ------------------------------------------------------------------------------------------------ 4. weights and exclusion
def test_weights_and_exclusion(cuda):
    from islam_amd import _lib, ops
    st = planted_stream('70x10')
    n = len(st['d'])
    rng = np.random.default_rng(3)
    w = rng.uniform(0.2, 3.0, n - 1)
    _check('70x10 weights', _solve(cuda, st, weight=w), _reference(st, weight=w), st)
    # weight 0 and a NaN in dpos of interval 20 (pairs 19 and 20 read it): nothing beyond what the zero weights do
    w0 = np.ones(n - 1)
    w0[[19, 20]] = 0.0
    dpn = st['dp'].copy()
    dpn[20, 1] = np.nan
    clean, dirty = _solve(cuda, st, weight=w0), _solve(cuda, st, weight=w0, dp=dpn)
    assert dirty[3] == 0 and clean[3] == 0
    assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1])
    keep = np.ones(n + 1, bool)
    keep[20] = False                                      # v_20 comes from (P_20), which reads the NaN; every other v_i does not
    assert np.array_equal(clean[2][keep], dirty[2][keep]) and np.isnan(dirty[2][20]).any()
    _check('70x10 zero weights', clean, _reference(st, weight=w0), st)
    # the same NaN with weight 1 on pair 20 only: excluded and counted, the rest still solves
    w1 = np.ones(n - 1)
    w1[19] = 0.0
    got = _solve(cuda, st, weight=w1, dp=dpn)
    assert got[3] == 1 and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    # a frame without samples (d = 0, no increments): its two pairs are excluded
    d0 = st['d'].copy()
    d0[33] = 0.0
    got = _solve(cuda, st, d=d0)
    wx = np.ones(n - 1)
    wx[[32, 33]] = 0.0
    want = _solve(cuda, st, weight=wx)
    assert got[3] == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # all weights zero: ISLAM_ENOTPD with the entry point's name; at the C level x and vel are zeros and H is written
    with pytest.raises(_lib.IslamHipError) as ei:
        _solve(cuda, st, weight=np.zeros(n - 1))
    assert ei.value.code == -3 and 'islam_imu_gravity_bias_solve' in str(ei.value)
    for rows, wz in ((n, np.zeros(n - 1)), (1, None)):
        out = torch.full((42 + 3 * (rows + 1),), 7.0, dtype=torch.float64, device=cuda)
        scratch = torch.empty(_lib.lib().islam_imu_gravity_bias_solve_scratch_bytes(rows), dtype=torch.uint8, device=cuda)
        a = [_t(cuda, st[k][:rows + (1 if k in ('quat', 'p') else 0)]) for k in ('quat', 'p', 'd', 'dv', 'dp', 'jac')]
        wt = None if wz is None else _t(cuda, wz)
        rc = _lib.lib().islam_imu_gravity_bias_solve(*[_lib.ptr(t) for t in a], None, _lib.ptr(wt), rows, 0.0, _lib.ptr(out[0:6]),
                                                     _lib.ptr(out[6:42]), _lib.ptr(out[42:]), _lib.ptr(scratch), 1, _lib.stream_ptr(cuda))
        assert rc == -3 and not out.cpu().numpy().any()
        with pytest.raises(_lib.IslamHipError) as ei:
            ops.imu_gravity_bias_solve(*a[:5], a[5], None, wt)
        assert ei.value.code == -3


# ------------------------------------------------------------------------------------------------ 5. IMUModule
def test_imu_module(cuda):
    """A module over a planted stream with a ragged rgb2imu_sync, a non-identity initial rotation and an accelerometer-bias error:
    the module holds accel_bias = B_START, the samples carry B_PLANTED.  The module's increments come from the shipped HIP integrator
    (a quaternion chain), not from the restatement's numpy one, so the summation-order margin does not apply to it: the bound is the
    larger of that margin and 1e-9 of the scale, the float64 tolerance the project holds that integrator's derived rows to
    (tests/test_imu_cov_gpu.py, tests/test_imu_bias_jac_gpu.py); a wrong frame, sign or bias bookkeeping is of order 1e-2."""
    from islam_amd.imu_integrator import IMUModule
    counts = (5, 9, 12, 3, 10, 10, 7, 25, 10, 6, 11, 10, 4, 10, 8, 10)
    s = make_stream(counts, 1.0, B_PLANTED, seed=5, tail=1)
    b_start = np.array([0.1, -0.02, 0.05])
    imu = IMUModule(s['acc'], s['gyro'], s['dt'], accel_bias=torch.tensor(b_start), gyro_bias=torch.zeros(3), gravity=9.79,
                    rgb2imu_sync=s['seg'], device='cuda:0', denoise_accel=False, denoise_gyro=False, dtype=torch.float64,
                    init={'rot': _mat_to_quat(s['R'][0]), 'pos': s['p'][0], 'vel': s['v'][0]})
    st, end = 2, 15
    quat = np.stack([_mat_to_quat(R) for R in s['R']])
    rel = np.stack([_mat_to_quat(s['R'][i].T @ s['R'][i + 1]) for i in range(st, end)])
    init = {'rot': quat[st], 'pos': s['p'][st], 'vel': s['v'][st]}
    before = (imu.estimate_gyro_bias(st, end, rel), imu.integrate(st, end, init), imu.integrate(st, end, init, motion_mode=True))
    attrs = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(imu).items()}
    g, ba, vel, H = imu.estimate_gravity_accel_bias(st, end, quat[st:end + 1], s['p'][st:end + 1])
    for k, v in vars(imu).items():
        assert torch.equal(v, attrs[k]) if torch.is_tensor(v) else (v is attrs[k] or np.array_equal(v, attrs[k])), k
    assert set(vars(imu)) == set(attrs)
    for t in (g, ba, vel, H):
        assert t.dtype == torch.float64 and t.device.type == 'cpu'
    assert tuple(g.shape) == (3,) and tuple(ba.shape) == (3,) and tuple(vel.shape) == (end - st + 1, 3) and tuple(H.shape) == (6, 6)
    # the restatement on numpy increments of the same frames, with the module's accel_bias subtracted
    n = end - st
    seg = s['seg']
    d, dv, dp = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        sl = slice(int(seg[st + i]), int(seg[st + i + 1]))
        d[i] = s['dt'][sl].sum()
        _, dv[i], dp[i] = integrate_reference(s['dt'][sl], s['gyro'][sl], s['acc'][sl] - b_start)
    lo, hi = int(seg[st]), int(seg[end])
    jac = jac_reference(s['dt'][lo:hi], s['gyro'][lo:hi], s['acc'][lo:hi] - b_start, seg[st:end + 1] - lo, True)
    xr, Hr, velr, _ = align_reference(quat[st:end + 1], s['p'][st:end + 1], d, dv, dp, jac)
    truth = dict(g=G_PLANTED, b=B_PLANTED, v=s['v'][st:end + 1])
    xr_total = np.concatenate([xr[0:3], xr[3:6] + b_start])
    e_ref = errors(xr_total, velr, truth)
    e_lib = errors(np.concatenate([g.numpy(), ba.numpy()]), vel.numpy(), truth)
    scale = np.array([np.linalg.norm(G_PLANTED), np.abs(B_PLANTED).max(), np.abs(truth['v']).max()])
    tol = np.maximum(bounds(e_ref, truth), 1e-9 * scale)
    print('module: restatement vs planted %s, module vs planted %s, bound %s, H %.3g' % (e_ref, e_lib, tol, h_error(H.numpy(), Hr)))
    assert np.all(e_lib <= tol) and h_error(H.numpy(), Hr) <= 1e-9
    # covariances, weights and the known magnitude pass through
    w = np.ones(n - 1)
    w[3] = 0.0
    g2, ba2, vel2, H2 = imu.estimate_gravity_accel_bias(st, end, quat[st:end + 1], s['p'][st:end + 1], weight=w, use_cov=True,
                                                         gravity_norm=float(np.linalg.norm(G_PLANTED)))
    e2 = errors(np.concatenate([g2.numpy(), ba2.numpy()]), vel2.numpy(), truth)
    print('module, cov + weight + norm: vs planted %s' % e2)
    assert np.all(e2 <= tol) and abs(np.linalg.norm(g2.numpy()) - np.linalg.norm(G_PLANTED)) <= 1e-14 * 9.79
    # the other entry points give what they gave before
    after = (imu.estimate_gyro_bias(st, end, rel), imu.integrate(st, end, init), imu.integrate(st, end, init, motion_mode=True))
    assert torch.equal(before[0][0], after[0][0]) and torch.equal(before[0][1], after[0][1])
    for a, b in zip(before[1:], after[1:]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].tensor(), b[1].tensor()) and torch.equal(a[3], b[3])
