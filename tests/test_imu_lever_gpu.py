"""GPU tests of the lever-arm / scale solve (islam_imu_lever_scale_solve through islam_amd.ops and IMUModule.estimate_lever_arm).

Reference: lever_reference below, a float64 numpy restatement written pair by pair from the definition in include/islam_hip.h as an
extension of tests/test_imu_align_gpu.py's align_reference: Y_i = [A_i | T_i | -Q_i | rhs_i], the unknowns that are solved compacted in
the order g, b, t, s, a Cholesky under the library's pivot rule, the same four gravity-norm rounds; `reverse` sums the pairs backwards.
Planted truth: the streams of tests/test_imu_align_gpu.py (make_stream; (P_i), (V_i) hold exactly in its discretisation) with a planted
lever arm t and scale s: the camera positions are q_i = (p_i + R_i t) / s, the body rotations are the stream's R_i.  So g, b, t, s and
every v_i are recovered to rounding times conditioning.

Tolerances are measured per case, not fixed: 10 x the larger of (restatement against the planted truth, restatement summed forwards
against backwards), with a floor of 1e-12 of |g|, max |b|, |t|, s, max |v| (where nothing is planted in b: |g|; in t: max |p|, a lever
arm being an offset of the positions).  That bound holds the library against the planted truth and against the restatement.  H against
the restatement: 1e-9 sqrt(H_aa H_bb) per entry, symmetric to the bit.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from tests.test_imu_align_gpu import (B_PLANTED, G_PLANTED, RAGGED12, _mat_to_quat, align_reference, h_error, make_stream)
from tests.test_imu_align_gpu import bounds as align_bounds, errors as align_errors
from tests.test_imu_bias_jac_gpu import integrate_reference, jac_reference
from tests.test_imu_cov_gpu import ACC_COV, GYRO_COV, _quat_to_mat, _rounded
from tests.test_imu_extrinsic_gpu import Q_TRUE, qinv, qmul

pytestmark = pytest.mark.gpu

T_PLANTED = np.array([0.11, -0.06, 0.23])
S_PLANTED = 1.7
PIVOT_REL = 1e-13
# frames x samples (gyro amplitude).  5x7: 4 pairs, the smallest count that determines all 10 unknowns; 1025x4 / 1026x4: P = 1024 and
# 1025 pairs, the last size the solve kernel sums by itself and the first with a partial-sum launch (csrc/imu_terms.h)
SHAPES = {'5x7': ((7,) * 5, 1.0), '12xragged': (RAGGED12, 1.0), '70x10': ((10,) * 70, 1.0), '300x10': ((10,) * 300, 0.5),
          '1025x4': ((4,) * 1025, 0.5), '1026x4': ((4,) * 1026, 0.5)}
# which of (t, s) are unknowns, and what is planted in them (an unknown that is not solved is planted at the value the solve assumes)
SETS = {'lever': (True, False, T_PLANTED, 1.0), 'scale': (False, True, np.zeros(3), S_PLANTED), 'both': (True, True, T_PLANTED, S_PLANTED)}


@functools.lru_cache(maxsize=None)
def base_stream(name, bias=True, amp=None):
    """One of SHAPES (seed = number of frames) in float64: body quaternions and positions, durations, increments in the start-body
    frame, bias Jacobians, and the planted g, b, v.  amp overrides the gyro amplitude (0: no rotation at all)."""
    counts, a = SHAPES[name]
    s = make_stream(counts, a if amp is None else amp, B_PLANTED if bias else np.zeros(3), seed=len(counts))
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


@functools.lru_cache(maxsize=None)
def lever_stream(name, which='both', bias=True, amp=None, t=None):
    """base_stream with the camera positions q = (p + R t) / s of the planted (t, s) of SETS[which] (t overrides the lever arm)."""
    st = dict(base_stream(name, bias, amp))
    lever, scale, tp, sp = SETS[which]
    tp = np.asarray(tp if t is None else t, np.float64)
    R = np.stack([_quat_to_mat(q) for q in st['quat']])
    st.update(q=(st['p'] + R @ tp) / sp, t=tp, s=float(sp), lever=lever, scale=scale)
    st['q'].setflags(write=False)
    return st


def chol_solve(M, rhs):
    """x of M x = rhs by Cholesky under the library's pivot rule (a pivot at or below 1e-13 of its diagonal entry fails: LinAlgError)"""
    n = len(rhs)
    L = np.zeros((n, n))
    for j in range(n):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        if not (p > PIVOT_REL * M[j, j]) or not np.isfinite(p):
            raise np.linalg.LinAlgError('pivot %d: %g of %g' % (j, p, M[j, j]))
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (M[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    x = np.zeros(n)
    for i in range(n):
        x[i] = (rhs[i] - L[i, :i] @ x[:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    if not np.isfinite(x).all():
        raise np.linalg.LinAlgError('not finite')
    return x, L


def lever_reference(quat, q, d, dv, dp, jac=None, cov=None, weight=None, solve_lever=True, solve_scale=False, gravity_norm=None,
                    reverse=False):
    """(x (10) = [g, b, t, s], H (10, 10), vel (n + 1, 3) of the body, excluded) from the definition, pair by pair, float64.
    Raises numpy.linalg.LinAlgError where the library returns ISLAM_ENOTPD."""
    quat, q, d, dv, dp = (np.asarray(a, np.float64) for a in (quat, q, d, dv, dp))
    n = len(d)
    R = [_quat_to_mat(u) for u in quat]
    H, c, bad = np.zeros((10, 10)), np.zeros(10), 0
    I3 = np.eye(3)
    with np.errstate(all='ignore'):
        for i in (range(n - 2, -1, -1) if reverse else range(n - 1)):
            w = 1.0 if weight is None else weight[i]
            if w == 0:
                continue
            Y = np.zeros((3, 11))
            Y[:, 0:3] = -0.5 * (d[i] + d[i + 1]) * I3
            if jac is not None:
                Jv0, Jp0, Jp1 = jac[i][3:6, 3:6], jac[i][6:9, 3:6], jac[i + 1][6:9, 3:6]
                Y[:, 3:6] = R[i] @ Jp0 / d[i] - R[i + 1] @ Jp1 / d[i + 1] - R[i] @ Jv0
            if solve_lever:
                Y[:, 6:9] = (R[i + 1] - R[i]) / d[i] - (R[i + 2] - R[i + 1]) / d[i + 1]
            Q = (q[i + 1] - q[i]) / d[i] - (q[i + 2] - q[i + 1]) / d[i + 1]
            m = R[i + 1] @ dp[i + 1] / d[i + 1] - R[i] @ dp[i] / d[i] + R[i] @ dv[i]
            if solve_scale:
                Y[:, 9], Y[:, 10] = -Q, m
            else:
                Y[:, 10] = m + Q
            ok = np.isfinite(w) and d[i] > 0 and d[i + 1] > 0 and np.isfinite(Y).all()
            if ok and cov is not None:
                S0, S1 = cov[i], cov[i + 1]
                C = R[i + 1] @ S1[6:9, 6:9] @ R[i + 1].T / d[i + 1] ** 2 + \
                    R[i] @ (S0[6:9, 6:9] / d[i] ** 2 - (S0[6:9, 3:6] + S0[3:6, 6:9]) / d[i] + S0[3:6, 3:6]) @ R[i].T
                try:
                    L = chol_solve(0.5 * (C + C.T), np.zeros(3))[1]
                    Y = np.linalg.solve(L, Y)
                except np.linalg.LinAlgError:
                    ok = False
            if not ok:
                bad += 1
                continue
            H += w * Y[:, :10].T @ Y[:, :10]
            c += w * Y[:, :10].T @ Y[:, 10]
    on = [0, 1, 2] + ([3, 4, 5] if jac is not None else []) + ([6, 7, 8] if solve_lever else []) + ([9] if solve_scale else [])
    nu = len(on)
    Hc, cc = H[np.ix_(on, on)], c[on]
    xc = chol_solve(Hc, cc)[0]
    if gravity_norm:
        G = float(gravity_norm)
        gh = xc[0:3] / np.linalg.norm(xc[0:3])
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
            M = B.T @ Hc @ B
            z = chol_solve(0.5 * (M + M.T), B.T @ (cc - Hc @ x0))[0]
            gn = x0[0:3] + b1 * z[0] + b2 * z[1]
            gh = gn / np.linalg.norm(gn)
        xc = np.concatenate([G * gh, z[2:]])
    x = np.zeros(10)
    x[9] = 1.0
    x[on] = xc
    g, b, t, s = x[0:3], x[3:6], x[6:9], x[9]
    vel = np.full((n + 1, 3), np.nan)
    for i in range(n + 1):
        k = i if i < n and d[i] > 0 else (i - 1 if i > 0 and d[i - 1] > 0 else -1)
        if k < 0:
            continue
        ddp = dp[k] + (jac[k][6:9, 3:6] @ b if jac is not None else 0.0)
        vel[i] = (s * (q[k + 1] - q[k]) - (R[k + 1] - R[k]) @ t - 0.5 * g * d[k] ** 2 - R[k] @ ddp) / d[k]
        if k != i:
            vel[i] = vel[i] + g * d[k] + R[k] @ (dv[k] + (jac[k][3:6, 3:6] @ b if jac is not None else 0.0))
    return x, H, vel, bad


def errors(x, vel, st):
    """the largest component of the error of (g, b, t, s, v) against the planted truth"""
    return np.array([np.abs(x[0:3] - st['g']).max(), np.abs(x[3:6] - st['b']).max(), np.abs(x[6:9] - st['t']).max(), abs(x[9] - st['s']),
                     np.abs(vel - st['v']).max()])


def differences(x, vel, xr, velr):
    return np.array([np.abs(x[0:3] - xr[0:3]).max(), np.abs(x[3:6] - xr[3:6]).max(), np.abs(x[6:9] - xr[6:9]).max(), abs(x[9] - xr[9]),
                     np.abs(vel - velr).max()])


def bounds(e_ref, e_order, st):
    """10 x the larger of the restatement's error against the planted truth and of its forwards / backwards difference; floor 1e-12 of
    |g|, max |b| (|g| where nothing is planted in b), |t| (max |p| where nothing is planted in t), s, max |v|"""
    scale = np.array([np.linalg.norm(st['g']), np.abs(st['b']).max() or np.linalg.norm(st['g']),
                      np.linalg.norm(st['t']) or np.abs(st['p']).max(), st['s'], np.abs(st['v']).max()])
    return np.maximum(10.0 * np.maximum(e_ref, e_order), 1e-12 * scale)


def _t(cuda, a, dtype=np.float64):
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), dtype=td, device=cuda)


def _solve(cuda, st, dtype=np.float64, jac=True, cov=None, weight=None, gravity_norm=None, dp=None, d=None):
    """ops.imu_lever_scale_solve on a planted stream -> (x (10), H, vel, excluded) as numpy"""
    from islam_amd import ops
    a = (_t(cuda, st['quat'], dtype), _t(cuda, st['q'], dtype), _t(cuda, st['d'] if d is None else d, dtype), _t(cuda, st['dv'], dtype),
         _t(cuda, st['dp'] if dp is None else dp, dtype))
    g, b, t, s, H, vel, bad = ops.imu_lever_scale_solve(*a, _t(cuda, st['jac']) if jac else None, None if cov is None else _t(cuda, cov),
                                                        None if weight is None else _t(cuda, weight), st['lever'], st['scale'], gravity_norm)
    n = len(st['d'])
    assert g.is_cuda and all(u.dtype == torch.float64 for u in (g, b, t, s, H, vel))
    assert tuple(s.shape) == () and tuple(H.shape) == (10, 10) and tuple(vel.shape) == (n + 1, 3)
    return np.concatenate([u.cpu().numpy().reshape(-1) for u in (g, b, t, s)]), H.cpu().numpy(), vel.cpu().numpy(), bad


def _reference(st, dtype=np.float64, jac=True, cov=None, weight=None, gravity_norm=None, reverse=False):
    r = lambda a: _rounded(a, dtype)
    return lever_reference(r(st['quat']), r(st['q']), r(st['d']), r(st['dv']), r(st['dp']), st['jac'] if jac else None, cov, weight,
                           st['lever'], st['scale'], gravity_norm, reverse)


def _measured(st, **kw):
    """(restatement forwards, its errors against the planted truth, its forwards / backwards difference, the bound)"""
    ref, back = _reference(st, **kw), _reference(st, reverse=True, **kw)
    e_ref, e_order = errors(ref[0], ref[2], st), differences(ref[0], ref[2], back[0], back[2])
    return ref, e_ref, e_order, bounds(e_ref, e_order, st)


def _check(tag, got, st, h_tol=1e-9, **kw):
    """library against the planted truth and against the restatement, under the measured bounds; prints every figure first"""
    x, H, vel, bad = got
    (xr, Hr, velr, badr), e_ref, e_order, tol = _measured(st, **kw)
    e_lib, par = errors(x, vel, st), differences(x, vel, xr, velr)
    he = h_error(H, Hr)
    on = np.flatnonzero(np.diag(Hr))
    print('%s (g, b, t, s, v): restatement vs planted %s, forwards vs backwards %s, bound %s, library vs planted %s, library vs '
          'restatement %s, H %.3g, cond(H) %.3g' % (tag, e_ref, e_order, tol, e_lib, par, he, np.linalg.cond(Hr[np.ix_(on, on)])))
    assert bad == badr
    assert np.all(e_lib <= tol), (e_lib, tol)
    assert np.all(par <= tol), (par, tol)
    assert he <= h_tol and np.array_equal(H, H.T)
    return tol


def _fixed_outputs(st, x, H, jac=True):
    """unknowns that are not solved: exactly 0.0 (b, t) and 1.0 (s), zero rows and columns of H"""
    off = ([] if jac else [3, 4, 5]) + ([] if st['lever'] else [6, 7, 8]) + ([] if st['scale'] else [9])
    for a in off:
        assert x[a] == (1.0 if a == 9 else 0.0) and not np.signbit(x[a]), (a, x[a])
        assert not H[a, :].any() and not H[:, a].any(), a


# ------------------------------------------------------------------------------------------------ 1. parity and recovery
@pytest.mark.parametrize('which', list(SETS))
@pytest.mark.parametrize('name,dtype', [(n, np.float64) for n in ('5x7', '12xragged', '70x10', '1025x4', '1026x4')] +
                         [(n, np.float32) for n in ('12xragged', '70x10')])
def test_against_the_restatement_and_the_planted_truth(cuda, name, dtype, which):
    st = lever_stream(name, which)
    got = _solve(cuda, st, dtype)
    _check('%s %s %s' % (name, which, np.dtype(dtype).name), got, st, dtype=dtype)
    _fixed_outputs(st, got[0], got[1])
    again = _solve(cuda, st, dtype)                       # a second call: the same bits, velocities included
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and again[3] == got[3] == 0


@pytest.mark.parametrize('name,which', [('5x7', 'both'), ('70x10', 'lever'), ('70x10', 'scale'), ('1026x4', 'both')])
def test_without_jacobians(cuda, name, which):
    """No Jacobians, on a stream that carries no accelerometer bias: b exactly 0.0 with zero rows and columns in H; g, t, s and the
    velocities are still the planted ones."""
    st = lever_stream(name, which, bias=False)
    got = _solve(cuda, st, jac=False)
    _fixed_outputs(st, got[0], got[1], jac=False)
    _check('%s %s no jac' % (name, which), got, st, jac=False)


# ------------------------------------------------------------------------------------------------ 2. covariances
def _motion_cov(cuda, st, dtype=np.float64):
    from islam_amd import ops
    seg = np.ascontiguousarray(st['seg'], dtype=np.int64)
    S = int(seg[-1])
    return ops.imu_preint_cov(_t(cuda, st['dt'][:S], dtype), _t(cuda, st['gyro'][:S], dtype), _t(cuda, st['acc'][:S], dtype),
                              torch.tensor(seg, device=cuda), seg, GYRO_COV, ACC_COV, True).cpu().numpy()


@pytest.mark.parametrize('name,dtype', [('12xragged', np.float64), ('70x10', np.float32), ('1026x4', np.float64)])
def test_with_covariances(cuda, name, dtype):
    """cov from ops.imu_preint_cov (motion rows): parity with the restatement's whitened solve; the planted values are still recovered
    (the equations are consistent, whatever the weights).  All S_i scaled by 4: x unchanged to 1e-12 relative, H divided by 4 to
    1e-12 of sqrt(H_aa H_bb) (the bounds of the gravity / bias solve's test; the scaling is by a power of two)."""
    st = lever_stream(name, 'both')
    cov = _motion_cov(cuda, st, dtype)
    got = _solve(cuda, st, dtype, cov=cov)
    _check('%s %s cov' % (name, np.dtype(dtype).name), got, st, dtype=dtype, cov=cov)
    x4, H4, vel4, bad4 = _solve(cuda, st, dtype, cov=4.0 * cov)
    print('cov x 4: x moves by %.3g relative, H / 4 by %.3g' % (np.abs(x4 - got[0]).max() / np.abs(got[0]).max(), h_error(4.0 * H4, got[1])))
    assert bad4 == 0 and np.abs(x4 - got[0]).max() <= 1e-12 * np.abs(got[0]).max()
    assert h_error(4.0 * H4, got[1]) <= 1e-12


# ------------------------------------------------------------------------------------------------ 3. gravity of known magnitude
@pytest.mark.parametrize('name', ['5x7', '70x10', '1026x4'])
def test_gravity_norm(cuda, name):
    st = lever_stream(name, 'both')
    G = float(np.linalg.norm(G_PLANTED))
    got = _solve(cuda, st, gravity_norm=G)
    print('|g| - G = %.3g' % (np.linalg.norm(got[0][0:3]) - G))
    assert abs(np.linalg.norm(got[0][0:3]) - G) <= 1e-12 * G
    _check('%s norm' % name, got, st, gravity_norm=G)


# ------------------------------------------------------------------------------------------------ 4. weights and exclusion
def test_weights_and_exclusion(cuda):
    st = lever_stream('70x10', 'both')
    n = len(st['d'])
    rng = np.random.default_rng(3)
    w = rng.uniform(0.2, 3.0, n - 1)
    _check('70x10 weights', _solve(cuda, st, weight=w), st, weight=w)
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
    _check('70x10 zero weights', clean, st, weight=w0)
    # the same NaN with weight 1 on pair 20 only: excluded and counted as the restatement counts, the rest still solves
    w1 = np.ones(n - 1)
    w1[19] = 0.0
    got = _solve(cuda, st, weight=w1, dp=dpn)
    ref = lever_reference(st['quat'], st['q'], st['d'], st['dv'], dpn, st['jac'], None, w1, True, True)
    assert got[3] == ref[3] == 1 and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
    # a frame without samples (d = 0, no increments): its two pairs are excluded
    d0 = st['d'].copy()
    d0[33] = 0.0
    got = _solve(cuda, st, d=d0)
    wx = np.ones(n - 1)
    wx[[32, 33]] = 0.0
    want = _solve(cuda, st, weight=wx)
    ref = lever_reference(st['quat'], st['q'], d0, st['dv'], st['dp'], st['jac'], None, None, True, True)
    assert got[3] == ref[3] == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 5. ISLAM_ENOTPD
def _raw(cuda, st, rows, weight=None, jac=True, lever=1, scale=1):
    """the C entry point on the first `rows` intervals -> (return code, out_x, out_H, out_vel); the outputs start out as sevens"""
    from islam_amd import _lib
    out = torch.full((110 + 3 * (rows + 1),), 7.0, dtype=torch.float64, device=cuda)
    scratch = torch.empty(_lib.lib().islam_imu_lever_scale_solve_scratch_bytes(rows), dtype=torch.uint8, device=cuda)
    a = [_t(cuda, st[k][:rows + (1 if k in ('quat', 'q') else 0)]) for k in ('quat', 'q', 'd', 'dv', 'dp')]
    a.append(_t(cuda, st['jac'][:rows]) if jac else None)
    wt = None if weight is None else _t(cuda, weight)
    rc = _lib.lib().islam_imu_lever_scale_solve(*[_lib.ptr(t) for t in a], None, _lib.ptr(wt), rows, lever, scale, 0.0, _lib.ptr(out[0:10]),
                                                _lib.ptr(out[10:110]), _lib.ptr(out[110:]), _lib.ptr(scratch), 1, _lib.stream_ptr(cuda))
    o = out.cpu().numpy()
    return rc, o[0:10], o[10:110].reshape(10, 10), o[110:].reshape(rows + 1, 3)


def test_not_positive_definite(cuda):
    """Only cases that fail exactly, not by rounding: no pair at all, all weights zero, and a stream without rotation (R_i constant: the
    lever columns are exact zeros and the first pivot of t is exactly 0).  On failure all ten of x and the velocities are zeros and H
    is written.  The same stream with the lever off and the scale on succeeds and recovers s."""
    from islam_amd import _lib
    st = lever_stream('70x10', 'both')
    n = len(st['d'])
    for rows, wz in ((0, None), (1, None), (n, np.zeros(n - 1))):
        rc, x, H, vel = _raw(cuda, st, rows, wz)
        assert rc == -3 and b'islam_imu_lever_scale_solve' in _lib.lib().islam_last_error()
        assert not x.any() and not vel.any() and not H.any()
    with pytest.raises(_lib.IslamHipError) as ei:
        _solve(cuda, st, weight=np.zeros(n - 1))
    assert ei.value.code == -3 and 'islam_imu_lever_scale_solve' in str(ei.value)
    # no rotation (amp = 0), no accelerometer bias, no Jacobians: t is unobservable, exactly
    flat = lever_stream('70x10', 'both', bias=False, amp=0.0)
    assert all(np.array_equal(u, flat['quat'][0]) for u in flat['quat'])
    with pytest.raises(np.linalg.LinAlgError):
        _reference(flat, jac=False)
    rc, x, H, vel = _raw(cuda, flat, n, jac=False)
    assert rc == -3 and not x.any() and not vel.any()
    assert H[0, 0] > 0 and H[9, 9] > 0 and not H[6:9, :].any() and not H[:, 6:9].any() and np.array_equal(H, H.T)
    with pytest.raises(_lib.IslamHipError) as ei:
        _solve(cuda, flat, jac=False)
    assert ei.value.code == -3
    # the lever off, the scale on: four unknowns, solved, s recovered (the constant R t / s in q does not enter the differences)
    only = dict(flat, lever=False, t=np.zeros(3))
    got = _solve(cuda, only, jac=False)
    _fixed_outputs(only, got[0], got[1], jac=False)
    _check('70x10 no rotation, scale only', got, only, jac=False)


# ------------------------------------------------------------------------------------------------ 6. consistency with the gravity / bias solve
def test_consistent_with_the_gravity_bias_solve(cuda):
    """Planted t = 0, s = 1, the lever solved: the camera positions are the body positions, g, b and v agree with
    ops.imu_gravity_bias_solve on the same rows within the sum of the two measured bounds, and |t| is under its bound."""
    from islam_amd import ops
    st = lever_stream('70x10', 'lever', t=(0.0, 0.0, 0.0))
    assert np.array_equal(st['q'], st['p'])
    got = _solve(cuda, st)
    tol = _check('70x10 t = 0', got, st)
    g, b, H6, vel, bad = ops.imu_gravity_bias_solve(*[_t(cuda, st[k]) for k in ('quat', 'p', 'd', 'dv', 'dp', 'jac')])
    x6, vel6 = np.concatenate([g.cpu().numpy(), b.cpu().numpy()]), vel.cpu().numpy()
    xr, _, velr, _ = align_reference(st['quat'], st['p'], st['d'], st['dv'], st['dp'], st['jac'])
    tol6 = align_bounds(align_errors(xr, velr, st), st)
    diff = np.array([np.abs(got[0][0:3] - x6[0:3]).max(), np.abs(got[0][3:6] - x6[3:6]).max(), np.abs(got[2] - vel6).max()])
    both = tol[[0, 1, 4]] + tol6
    print('against the gravity / bias solve (g, b, v): %s, bound %s; |t| = %.3g, bound %.3g' % (diff, both, np.linalg.norm(got[0][6:9]), tol[2]))
    assert bad == 0 and np.all(diff <= both)
    assert np.abs(got[0][6:9]).max() <= tol[2]


# ------------------------------------------------------------------------------------------------ 7. IMUModule
@pytest.mark.parametrize('solve_scale', [False, True])
def test_imu_module(cuda, solve_scale):
    """A module over a planted stream with a ragged rgb2imu_sync, a non-identity initial rotation, an accelerometer-bias error and a
    mount R_x = Exp((1.1, -0.7, 0.4)): the camera rotations are R_i R_x, the camera positions (p_i + R_i t) / s.  The module's increments
    come from the shipped HIP integrator (a quaternion chain), not from the restatement's numpy one, so the bound is the larger of the
    measured one and 1e-9 of the scale, the float64 tolerance the project holds that integrator's derived rows to; a wrong frame, sign,
    conjugation or bias bookkeeping is of order 1e-2."""
    from islam_amd.imu_integrator import IMUModule
    counts = (5, 9, 12, 3, 10, 10, 7, 25, 10, 6, 11, 10, 4, 10, 8, 10)
    s = make_stream(counts, 1.0, B_PLANTED, seed=5, tail=1)
    b_start = np.array([0.1, -0.02, 0.05])
    imu = IMUModule(s['acc'], s['gyro'], s['dt'], accel_bias=torch.tensor(b_start), gyro_bias=torch.zeros(3), gravity=9.79,
                    rgb2imu_sync=s['seg'], device='cuda:0', denoise_accel=False, denoise_gyro=False, dtype=torch.float64,
                    init={'rot': _mat_to_quat(s['R'][0]), 'pos': s['p'][0], 'vel': s['v'][0]})
    st, end = 2, 15
    n = end - st
    sp = S_PLANTED if solve_scale else 1.0
    quat = np.stack([_mat_to_quat(R) for R in s['R']])[st:end + 1]
    Rb = np.stack([_quat_to_mat(u) for u in quat])
    cam_rots = qmul(quat, Q_TRUE)
    cam_pos = (s['p'][st:end + 1] + Rb @ T_PLANTED) / sp
    attrs = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(imu).items()}
    g, ba, t, sc, vel, H = imu.estimate_lever_arm(st, end, cam_rots, cam_pos, Q_TRUE, solve_scale=solve_scale)
    for k, v in vars(imu).items():
        assert torch.equal(v, attrs[k]) if torch.is_tensor(v) else (v is attrs[k] or np.array_equal(v, attrs[k])), k
    assert set(vars(imu)) == set(attrs)
    for u in (g, ba, t, sc, vel, H):
        assert u.dtype == torch.float64 and u.device.type == 'cpu'
    assert tuple(g.shape) == tuple(ba.shape) == tuple(t.shape) == (3,) and tuple(sc.shape) == ()
    assert tuple(vel.shape) == (n + 1, 3) and tuple(H.shape) == (10, 10)
    if not solve_scale:
        assert float(sc) == 1.0 and not H[9].any()
    # the restatement on numpy increments of the same frames, with the module's accel_bias subtracted, and on the body rotations
    # conjugated in numpy
    seg = s['seg']
    d, dv, dp = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        sl = slice(int(seg[st + i]), int(seg[st + i + 1]))
        d[i] = s['dt'][sl].sum()
        _, dv[i], dp[i] = integrate_reference(s['dt'][sl], s['gyro'][sl], s['acc'][sl] - b_start)
    lo, hi = int(seg[st]), int(seg[end])
    jac = jac_reference(s['dt'][lo:hi], s['gyro'][lo:hi], s['acc'][lo:hi] - b_start, seg[st:end + 1] - lo, True)
    body = qmul(cam_rots, qinv(Q_TRUE))
    truth = dict(g=G_PLANTED, b=B_PLANTED, t=T_PLANTED, s=sp, v=s['v'][st:end + 1], p=s['p'][st:end + 1])
    ref = lever_reference(body, cam_pos, d, dv, dp, jac, None, None, True, solve_scale)
    back = lever_reference(body, cam_pos, d, dv, dp, jac, None, None, True, solve_scale, reverse=True)
    total = lambda x: np.concatenate([x[0:3], x[3:6] + b_start, x[6:10]])
    e_ref, e_order = errors(total(ref[0]), ref[2], truth), differences(ref[0], ref[2], back[0], back[2])
    x = np.concatenate([g.numpy(), ba.numpy(), t.numpy(), [float(sc)]])
    e_lib = errors(x, vel.numpy(), truth)
    scale = np.array([np.linalg.norm(G_PLANTED), np.abs(B_PLANTED).max(), np.linalg.norm(T_PLANTED), sp, np.abs(truth['v']).max()])
    tol = np.maximum(bounds(e_ref, e_order, truth), 1e-9 * scale)
    print('module, solve_scale=%s (g, b, t, s, v): restatement vs planted %s, forwards vs backwards %s, module vs planted %s, bound %s, '
          'H %.3g' % (solve_scale, e_ref, e_order, e_lib, tol, h_error(H.numpy(), ref[1])))
    assert np.all(e_lib <= tol) and h_error(H.numpy(), ref[1]) <= 1e-9
    # covariances, weights and the known magnitude pass through
    w = np.ones(n - 1)
    w[3] = 0.0
    out = imu.estimate_lever_arm(st, end, cam_rots, cam_pos, Q_TRUE, weight=w, use_cov=True, gravity_norm=float(np.linalg.norm(G_PLANTED)),
                                 solve_scale=solve_scale)
    e2 = errors(np.concatenate([out[0].numpy(), out[1].numpy(), out[2].numpy(), [float(out[3])]]), out[4].numpy(), truth)
    print('module, cov + weight + norm: vs planted %s' % e2)
    assert np.all(e2 <= tol) and abs(np.linalg.norm(out[0].numpy()) - np.linalg.norm(G_PLANTED)) <= 1e-12 * 9.79
