"""GPU tests of the time-offset / gyro-bias solve (islam_imu_time_offset_solve and islam_imu_time_shift through islam_amd.ops, and
IMUModule.estimate_time_offset).

Reference: time_offset_reference below, a float64 numpy restatement written row by row from the definition in include/islam_hip.h:
e_i = Log(DR_i^T DRref_i) as islam_imu_gyro_bias_solve takes it, u_i = we_i - DR_i^T ws_i, Y_i = [J_phig,i | u_i], the unknowns that are
solved compacted, a Cholesky under the library's pivot rule (tests/test_imu_lever_gpu.py: chol_solve, whose LinAlgError names the
pivot), the same Huber rounds; `reverse` sums the rows backwards.  loop_reference restates the round loop of the module.

Two planted truths, on streams of uniform dt = 5 ms whose three gyro axes are sines of different frequency (so that u_i varies):
  linear-exact  DRref_i := DR_i Exp(J_phig,i b + u_i td): the equations hold exactly and (b, td) come back to rounding times
                conditioning;
  physical      a zero-order-hold body rotation W(t) from the true rates, DRref_i = W(t_i + td)^T W(t_{i+1} + td), the measured rates
                are true + b, with spare samples on both sides of the window: one solve is right to second order in (b, td), the
                module's rounds converge to rounding.

Tolerances are measured per case, never fixed in advance: 10 x the larger of (restatement against planted, restatement summed forwards
against backwards), with a floor of 1e-12 of max |b| and of |td|; a pair (rad/s, s).  The residuals are held to that pair carried through
their definition, max |J_i| tol_b + max |u_i| tol_td, plus 16 roundings of the largest |e_i|.  H against the restatement: 1e-9
sqrt(H_aa H_bb) per entry, symmetric to the bit.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from tests.test_imu_align_gpu import RAGGED12, h_error
from tests.test_imu_bias_jac_gpu import jac_reference
from tests.test_imu_cov_gpu import _quat_to_mat, _rounded
from tests.test_imu_extrinsic_gpu import qexp, qinv, qmul
from tests.test_imu_lever_gpu import chol_solve

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
DT = 0.005
PAD = 8                                               # spare samples on either side of the window
B_PLANTED = np.array([0.02, -0.01, 0.015])            # rad/s
TD_PLANTED = 0.003                                    # s
# frames x samples.  5x7: the smallest that determines four unknowns with room; 1024x4 / 1025x4: the last size the solve kernel sums by
# itself and the first with a partial-sum launch (csrc/imu_terms.h)
SHAPES = {'5x7': (7,) * 5, '12xragged': RAGGED12, '12x10': (10,) * 12, '70x10': (10,) * 70, '1024x4': (4,) * 1024, '1025x4': (4,) * 1025}


def true_rates(S):
    """(S, 3) rad/s at the sample times k DT: three sines of different frequency"""
    t = np.arange(S) * DT
    return np.stack([0.9 * np.sin(2 * np.pi * 0.9 * t + 0.2), 0.7 * np.sin(2 * np.pi * 1.4 * t + 1.1), 1.1 * np.sin(2 * np.pi * 2.3 * t + 0.5)], 1)


def frame_rotations(dt, gyro, seg):
    """DR_i (n, 4) xyzw: the zero-order-hold chain of Exp(w_k dt_k) over the samples [seg[i], seg[i+1]) of every frame"""
    out = np.zeros((len(seg) - 1, 4))
    for i in range(len(seg) - 1):
        q = np.array([0.0, 0.0, 0.0, 1.0])
        for j in range(int(seg[i]), int(seg[i + 1])):
            q = qmul(q, qexp(gyro[j] * dt[j]))
        out[i] = q
    return out


def _acc(S):
    return np.tile(np.array([0.0, 0.0, 9.8]), (S, 1))


def rows_of(dt, gyro, seg):
    """(rot (n, 4), jac (n, 9, 6), rate_start, rate_end (n, 3)) of the frames of seg; needs the sample gyro[seg[-1]]"""
    seg = np.asarray(seg, np.int64)
    return (frame_rotations(dt, gyro, seg), jac_reference(dt, gyro, _acc(len(dt)), seg, True), gyro[seg[:-1]].copy(), gyro[seg[1:]].copy())


def _u(rot, ws, we):
    return np.stack([we[i] - _quat_to_mat(rot[i]).T @ ws[i] for i in range(len(rot))])


@functools.lru_cache(maxsize=None)
def linear_stream(name, bias=True):
    """The linear-exact truth on one of SHAPES: dict(rot, ref, jac, ws, we, b, td).  bias=False plants b = 0 (for solve_bias = 0)."""
    counts = SHAPES[name]
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S = int(seg[-1]) + 1
    dt, gyro = np.full(S, DT), true_rates(S)
    rot, jac, ws, we = rows_of(dt, gyro, seg)
    b = B_PLANTED if bias else np.zeros(3)
    ref = qmul(rot, qexp(jac[:, 0:3, 0:3] @ b + _u(rot, ws, we) * TD_PLANTED))
    out = dict(rot=rot, ref=ref, jac=jac, ws=ws, we=we, b=b, td=TD_PLANTED)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def body_rotation(gyro, tau):
    """W(tau), xyzw: the zero-order-hold rotation of the body from time 0 of the stream to tau (uniform DT)"""
    k = int(np.floor(tau / DT + 1e-9))
    q = np.array([0.0, 0.0, 0.0, 1.0])
    for j in range(k):
        q = qmul(q, qexp(gyro[j] * DT))
    return qmul(q, qexp(gyro[k] * (tau - k * DT)))


@functools.lru_cache(maxsize=None)
def physical_stream(name, scale=1.0, td=None):
    """The physical truth on one of SHAPES with PAD spare samples on both sides: dict(dt, gyro (measured = true + b), seg (into the padded
    stream), ref, b, td) with (b, td) = scale x the planted pair (td overrides the offset, in seconds)."""
    counts = SHAPES[name]
    seg = PAD + np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S = int(seg[-1]) + PAD
    b = scale * B_PLANTED
    td = scale * TD_PLANTED if td is None else float(td)
    true = true_rates(S)
    W = [body_rotation(true, s * DT + td) for s in seg]
    ref = np.stack([qmul(qinv(W[i]), W[i + 1]) for i in range(len(counts))])
    out = dict(dt=np.full(S, DT), gyro=true + b, seg=seg, ref=ref, b=b, td=td)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def physical_rows(ph):
    rot, jac, ws, we = rows_of(ph['dt'], ph['gyro'], ph['seg'])
    return dict(rot=rot, ref=ph['ref'], jac=jac, ws=ws, we=we, b=ph['b'], td=ph['td'])


def _log(a, b):
    """Log(a^-1 (x) b) as the library takes it: the quaternion with w >= 0, 2 atan2(|vec|, w) / |vec| (2 / w below 1e-8 w)"""
    q = qmul(qinv(a), b)
    if q[3] < 0:
        q = -q
    vn = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    k = 2.0 * np.arctan2(vn, q[3]) / vn if vn > 1e-8 * q[3] else 2.0 / q[3]
    return k * q[:3]


def time_offset_reference(jac, rot_imu, rot_ref, rate_start, rate_end, weight=None, solve_bias=True, delta=None, rounds=4, reverse=False):
    """(x (4) = [dbg, td], H (4, 4), res (n), excluded) from the definition, row by row, float64.  Raises numpy.linalg.LinAlgError
    (naming the pivot) where the library returns ISLAM_ENOTPD."""
    rot_imu, rot_ref, ws, we = (np.asarray(a, np.float64) for a in (rot_imu, rot_ref, rate_start, rate_end))
    n = len(rot_imu)
    Y = np.zeros((n, 3, 5))
    with np.errstate(all='ignore'):
        for i in range(n):
            if solve_bias:
                Y[i, :, 0:3] = jac[i][0:3, 0:3]
            Y[i, :, 3] = we[i] - _quat_to_mat(rot_imu[i]).T @ ws[i]
            Y[i, :, 4] = _log(rot_imu[i], rot_ref[i])
    fin = np.isfinite(Y).all((1, 2))
    on = [0, 1, 2, 3] if solve_bias else [3]
    K = int(rounds) if delta else 0
    x = np.zeros(4)
    for r in range(K + 1):
        H, c, bad = np.zeros((4, 4)), np.zeros(4), 0
        for i in (range(n - 1, -1, -1) if reverse else range(n)):
            w = 1.0 if weight is None else weight[i]
            if w == 0:
                continue
            if not fin[i] or not np.isfinite(w) or w < 0:
                bad += 1
                continue
            rho = 1.0
            if r > 0:
                rn = np.linalg.norm(Y[i, :, 4] - Y[i, :, :4] @ x)
                rho = min(1.0, delta / rn) if rn > 0 else 1.0
            H += w * rho * Y[i, :, :4].T @ Y[i, :, :4]
            c += w * rho * Y[i, :, :4].T @ Y[i, :, 4]
        x = np.zeros(4)
        x[on] = chol_solve(H[np.ix_(on, on)], c[on])[0]
    with np.errstate(all='ignore'):
        res = np.array([np.linalg.norm(Y[i, :, 4] - Y[i, :, :4] @ x) if fin[i] else np.nan for i in range(n)])
    return x, H, res, bad


def shift_reference(rot, ws, we, tau):
    q = qmul(qmul(qexp(-np.asarray(ws, np.float64) * tau), np.asarray(rot, np.float64)), qexp(np.asarray(we, np.float64) * tau))
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def loop_reference(dt, gyro, sync, ref, gn_rounds=3, weight=None, solve_bias=True, shift=True):
    """The round loop of IMUModule.estimate_time_offset on a stream with zero module bias: (T, bias (3), H, res, k).  shift=False leaves
    the sub-sample part tau out of the rotations (what the loop would do without islam_imu_time_shift)."""
    sync = np.asarray(sync, np.int64)
    n, S = len(sync) - 1, len(dt)
    w0 = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    d0 = float(dt[sync[0]])
    T, k, tau, bias = 0.0, 0, 0.0, np.zeros(3)
    for _ in range(1 + gn_rounds):
        moved = sync + k
        inside = (moved[:-1] >= 0) & (moved[1:] <= S - 1)
        segc = np.clip(moved, 0, S - 1)
        rot, jac, ws, we = rows_of(dt, gyro - bias, segc)
        if shift:
            rot = shift_reference(rot, ws, we, tau)
        x, H, res, _ = time_offset_reference(jac, rot, ref, ws, we, np.where(inside, w0, 0.0), solve_bias)
        bias = bias + x[0:3]
        T = T + x[3]
        k = int(np.floor(T / d0))
        tau = T - k * d0
    return T, bias, H, res, k


def errors(x, st):
    """(error of b, error of td) against the planted truth"""
    return np.array([np.abs(x[0:3] - st['b']).max(), abs(x[3] - st['td'])])


def differences(x, y):
    return np.array([np.abs(x[0:3] - y[0:3]).max(), abs(x[3] - y[3])])


def bounds(e_ref, e_order, st):
    """10 x the larger of the restatement's error against the planted truth and of its forwards / backwards difference; floor 1e-12 of
    max |b| and of |td|"""
    return np.maximum(10.0 * np.maximum(e_ref, e_order), 1e-12 * np.array([np.abs(st['b']).max(), abs(st['td'])]))


def res_bound(st, tol):
    """the bound (tol_b, tol_td) carried through r = e - J dbg - u td, plus 16 roundings of the largest |e|"""
    u = _u(st['rot'], st['ws'], st['we'])
    e = np.array([np.linalg.norm(_log(st['rot'][i], st['ref'][i])) for i in range(len(u))])
    return float(np.abs(st['jac'][:, 0:3, 0:3]).sum(2).max() * tol[0] + np.linalg.norm(u, axis=1).max() * tol[1] + 16 * EPS * e.max())


def rounded(st, dtype):
    """the stream with its I/O arrays rounded to dtype (both sides get the rounded inputs)"""
    return dict(st, **{k: _rounded(st[k], dtype) for k in ('rot', 'ref', 'ws', 'we')})


def reference(st, reverse=False, **kw):
    return time_offset_reference(st['jac'], st['rot'], st['ref'], st['ws'], st['we'], reverse=reverse, **kw)


def measured(st, **kw):
    """(restatement forwards, its errors against the planted truth, its forwards / backwards difference, the bound)"""
    ref, back = reference(st, **kw), reference(st, reverse=True, **kw)
    e_ref, e_order = errors(ref[0], st), differences(ref[0], back[0])
    return ref, e_ref, e_order, bounds(e_ref, e_order, st)


def _t(cuda, a, dtype=np.float64):
    td = {np.float64: torch.float64, np.float32: torch.float32}[dtype]
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype), dtype=td, device=cuda)


def _solve(cuda, st, dtype=np.float64, weight=None, solve_bias=True, delta=None, rounds=4, jac=True):
    """ops.imu_time_offset_solve on a stream -> (x (4), H, res, excluded) as numpy"""
    from islam_amd import ops
    dbg, td, H, res, bad = ops.imu_time_offset_solve(_t(cuda, st['jac']) if jac else None, _t(cuda, st['rot'], dtype), _t(cuda, st['ref'], dtype),
                                                     _t(cuda, st['ws'], dtype), _t(cuda, st['we'], dtype),
                                                     None if weight is None else _t(cuda, weight), solve_bias, delta, rounds)
    n = len(st['rot'])
    assert dbg.is_cuda and all(u.dtype == torch.float64 for u in (dbg, td, H, res))
    assert tuple(dbg.shape) == (3,) and tuple(td.shape) == () and tuple(H.shape) == (4, 4) and tuple(res.shape) == (n,)
    return np.concatenate([dbg.cpu().numpy(), td.cpu().numpy().reshape(1)]), H.cpu().numpy(), res.cpu().numpy(), bad


def _check(tag, got, st, tol=None, **kw):
    """library against the planted truth and against the restatement, under the measured bounds; prints every figure first"""
    x, H, res, bad = got
    (xr, Hr, resr, badr), e_ref, e_order, own = measured(st, **kw)
    tol = own if tol is None else tol
    e_lib, par = errors(x, st), differences(x, xr)
    he, rb = h_error(H, Hr), res_bound(st, tol)
    e_res = float(np.nanmax(np.abs(res - resr)))
    on = np.flatnonzero(np.diag(Hr))
    print('%s (b, td): restatement vs planted %s, forwards vs backwards %s, bound %s, library vs planted %s, library vs restatement %s, '
          'H %.3g, residuals %.3g (bound %.3g), cond(H) %.3g' % (tag, e_ref, e_order, tol, e_lib, par, he, e_res, rb,
                                                                 np.linalg.cond(Hr[np.ix_(on, on)])))
    assert bad == badr
    assert np.all(e_lib <= tol), (e_lib, tol)
    assert np.all(par <= tol), (par, tol)
    assert he <= 1e-9 and np.array_equal(H, H.T)
    assert np.array_equal(np.isnan(res), np.isnan(resr)) and e_res <= rb
    return tol


# ------------------------------------------------------------------------------------------------ 1. the linear-exact truth
@pytest.mark.parametrize('solve_bias', [True, False])
@pytest.mark.parametrize('name,dtype', [(n, np.float64) for n in ('5x7', '12xragged', '70x10', '1024x4', '1025x4')] + [('70x10', np.float32)])
def test_linear_exact(cuda, name, dtype, solve_bias):
    st = rounded(linear_stream(name, solve_bias), dtype)
    got = _solve(cuda, st, dtype, solve_bias=solve_bias)
    _check('%s %s solve_bias=%d' % (name, np.dtype(dtype).name, solve_bias), got, st, solve_bias=solve_bias)
    if not solve_bias:                                    # dbg exactly 0.0, zero rows and columns of H, and the Jacobians are not needed
        assert not got[0][0:3].any() and not np.signbit(got[0][0:3]).any() and not got[1][0:3].any() and not got[1][:, 0:3].any()
        none = _solve(cuda, st, dtype, solve_bias=False, jac=False)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], none[:3]))
    again = _solve(cuda, st, dtype, solve_bias=solve_bias)  # a second call: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and again[3] == got[3] == 0


# ------------------------------------------------------------------------------------------------ 2. the physical truth
@pytest.mark.parametrize('name', ['12x10', '70x10'])
def test_physical_second_order(cuda, name):
    """One solve is right to second order: halving (b, td) divides the error of td and of b by more than 3 (second order gives 4, a
    wrong first-order term gives 2), and the library stays within the stream's linear-exact bound of the restatement."""
    tol = measured(linear_stream(name))[3]
    err = []
    for scale in (1.0, 0.5):
        st = physical_rows(physical_stream(name, scale))
        x = _solve(cuda, st)[0]
        xr = reference(st)[0]
        err.append(errors(x, st))
        print('%s physical, (b, td) x %g: library vs planted %s, restatement vs planted %s, library vs restatement %s (bound %s)'
              % (name, scale, err[-1], errors(xr, st), differences(x, xr), tol))
        assert np.all(differences(x, xr) <= tol)
    print('%s physical: the error falls by %s' % (name, err[0] / err[1]))
    assert np.all(err[0] > 3.0 * err[1])


# ------------------------------------------------------------------------------------------------ 3. same bits, weights, exclusion
def test_same_bits_weights_and_exclusion(cuda):
    st = linear_stream('70x10')
    n = len(st['rot'])
    w = np.ones(n)
    w[4] = 0.0
    dirty = dict(st, rot=st['rot'].copy(), ref=st['ref'].copy(), ws=st['ws'].copy())
    dirty['rot'][4, 1] = dirty['ws'][4, 0] = np.nan
    clean, nan4 = _solve(cuda, st, weight=w), _solve(cuda, dirty, weight=w)
    assert clean[3] == 0 and nan4[3] == 0 and np.array_equal(clean[0], nan4[0]) and np.array_equal(clean[1], nan4[1])
    keep = np.arange(n) != 4
    assert np.array_equal(clean[2][keep], nan4[2][keep]) and np.isnan(nan4[2][4]) and np.isfinite(clean[2]).all()
    _check('70x10 weight 0 on row 4', clean, st, weight=w)
    # NaN in rot_ref of row 5: counted under weight 1, not under weight 0; x is the bits of the call without rows 4 and 5
    dirty['ref'][5, 2] = np.nan
    w5 = w.copy()
    w5[5] = 0.0
    one, zero = _solve(cuda, dirty, weight=w), _solve(cuda, dirty, weight=w5)
    assert one[3] == 1 and zero[3] == 0 and np.array_equal(one[0], zero[0]) and np.array_equal(one[1], zero[1]) and np.isnan(one[2][5])
    assert reference(dirty, weight=w)[3] == 1 and reference(dirty, weight=w5)[3] == 0
    # a negative and a non-finite weight: each counted, neither takes part
    wn = w5.copy()
    wn[4], wn[5] = -1.0, np.inf
    neg = _solve(cuda, st, weight=wn)
    assert neg[3] == 2 and np.array_equal(neg[0], zero[0]) and np.array_equal(neg[1], zero[1])


# ------------------------------------------------------------------------------------------------ 4. no change of rate
def constant_rate_rows(n=8, c=0.4):
    """Rows of a constant rate (0, 0, c): rot_imu = (0, 0, sin, cos) exactly about z, so u_i is exactly 0"""
    a = 0.5 * c * 10 * DT
    rot = np.tile(np.array([0.0, 0.0, np.sin(a), np.cos(a)]), (n, 1))
    rate = np.tile(np.array([0.0, 0.0, c]), (n, 1))
    st = linear_stream('70x10')
    return dict(rot=rot, ref=np.array(st['ref'][:n]), jac=np.array(st['jac'][:n]), ws=rate, we=rate.copy(), b=np.zeros(3), td=0.0)


@pytest.mark.parametrize('solve_bias', [1, 0])
def test_not_positive_definite(cuda, solve_bias):
    from islam_amd import _lib, ops
    st = constant_rate_rows()
    n = len(st['rot'])
    with pytest.raises(_lib.IslamHipError) as ei:
        _solve(cuda, st, solve_bias=bool(solve_bias))
    assert ei.value.code == -3 and 'islam_imu_time_offset_solve' in str(ei.value)
    with pytest.raises(_lib.IslamHipError) as ei:         # no row at all
        ops.imu_time_offset_solve(_t(cuda, np.zeros((0, 9, 6))), *[_t(cuda, np.zeros((0, k))) for k in (4, 4, 3, 3)], None, bool(solve_bias))
    assert ei.value.code == -3
    # at the C level: out_x and out_res zeros, out_H written (its td row and column exact zeros: that is the pivot that fails)
    out = torch.full((20 + n,), 7.0, dtype=torch.float64, device=cuda)
    scratch = torch.empty(_lib.lib().islam_imu_time_offset_solve_scratch_bytes(n), dtype=torch.uint8, device=cuda)
    a = [_t(cuda, st[k]) for k in ('jac', 'rot', 'ref', 'ws', 'we')]
    rc = _lib.lib().islam_imu_time_offset_solve(*[_lib.ptr(t) for t in a], None, n, solve_bias, 1e-3, 2, _lib.ptr(out[0:4]), _lib.ptr(out[4:20]),
                                                _lib.ptr(out[20:]), _lib.ptr(scratch), 1, _lib.stream_ptr(cuda))
    host = out.cpu().numpy()
    H = host[4:20].reshape(4, 4)
    assert rc == -3 and not host[0:4].any() and not host[20:].any()
    assert not (H == 7.0).any() and not H[3].any() and not H[:, 3].any() and (np.diag(H)[0:3] > 0).all() == bool(solve_bias)


# ------------------------------------------------------------------------------------------------ 5. Huber rounds
OUTLIERS = (7, 31, 55)


@functools.lru_cache(maxsize=None)
def huber_stream():
    """70x10 linear-exact with 3 of the 70 references turned by 0.3 rad"""
    st = dict(linear_stream('70x10'))
    ref = st['ref'].copy()
    for k, i in enumerate(OUTLIERS):
        axis = np.eye(3)[k]
        ref[i] = qmul(ref[i], qexp(0.3 * axis))
    ref.setflags(write=False)
    st['ref'] = ref
    return st


def test_huber_rounds(cuda):
    st = huber_stream()
    kw = dict(delta=1e-3, rounds=4)
    # library against restatement: what the order of summation moves in this case, no less than the bound of the clean case
    ref, back = reference(st, **kw), reference(st, reverse=True, **kw)
    tol = np.maximum(10.0 * differences(ref[0], back[0]), measured(linear_stream('70x10'))[3])
    plain, robust = _solve(cuda, st), _solve(cuda, st, **kw)
    par = differences(robust[0], ref[0])
    e_res = float(np.abs(robust[2] - ref[2]).max())
    gain_ref = errors(reference(st)[0], st)[1] / errors(ref[0], st)[1]
    gain_lib = errors(plain[0], st)[1] / errors(robust[0], st)[1]
    print('huber: library vs restatement %s (bound %s), residuals %.3g (bound %.3g), H %.3g; error of td plain / robust: library %.3g, '
          'restatement %.3g' % (par, tol, e_res, res_bound(st, tol), h_error(robust[1], ref[1]), gain_lib, gain_ref))
    assert robust[3] == 0 and np.all(par <= tol) and e_res <= res_bound(st, tol)
    assert h_error(robust[1], ref[1]) <= 1e-9 and np.array_equal(robust[1], robust[1].T)
    assert gain_lib >= 0.5 * gain_ref
    # delta = 0 with rounds = 4: the bits of the plain solve
    zero = _solve(cuda, st, delta=0.0, rounds=4)
    assert all(np.array_equal(a, b) for a, b in zip(zero[:3], plain[:3]))


# ------------------------------------------------------------------------------------------------ 6. islam_imu_time_shift
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_time_shift(cuda, dtype):
    """Against numpy: the output is the float64 value rounded once to the I/O type, 2^-53 or 2^-24 of a component <= 1, behind two
    Exp, two products and a normalisation in float64 (8 roundings)."""
    from islam_amd import _lib, ops
    st = rounded(linear_stream('70x10'), dtype)
    n, tau = len(st['rot']), 0.0021
    a = [_t(cuda, st[k], dtype) for k in ('rot', 'ws', 'we')]
    out = ops.imu_time_shift(*a, tau)
    assert out.dtype == a[0].dtype and tuple(out.shape) == (n, 4) and out.data_ptr() != a[0].data_ptr()
    want = shift_reference(st['rot'], st['ws'], st['we'], tau)
    tol = 8 * EPS + (2.0 ** -24 if dtype == np.float32 else 0.0)
    e = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    # out aliasing in, at the C level
    alias = a[0].clone()
    rc = _lib.lib().islam_imu_time_shift(_lib.ptr(alias), _lib.ptr(a[1]), _lib.ptr(a[2]), n, tau, _lib.ptr(alias), 1 if dtype == np.float64 else 0,
                                         _lib.stream_ptr(cuda))
    # tau = 0: the renormalised input
    same = ops.imu_time_shift(*a, 0.0).cpu().numpy().astype(np.float64)
    e0 = float(np.abs(same - st['rot'] / np.linalg.norm(st['rot'], axis=1, keepdims=True)).max())
    # there and back with the same rates: the identity
    back = ops.imu_time_shift(out, a[1], a[2], -tau).cpu().numpy().astype(np.float64)
    eb = float(np.abs(back - st['rot']).max())
    print('time shift %s: vs numpy %.3g (bound %.3g), tau = 0 %.3g, there and back %.3g' % (np.dtype(dtype).name, e, tol, e0, eb))
    assert rc == 0 and torch.equal(alias, out)
    assert e <= tol and e0 <= tol
    assert eb <= (1e-15 if dtype == np.float64 else 2.0 ** -22)


# ------------------------------------------------------------------------------------------------ 7. IMUModule
def _module(ph, dt=None):
    from islam_amd.imu_integrator import IMUModule
    S = len(ph['dt'])
    return IMUModule(_acc(S), np.array(ph['gyro']), np.array(ph['dt'] if dt is None else dt), accel_bias=torch.zeros(3), gyro_bias=torch.zeros(3), gravity=9.8,
                     rgb2imu_sync=ph['seg'], device='cuda:0', denoise_accel=False, denoise_gyro=False, dtype=torch.float64)


@pytest.mark.parametrize('samples', [2.4, -1.7, 0.5])
def test_imu_module(cuda, samples):
    """The rounds reach the planted offset of whole samples and a fraction, and the planted bias, to rounding: the restatement of the
    same loop reaches 1e-13 after three rounds and rounding after four; without the sub-sample shift it stalls near 1e-7 s."""
    ph = physical_stream('12x10', 1.0, samples * DT)
    ph = dict(ph, ref=np.array(ph['ref']))                # (a writable copy for torch)
    imu, n = _module(ph), len(ph['ref'])
    attrs = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(imu).items()}
    T, bias, H, res, k = imu.estimate_time_offset(0, n, ph['ref'], gn_rounds=4)
    for key, v in vars(imu).items():
        assert torch.equal(v, attrs[key]) if torch.is_tensor(v) else (v is attrs[key] or np.array_equal(v, attrs[key])), key
    assert set(vars(imu)) == set(attrs)
    for t, shape in ((T, ()), (bias, (3,)), (H, (4, 4)), (res, (n,))):
        assert t.dtype == torch.float64 and t.device.type == 'cpu' and tuple(t.shape) == shape
    Tr, br, Hr, resr, kr = loop_reference(ph['dt'], ph['gyro'], ph['seg'], ph['ref'], 4)
    e_ref = np.array([np.abs(br - ph['b']).max(), abs(Tr - ph['td'])])
    tol = np.maximum(10.0 * e_ref, 1e-12)
    e_lib = np.array([np.abs(bias.numpy() - ph['b']).max(), abs(float(T) - ph['td'])])
    par = np.array([np.abs(bias.numpy() - br).max(), abs(float(T) - Tr)])
    print('module, td = %+.1f samples (b, T): restatement vs planted %s, bound %s, module vs planted %s, module vs restatement %s, k = %d, '
          'largest residual %.3g' % (samples, e_ref, tol, e_lib, par, k, float(res.max())))
    assert isinstance(k, int) and k == kr == int(np.floor(samples))
    assert np.all(e_lib <= tol) and np.all(par <= tol)
    assert np.array_equal(H.numpy(), H.numpy().T) and h_error(H.numpy(), Hr) <= 1e-9


def test_imu_module_single_solve_and_spacing(cuda):
    from islam_amd import ops
    ph = physical_stream('12x10')
    ph = dict(ph, ref=np.array(ph['ref']))                # (a writable copy for torch)
    imu, n = _module(ph), len(ph['ref'])
    T, bias, H, res, k = imu.estimate_time_offset(0, n, ph['ref'], gn_rounds=0)
    # gn_rounds = 0 is one ops solve on the module's rows
    seg_host = np.ascontiguousarray(ph['seg'] - ph['seg'][0], dtype=np.int64)
    b0, b1 = int(ph['seg'][0]), int(ph['seg'][-1]) + 1
    seg = torch.from_numpy(seg_host).to(cuda)
    dts, gyros, accels = _t(cuda, ph['dt'][b0:b1]), _t(cuda, ph['gyro'][b0:b1]), _t(cuda, _acc(b1 - b0))
    init = _t(cuda, np.array([0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0]))
    _, rot, _ = ops.imu_preint(dts, gyros, accels, seg, seg_host, init[0:3], init[3:7], init[7:10], 0.0, True)
    jac = ops.imu_preint_bias_jac(dts, gyros, accels, seg, seg_host, True)
    ws, we = gyros[seg[:-1]].contiguous(), gyros[seg[1:]].contiguous()
    dbg, td, H1, res1, _ = ops.imu_time_offset_solve(jac, ops.imu_time_shift(rot, ws, we, 0.0), _t(cuda, ph['ref']), ws, we)
    assert float(T) == float(td) and torch.equal(bias, dbg.cpu()) and torch.equal(H, H1.cpu()) and torch.equal(res, res1.cpu())
    assert k == int(np.floor(float(td) / DT))
    # the module's rows are the restatement's
    xr = reference(physical_rows(ph))[0]
    assert np.all(differences(np.concatenate([bias.numpy(), [float(T)]]), xr) <= measured(linear_stream('12x10'))[3])
    # a spacing that is not uniform: the rounds refuse, the single solve does not
    dt = np.array(ph['dt'])
    dt[ph['seg'][3] + 2] *= 1.001
    odd = _module(ph, dt)
    with pytest.raises(ValueError, match='uniform'):
        odd.estimate_time_offset(0, n, ph['ref'])
    assert np.isfinite(float(odd.estimate_time_offset(0, n, ph['ref'], gn_rounds=0)[0]))
    # weights, the Huber rounds and solve_bias pass through
    w = np.ones(n)
    w[3] = 0.0
    T2, b2, H2, _, _ = imu.estimate_time_offset(0, n, ph['ref'], weight=w, solve_bias=False, delta=1e-3, rounds=2, gn_rounds=1)
    assert not b2.numpy().any() and not H2.numpy()[0:3].any() and np.isfinite(float(T2))
