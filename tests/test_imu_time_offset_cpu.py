"""CPU tests of the time-offset / gyro-bias solve (islam_imu_time_offset_solve, islam_imu_time_shift, ops.imu_time_offset_solve,
ops.imu_time_shift, IMUModule.estimate_time_offset): the symbols exist and validate their arguments on the host, the Python surface
refuses to run without a GPU, the new kernels use no private memory, and the numpy restatements the GPU tests compare against
(tests/test_imu_time_offset_gpu.py: time_offset_reference, loop_reference) recover the planted offset and bias of their planted streams."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import test_imu_time_offset_gpu as ref

SYMBOLS = ('islam_imu_time_offset_solve_scratch_bytes', 'islam_imu_time_offset_solve', 'islam_imu_time_shift')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib, ops
    from islam_amd.imu_integrator import IMUModule
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
        assert hasattr(lib._cdll, s), 'libislam_hip.so does not export %s' % s
    assert lib.islam_abi_version() == 1
    sol = inspect.signature(ops.imu_time_offset_solve).parameters
    assert list(sol) == ['jac', 'rot_imu', 'rot_ref', 'rate_start', 'rate_end', 'weight', 'solve_bias', 'delta', 'rounds']
    assert sol['weight'].default is None and sol['solve_bias'].default is True and sol['delta'].default is None and sol['rounds'].default == 4
    assert list(inspect.signature(ops.imu_time_shift).parameters) == ['rot', 'rate_start', 'rate_end', 'tau']
    est = inspect.signature(IMUModule.estimate_time_offset).parameters
    assert list(est) == ['self', 'st', 'end', 'ref_rots', 'weight', 'solve_bias', 'delta', 'rounds', 'gn_rounds']
    assert est['weight'].default is None and est['solve_bias'].default is True and est['delta'].default is None
    assert est['rounds'].default == 4 and est['gn_rounds'].default == 3
    doc = IMUModule.estimate_time_offset.__doc__
    assert 'ADD T to the camera' in doc and 'rgb2imu_sync' in doc and 'k samples' in doc
    # the older methods keep their surface
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(IMUModule.estimate_gyro_bias) == ['self', 'st', 'end', 'ref_rots', 'weight']
    assert sig(IMUModule.estimate_gravity_accel_bias) == ['self', 'st', 'end', 'ref_rots', 'ref_pos', 'weight', 'use_cov', 'gravity_norm']
    assert sig(IMUModule.estimate_lever_arm) == ['self', 'st', 'end', 'cam_rots', 'cam_pos', 'ext_rot', 'weight', 'use_cov', 'gravity_norm',
                                                 'solve_scale']
    assert sig(IMUModule.estimate_extrinsic_rotation) == ['self', 'st', 'end', 'cam_rots', 'weight', 'delta', 'rounds', 'min_gap']


def test_scratch_bytes(lib):
    f = lib.islam_imu_time_offset_solve_scratch_bytes
    assert f(0) > 0 and f(0) == f(-3)                      # the status words and the estimate alone
    prev = 0
    for n in (0, 1, 2, 3, 64, 257, 1024, 1025, 1100, 5000, 70001, 300007):
        b = f(n)
        assert b >= prev and b >= 8 * 14 * n               # at least the 10 + 4 terms of every row
        prev = b
    assert f(1) > f(0) and f(300007) < 40 * 10 ** 6


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    name = 'islam_imu_time_offset_solve'
    # jac, rot_imu, rot_ref, rate_start, rate_end, weight, rows, solve_bias, delta, rounds, out_x, out_H, out_res, scratch, dtype, stream
    good = [one, one, one, one, one, None, 4, 1, 0.0, 4, one, None, None, one, 1, None]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert getattr(lib, name)(*a) == -1
        assert name.encode() in lib.islam_last_error()

    bad(a6=-1)                           # rows < 0
    bad(a14=7)                           # dtype
    bad(a14=-1)
    bad(a7=2)                            # a flag that is neither 0 nor 1
    bad(a7=-1)
    bad(a8=-1e-3)                        # a negative threshold
    bad(a8=float('nan'))
    bad(a8=float('inf'))
    bad(a9=-1)                           # rounds < 0, with and without a threshold
    bad(a9=-1, a8=1e-3)
    for k in (1, 2, 3, 4, 10, 13):       # rot_imu, rot_ref, rate_start, rate_end, out_x, scratch
        bad(**{'a%d' % k: None})
    bad(a0=None)                         # no Jacobians with solve_bias = 1
    bad(a10=None, a6=0)                  # out_x and scratch are required whatever rows is
    bad(a13=None, a6=0)
    bad(a0=None, a7=0, a1=None)          # without the bias the Jacobians may be missing, the rotations may not
    name = 'islam_imu_time_shift'
    # rot, rate_start, rate_end, rows, tau, out_rot, dtype, stream
    good = [one, one, one, 4, 1e-3, one, 1, None]
    bad(a3=-1)
    bad(a6=7)
    bad(a4=float('nan'))                 # a shift that is not finite
    bad(a4=float('inf'))
    bad(a4=-float('inf'))
    for k in (0, 1, 2, 5):
        bad(**{'a%d' % k: None})
    assert lib.islam_imu_time_shift(None, None, None, 0, 0.0, None, 1, None) == 0     # no row: nothing to do


def test_python_surface_refuses_to_run_without_a_gpu(lib):
    import torch
    from islam_amd import ops
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_time_offset_solve(z(5, 9, 6), z(5, 4), z(5, 4), z(5, 3), z(5, 3))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_time_offset_solve(None, z(5, 4), z(5, 4), z(5, 3), z(5, 3), z(5), False, 1e-3, 2)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_time_shift(z(5, 4), z(5, 3), z(5, 3), 1e-3)


KERNELS = ('td_row_kernel', 'td_partial_kernel', 'td_solve_kernel', 'td_res_kernel', 'td_shift_kernel')


def test_new_kernels_use_no_private_memory(lib):
    """No scratch memory and no spilled register in any kernel of csrc/imu_time_offset.hip; the 4x4 of the solve lives in LDS.  Five
    kernels, three of them templated on the I/O type: eight code objects."""
    from tests import test_codeobj_cpu as co
    ks = {n: b for n, b in co._kernels().items() if any(k in n for k in KERNELS)}
    assert len(ks) == 8 and all(sum(k in n for n in ks) == (1 if k in ('td_partial_kernel', 'td_solve_kernel') else 2) for k in KERNELS), sorted(ks)
    assert sorted(ks) == sorted(n for n in co._kernels() if 'td_' in n)
    for n, b in ks.items():
        assert co._field(b, 'private_segment_fixed_size') == 0 and co._field(b, 'vgpr_spill_count') == 0 and co._field(b, 'sgpr_spill_count') == 0, n
        assert co._field(b, 'group_segment_fixed_size') <= 8192, n
    # the older tests count kernels by these substrings
    assert not any(s in n for n in ks for s in ('ga_', 'la_', 'ex_', 'bj_', 'bias_correct_kernel', 'gyro_bias_solve_kernel'))


# Rounding times conditioning with two decades of room, as for the other closed-form solves.  H is the matrix of the unknowns solved.
def _bound(H, x):
    on = np.flatnonzero(np.diag(H))
    return 100 * 2.0 ** -53 * np.linalg.cond(H[np.ix_(on, on)]) * np.abs(x).max()


@pytest.mark.parametrize('solve_bias', [True, False])
@pytest.mark.parametrize('name', ['5x7', '12xragged', '12x10', '70x10', '1024x4', '1025x4'])
def test_restatement_recovers_the_linear_exact_truth(name, solve_bias):
    st = ref.linear_stream(name, solve_bias)
    x, H, res, bad = ref.reference(st, solve_bias=solve_bias)
    back = ref.reference(st, reverse=True, solve_bias=solve_bias)
    e, o = ref.errors(x, st), ref.differences(x, back[0])
    on = np.flatnonzero(np.diag(H))
    print('%s solve_bias=%d: errors of (b, td) %s, forwards vs backwards %s, cond(H) %.3g, bound %.3g, largest residual %.3g'
          % (name, solve_bias, e, o, np.linalg.cond(H[np.ix_(on, on)]), _bound(H, x), res.max()))
    assert bad == 0 and np.array_equal(H, H.T)
    assert e.max() <= _bound(H, x) and o.max() <= _bound(H, x)
    if not solve_bias:
        assert not x[0:3].any() and not H[0:3].any() and not H[:, 0:3].any()
    # float32 I/O: both sides get the rounded inputs, and the planted pair is still there to the rounding of the inputs
    if name == '70x10':
        x32 = ref.reference(ref.rounded(st, np.float32), solve_bias=solve_bias)[0]
        print('float32 inputs: errors of (b, td) %s' % ref.errors(x32, st))
        assert ref.errors(x32, st).max() <= 1e-3 * np.abs(x).max()


@pytest.mark.parametrize('name', ['12x10', '70x10'])
def test_restatement_is_second_order_on_the_physical_truth(name):
    err = []
    for scale in (1.0, 0.5):
        st = ref.physical_rows(ref.physical_stream(name, scale))
        err.append(ref.errors(ref.reference(st)[0], st))
    print('%s physical: errors of (b, td) %s at full, %s at half, ratio %s' % (name, err[0], err[1], err[0] / err[1]))
    assert np.all(err[0] > 3.0 * err[1])
    assert err[0][0] < 0.05 * np.abs(ref.B_PLANTED).max() and err[0][1] < 0.05 * ref.TD_PLANTED


@pytest.mark.parametrize('samples', [2.4, -1.7, 0.5])
def test_restatement_round_loop_converges(samples):
    """|dT| <= 1e-13 s and |db| <= 1e-13 rad/s after three rounds, no worse after four; without the sub-sample shift the loop stalls
    orders of magnitude above that: the case that shows the shift is wired in."""
    ph = ref.physical_stream('12x10', 1.0, samples * ref.DT)
    a = (ph['dt'], ph['gyro'], ph['seg'], ph['ref'])
    e = {}
    for g in (0, 1, 2, 3, 4):
        T, b, _, res, k = ref.loop_reference(*a, g)
        e[g] = (np.abs(b - ph['b']).max(), abs(T - ph['td']))
    Tn, bn, _, _, kn = ref.loop_reference(*a, 4, shift=False)
    print('td = %+.1f samples: errors of (b, T) after 0..4 further rounds %s; without the shift %s'
          % (samples, [tuple(float('%.2g' % v) for v in e[g]) for g in e], (np.abs(bn - ph['b']).max(), abs(Tn - ph['td']))))
    assert k == int(np.floor(samples))
    assert max(e[3]) <= 1e-13 and max(e[4]) <= 1e-13
    if samples != int(samples) and abs(samples) > 1:
        assert abs(Tn - ph['td']) >= 1e-9


def test_restatement_huber_gain():
    st = ref.huber_stream()
    plain, robust = ref.reference(st), ref.reference(st, delta=1e-3, rounds=4)
    e0, e4 = ref.errors(plain[0], st), ref.errors(robust[0], st)
    print('huber: errors of (b, td) %s plain, %s after 4 rounds; residuals of the outliers %s' % (e0, e4, robust[2][list(ref.OUTLIERS)]))
    assert e0[1] >= 10.0 * e4[1]
    assert np.all(np.abs(robust[2][list(ref.OUTLIERS)] - 0.3) < 0.01)


def test_restatement_weights_and_exclusion():
    st = ref.linear_stream('12xragged')
    n = len(st['rot'])
    w = np.ones(n)
    w[4] = 0.0
    dirty = dict(st, ref=st['ref'].copy())
    dirty['ref'][4, 0] = np.nan
    clean, nan4 = ref.reference(st, weight=w), ref.reference(dirty, weight=w)
    assert clean[3] == 0 and nan4[3] == 0 and np.array_equal(clean[0], nan4[0]) and np.isnan(nan4[2][4]) and np.isfinite(clean[2][4])
    assert ref.reference(dirty)[3] == 1 and np.array_equal(ref.reference(dirty)[0], clean[0])
    w[5] = -2.0
    assert ref.reference(st, weight=w)[3] == 1
    w[5] = np.inf
    assert ref.reference(st, weight=w)[3] == 1
    with pytest.raises(np.linalg.LinAlgError, match='pivot 0: 0 of 0'):       # no row takes part
        ref.reference(st, weight=np.zeros(n))


@pytest.mark.parametrize('solve_bias,pivot', [(True, 3), (False, 0)])
def test_restatement_without_a_change_of_rate(solve_bias, pivot):
    """What the GPU test of ISLAM_ENOTPD rests on: a constant rate about a fixed axis makes u_i exactly 0, so the pivot of td is exactly 0
    with either solve_bias."""
    st = ref.constant_rate_rows()
    assert not ref._u(st['rot'], st['ws'], st['we']).any()
    with pytest.raises(np.linalg.LinAlgError, match='pivot %d: 0 of 0' % pivot):
        ref.reference(st, solve_bias=solve_bias)
