"""CPU tests of the lever-arm / scale solve (islam_imu_lever_scale_solve, ops.imu_lever_scale_solve, IMUModule.estimate_lever_arm): the
symbols exist and validate their arguments on the host, the Python surface refuses to run without a GPU, the new kernels use no
private memory, and the numpy restatement the GPU tests compare against (tests/test_imu_lever_gpu.py: lever_reference) recovers the
planted gravity, bias, lever arm, scale and velocities of its planted streams."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import test_imu_lever_gpu as ref

SYMBOLS = ('islam_imu_lever_scale_solve_scratch_bytes', 'islam_imu_lever_scale_solve')


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
    sol = inspect.signature(ops.imu_lever_scale_solve).parameters
    assert list(sol) == ['rot_body', 'pos_cam', 'dts', 'dvel', 'dpos', 'jac', 'cov', 'weight', 'solve_lever', 'solve_scale', 'gravity_norm']
    assert all(sol[k].default is None for k in ('jac', 'cov', 'weight', 'gravity_norm'))
    assert sol['solve_lever'].default is True and sol['solve_scale'].default is False
    est = inspect.signature(IMUModule.estimate_lever_arm).parameters
    assert list(est) == ['self', 'st', 'end', 'cam_rots', 'cam_pos', 'ext_rot', 'weight', 'use_cov', 'gravity_norm', 'solve_scale']
    assert est['weight'].default is None and est['use_cov'].default is False and est['gravity_norm'].default is None
    assert est['solve_scale'].default is False
    # the older method keeps its surface
    old = inspect.signature(IMUModule.estimate_gravity_accel_bias).parameters
    assert list(old) == ['self', 'st', 'end', 'ref_rots', 'ref_pos', 'weight', 'use_cov', 'gravity_norm']


def test_scratch_bytes(lib):
    f = lib.islam_imu_lever_scale_solve_scratch_bytes
    assert f(0) > 0 and f(0) == f(1) == f(-3)              # the status words alone
    prev = 0
    for n in (0, 1, 2, 3, 64, 257, 1025, 1026, 1100, 5000, 300007):
        b = f(n)
        assert b >= prev and b >= 8 * 65 * max(n - 1, 0)   # at least the 55 + 10 terms of every pair
        prev = b
    assert f(300007) < 170 * 10 ** 6


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    name = 'islam_imu_lever_scale_solve'
    # rot_body, pos_cam, dts, dvel, dpos, jac, cov, weight, rows, solve_lever, solve_scale, gravity_norm, out_x, out_H, out_vel, scratch,
    # dtype, stream
    good = [one, one, one, one, one, None, None, None, 4, 1, 0, 0.0, one, None, None, one, 1, None]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert getattr(lib, name)(*a) == -1
        assert name.encode() in lib.islam_last_error()

    bad(a8=-1)                           # rows < 0
    bad(a16=7)                           # dtype
    bad(a16=-1)
    bad(a11=-9.81)                       # a negative magnitude
    bad(a11=float('nan'))
    bad(a11=float('inf'))
    bad(a9=2)                            # a flag that is neither 0 nor 1
    bad(a10=2)
    bad(a9=-1)
    bad(a10=-1, a9=1)
    bad(a9=0, a10=0)                     # nothing beyond the gravity / bias solve is asked for: the message names that solve
    assert b'islam_imu_gravity_bias_solve' in lib.islam_last_error()
    for k in (0, 1, 2, 3, 4, 12, 15):    # rot_body, pos_cam, dts, dvel, dpos, out_x, scratch
        bad(**{'a%d' % k: None})
    bad(a0=None, a8=0)                   # the one pose of rows = 0 is still required
    bad(a12=None, a8=1)


def test_python_surface_refuses_to_run_without_a_gpu(lib):
    import torch
    from islam_amd import ops
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_lever_scale_solve(z(5, 4), z(5, 3), z(4), z(4, 3), z(4, 3))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_lever_scale_solve(z(5, 4), z(5, 3), z(4), z(4, 3), z(4, 3), z(4, 9, 6), z(4, 9, 9), z(3), True, True, 9.81)


def test_new_kernels_use_no_private_memory(lib):
    """No scratch memory and no spilled register in the kernels of this solve, csrc/imu_align.hip's at ten unknowns; the small matrices of
    the solve live in LDS."""
    from tests import test_codeobj_cpu as co
    ks = {n: b for n, b in co._kernels().items()
          if any(k + 'ILi10E' in n for k in ('ga_pair_kernel', 'ga_partial_kernel', 'ga_solve_kernel', 'ga_vel_kernel'))}
    assert len(ks) == 6, sorted(ks)        # two templated on the I/O type
    for n, b in ks.items():
        assert co._field(b, 'private_segment_fixed_size') == 0 and co._field(b, 'vgpr_spill_count') == 0 and co._field(b, 'sgpr_spill_count') == 0, n
        assert co._field(b, 'group_segment_fixed_size') <= 8192, n


# The bound is rounding times conditioning with two decades of room, as for the gravity / bias solve.  Two things are rounded: the solve,
# cond(H) |x| 2^-53, and the data: g (and with it everything else) rests on a second difference of the positions over d^2, so a rounding
# of q moves it by 4 |q| 2^-53 / d^2 whatever cond(H) is.  H is the matrix of the unknowns that are solved.
def _bound(st, H, x):
    on = np.flatnonzero(np.diag(H))
    return 100 * 2.0 ** -53 * (np.linalg.cond(H[np.ix_(on, on)]) * np.abs(x).max() + 4 * np.abs(st['q']).max() / st['d'].min() ** 2)


@pytest.mark.parametrize('which', list(ref.SETS))
@pytest.mark.parametrize('name', ['5x7', '12xragged', '70x10', '300x10'])
def test_restatement_recovers_the_planted_truth(name, which):
    st = ref.lever_stream(name, which)
    x, H, vel, bad = ref._reference(st)
    back = ref._reference(st, reverse=True)
    e = ref.errors(x, vel, st)
    print('%s %s: errors of (g, b, t, s, v) %s, forwards vs backwards %s, cond(H) %.3g, bound %.3g'
          % (name, which, e, ref.differences(x, vel, back[0], back[2]), np.linalg.cond(H[np.ix_(*[np.flatnonzero(np.diag(H))] * 2)]), _bound(st, H, x)))
    assert bad == 0 and np.array_equal(H, H.T)
    assert e.max() <= _bound(st, H, x)
    assert ref.differences(x, vel, back[0], back[2]).max() <= _bound(st, H, x)
    if not st['lever']:
        assert not x[6:9].any() and not H[6:9].any()
    if not st['scale']:
        assert x[9] == 1.0 and not H[9].any()
    # the same with the known magnitude, and without Jacobians on the stream that carries no bias
    G = float(np.linalg.norm(st['g']))
    xn, _, veln, _ = ref._reference(st, gravity_norm=G)
    assert ref.errors(xn, veln, st).max() <= _bound(st, H, x) and abs(np.linalg.norm(xn[0:3]) - G) <= 1e-12 * G
    s0 = ref.lever_stream(name, which, bias=False)
    x0, H0, vel0, _ = ref._reference(s0, jac=False)
    assert ref.errors(x0, vel0, s0).max() <= _bound(s0, H0, x0) and not x0[3:6].any() and not H0[3:6].any()


def test_restatement_weights_and_exclusion():
    st = ref.lever_stream('12xragged', 'both')
    n = len(st['d'])
    w = np.ones(n - 1)
    w[4] = 0.0
    dp = st['dp'].copy()
    dp[5, 0] = np.nan                    # pairs 4 and 5 read it
    a = (st['quat'], st['q'], st['d'], st['dv'])
    clean = ref.lever_reference(*a, st['dp'], st['jac'], weight=w, solve_scale=True)
    dirty = ref.lever_reference(*a, dp, st['jac'], weight=w, solve_scale=True)
    assert dirty[3] == 1 and clean[3] == 0
    w[5] = 0.0
    both = ref.lever_reference(*a, dp, st['jac'], weight=w, solve_scale=True)
    assert both[3] == 0 and np.array_equal(both[0], dirty[0]) and np.array_equal(both[1], dirty[1])


def test_restatement_without_rotation():
    """What the GPU test of ISLAM_ENOTPD rests on: without rotation (and without Jacobians) the lever columns are exact zeros, so the
    restatement's first pivot of t fails exactly; with the lever off and the scale on the four unknowns are recovered."""
    flat = ref.lever_stream('70x10', 'both', bias=False, amp=0.0)
    assert all(np.array_equal(u, flat['quat'][0]) for u in flat['quat'])
    with pytest.raises(np.linalg.LinAlgError, match='pivot 3: 0 of 0'):
        ref._reference(flat, jac=False)
    with pytest.raises(np.linalg.LinAlgError):      # with Jacobians b is unobservable without rotation: an earlier pivot fails
        ref._reference(dict(flat, lever=False))
    only = dict(flat, lever=False, t=np.zeros(3))
    x, H, vel, bad = ref._reference(only, jac=False)
    e = ref.errors(x, vel, only)
    print('no rotation, scale only: errors of (g, b, t, s, v) %s, bound %.3g' % (e, _bound(only, H, x)))
    assert bad == 0 and e.max() <= _bound(only, H, x)
