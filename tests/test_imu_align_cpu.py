"""CPU tests of the gravity / accelerometer-bias / velocity solve (islam_imu_gravity_bias_solve, ops.imu_gravity_bias_solve,
IMUModule.estimate_gravity_accel_bias): the symbols exist and validate their arguments on the host, the Python surface refuses to run
without a GPU, the new kernels use no private memory, and the numpy restatement the GPU tests compare against
(tests/test_imu_align_gpu.py: align_reference) recovers the planted gravity, bias and velocities of its planted streams."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import test_imu_align_gpu as ref

SYMBOLS = ('islam_imu_gravity_bias_solve_scratch_bytes', 'islam_imu_gravity_bias_solve')


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
    assert list(inspect.signature(ops.imu_gravity_bias_solve).parameters) == ['rot_ref', 'pos_ref', 'dts', 'dvel', 'dpos', 'jac', 'cov', 'weight',
                                                                             'gravity_norm']
    est = inspect.signature(IMUModule.estimate_gravity_accel_bias).parameters
    assert list(est) == ['self', 'st', 'end', 'ref_rots', 'ref_pos', 'weight', 'use_cov', 'gravity_norm']
    assert est['weight'].default is None and est['use_cov'].default is False and est['gravity_norm'].default is None


def test_scratch_bytes(lib):
    f = lib.islam_imu_gravity_bias_solve_scratch_bytes
    assert f(0) > 0 and f(0) == f(1) == f(-3)              # the status words alone
    prev = 0
    for n in (0, 1, 2, 3, 64, 257, 1025, 1026, 1100, 5000, 300007):
        b = f(n)
        assert b >= prev and b >= 8 * 27 * max(n - 1, 0)   # at least the 21 + 6 terms of every pair
        prev = b
    assert f(300007) < 80 << 20


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    name = 'islam_imu_gravity_bias_solve'
    # rot_ref, pos_ref, dts, dvel, dpos, jac, cov, weight, rows, gravity_norm, out_x, out_H, out_vel, scratch, dtype, stream
    good = [one, one, one, one, one, None, None, None, 4, 0.0, one, None, None, one, 1, None]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert getattr(lib, name)(*a) == -1
        assert name.encode() in lib.islam_last_error()

    bad(a8=-1)                           # rows < 0
    bad(a14=7)                           # dtype
    bad(a14=-1)
    bad(a9=-9.81)                        # a negative magnitude
    bad(a9=float('nan'))
    bad(a9=float('inf'))
    for k in (0, 1, 2, 3, 4, 10, 13):    # rot_ref, pos_ref, dts, dvel, dpos, out_x, scratch
        bad(**{'a%d' % k: None})
    bad(a0=None, a8=0)                   # the one pose of rows = 0 is still required
    bad(a10=None, a8=1)


def test_python_surface_refuses_to_run_without_a_gpu(lib):
    import torch
    from islam_amd import ops
    from islam_amd.imu_integrator import IMUModule
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_gravity_bias_solve(z(5, 4), z(5, 3), z(4), z(4, 3), z(4, 3))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_gravity_bias_solve(z(5, 4), z(5, 3), z(4), z(4, 3), z(4, 3), z(4, 9, 6), z(4, 9, 9), z(3), 9.81)
    with pytest.raises(RuntimeError):
        IMUModule(torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5), device='cpu')


def test_new_kernels_use_no_private_memory(lib):
    """No scratch memory and no spilled register in any kernel of csrc/imu_align.hip; the small matrices of the solve live in LDS.  Four
    kernels at two numbers of unknowns (6: this solve, 10: the lever / scale solve), two of the four also at two I/O types."""
    from tests import test_codeobj_cpu as co
    ks = {n: b for n, b in co._kernels().items() if 'ga_' in n}
    assert len(ks) == 12, sorted(ks)
    for nx, lds in (('ILi6E', 4096), ('ILi10E', 8192)):
        for k, count in (('ga_pair_kernel', 2), ('ga_partial_kernel', 1), ('ga_solve_kernel', 1), ('ga_vel_kernel', 2)):
            assert sum(k + nx in n for n in ks) == count, (k, nx, sorted(ks))
        for n, b in ks.items():
            if nx in n:
                assert co._field(b, 'private_segment_fixed_size') == 0 and co._field(b, 'vgpr_spill_count') == 0, n
                assert co._field(b, 'sgpr_spill_count') == 0, n
                assert co._field(b, 'group_segment_fixed_size') <= lds, n


# the issue's CPU figures for these streams (worst error of (g, b)): 4e-12, 6e-13, 4e-14, 3e-13 at cond(H) 1e7, 2e4, 45, 41.  The bound
# here is rounding times conditioning with two decades of room.  Two things are rounded: the solve, cond(H) |x| 2^-53, and the data:
# g is a second difference of the positions over d^2, so a rounding of p moves it by 4 |p| 2^-53 / d^2 whatever cond(H) is.
def _bound(st, H, x):
    return 100 * 2.0 ** -53 * (np.linalg.cond(H) * np.abs(x).max() + 4 * np.abs(st['p']).max() / st['d'].min() ** 2)


@pytest.mark.parametrize('name', ['4x7', '12xragged', '70x10', '300x10'])
def test_restatement_recovers_the_planted_truth(name):
    st = ref.planted_stream(name)
    x, H, vel, bad = ref._reference(st)
    e = ref.errors(x, vel, st)
    cond = np.linalg.cond(H)
    print('%s: errors of (g, b, v) %s, cond(H) %.3g' % (name, e, cond))
    assert bad == 0 and np.array_equal(H, H.T)
    assert e.max() <= _bound(st, H, x)
    # the same with the known magnitude, and without Jacobians on the stream that carries no bias
    G = float(np.linalg.norm(st['g']))
    xn, _, veln, _ = ref._reference(st, gravity_norm=G)
    assert ref.errors(xn, veln, st).max() <= _bound(st, H, x)
    s0 = ref.planted_stream(name, bias=False)
    x0, H0, vel0, _ = ref._reference(s0, jac=False)
    assert ref.errors(x0, vel0, s0).max() <= _bound(s0, H0[:3, :3], x0) and not x0[3:6].any()


def test_restatement_weights_and_exclusion():
    st = ref.planted_stream('12xragged')
    n = len(st['d'])
    w = np.ones(n - 1)
    w[4] = 0.0
    dp = st['dp'].copy()
    dp[5, 0] = np.nan                    # pairs 4 and 5 read it
    clean = ref.align_reference(st['quat'], st['p'], st['d'], st['dv'], st['dp'], st['jac'], weight=w)
    dirty = ref.align_reference(st['quat'], st['p'], st['d'], st['dv'], dp, st['jac'], weight=w)
    assert dirty[3] == 1 and clean[3] == 0
    w[5] = 0.0
    both = ref.align_reference(st['quat'], st['p'], st['d'], st['dv'], dp, st['jac'], weight=w)
    assert both[3] == 0 and np.array_equal(both[0], dirty[0]) and np.array_equal(both[1], dirty[1])
