"""CPU tests of the pre-integration bias Jacobians (islam_imu_preint_bias_jac, islam_imu_bias_correct, islam_imu_gyro_bias_solve,
IMUModule(bias_jac=True)): the symbols exist and validate their arguments on the host, the Python surface keeps the reference's
signature prefix, the new kernels do not spill, and the numpy restatement the GPU tests compare against
(tests/test_imu_bias_jac_gpu.py: jac_reference) reproduces the closed form for a sensor at rest and the central finite differences
of a plain numpy integrator of the same discretisation, to second order."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import test_imu_bias_jac_gpu as ref

SYMBOLS = ('islam_imu_preint_bias_jac_scratch_bytes', 'islam_imu_preint_bias_jac', 'islam_imu_bias_correct', 'islam_imu_gyro_bias_solve')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib
    for s in SYMBOLS + ('islam_imu_gyro_bias_solve_scratch_bytes',):
        assert s in _lib.SIGNATURES
        assert hasattr(lib._cdll, s), 'libislam_hip.so does not export %s' % s
    from islam_amd import ops
    assert callable(ops.imu_preint_bias_jac) and callable(ops.imu_bias_correct) and callable(ops.imu_gyro_bias_solve)


def test_scratch_bytes(lib):
    f = lib.islam_imu_preint_bias_jac_scratch_bytes
    assert f(0, 0) == 0
    prev = 0
    for n in (1, 2, 63, 64, 65, 300, 4096, 4097, 5000, 300000):
        b = f(10 * n + 1, n)
        assert b >= prev and b >= 73 * 8 * n       # at least one 28 + 45 double element per frame
        prev = b
    for n in (1, 64, 5000):
        assert f(1, n) <= f(1000, n) <= f(10 ** 9, n)
    assert f(50001, 5000) < 4 << 20
    g = lib.islam_imu_gyro_bias_solve_scratch_bytes
    assert 0 < g(0) <= g(1) <= g(5000) and g(5000) >= 9 * 8 * 5000


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    v = (ctypes.c_double * 3)(0.0, 0.0, 0.0)

    def bad(name, *args):
        assert getattr(lib, name)(*args) == -1
        assert name.encode() in lib.islam_last_error()

    j = 'islam_imu_preint_bias_jac'       # dt, gyro, acc, seg, nframes, S, maxF, init_jac, motion, out, scratch, dtype, stream
    bad(j, None, None, None, None, -1, 0, 0, None, 0, one, one, 1, None)          # nframes < 0
    bad(j, None, None, None, None, 1, -5, 0, None, 0, one, one, 1, None)          # S < 0
    bad(j, one, one, one, one, 2, 10, -1, None, 0, one, one, 1, None)             # a negative frame length
    bad(j, one, one, one, one, 2, 10, 11, None, 0, one, one, 1, None)             # a frame longer than the slice
    bad(j, None, one, one, one, 2, 10, 5, None, 1, one, one, 1, None)             # no dt
    bad(j, one, None, one, one, 2, 10, 5, None, 1, one, one, 1, None)             # no gyro
    bad(j, one, one, None, one, 2, 10, 5, None, 1, one, one, 1, None)             # no acc
    bad(j, one, one, one, None, 2, 10, 5, None, 0, one, one, 1, None)             # no frame offsets
    bad(j, one, one, one, one, 2, 10, 5, None, 0, None, one, 1, None)             # no output
    bad(j, one, one, one, one, 2, 10, 5, None, 1, None, one, 1, None)             # no output, motion mode
    bad(j, one, one, one, one, 2, 10, 5, None, 0, one, one, 7, None)              # dtype
    bad(j, one, one, one, one, 2, 10, 5, None, 0, one, None, 1, None)             # world mode without scratch
    c = 'islam_imu_bias_correct'          # jac, rot, vel, pos, rows, dbg, dba, out_rot, out_vel, out_pos, dtype, stream
    bad(c, one, one, one, one, -1, v, v, one, one, one, 1, None)
    bad(c, one, one, one, one, 4, v, v, one, one, one, 3, None)
    bad(c, one, one, one, one, 4, None, v, one, one, one, 1, None)
    bad(c, one, one, one, one, 4, v, None, one, one, one, 1, None)
    for k in (0, 1, 2, 3, 7, 8, 9):
        a = [one, one, one, one, 4, v, v, one, one, one, 1, None]
        a[k] = None
        bad(c, *a)
    s = 'islam_imu_gyro_bias_solve'       # jac, rot_imu, rot_ref, weight, rows, out_dbg, out_H, scratch, dtype, stream
    bad(s, one, one, one, None, -1, one, None, one, 1, None)
    bad(s, one, one, one, None, 4, one, None, one, 5, None)
    for k in (0, 1, 2, 5, 7):
        a = [one, one, one, None, 4, one, None, one, 1, None]
        a[k] = None
        bad(s, *a)


def test_ops_refuse_cpu_tensors(lib):
    import torch
    from islam_amd import ops
    z = torch.zeros
    seg = np.array([0, 2], dtype=np.int64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_preint_bias_jac(z(2, dtype=torch.float64), z(2, 3, dtype=torch.float64), z(2, 3, dtype=torch.float64), torch.from_numpy(seg), seg, True)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_bias_correct(z(1, 9, 6, dtype=torch.float64), z(1, 4), z(1, 3), z(1, 3), np.zeros(3), np.zeros(3))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_gyro_bias_solve(z(1, 9, 6, dtype=torch.float64), z(1, 4), z(1, 4))


def test_python_surface_keeps_the_reference_prefix():
    from islam_amd.imu_integrator import IMUModule
    ref_args = ['self', 'accels', 'gyros', 'dts', 'accel_bias', 'gyro_bias', 'init', 'gravity', 'rgb2imu_sync', 'device',
                'denoise_model_name', 'denoise_accel', 'denoise_gyro', 'use_est_cov']
    init = inspect.signature(IMUModule.__init__).parameters
    assert list(init)[:len(ref_args)] == ref_args
    for k in ('prop_cov', 'gyro_cov', 'acc_cov', 'bias_jac'):
        assert k in init and list(init).index(k) >= len(ref_args)
    assert init['bias_jac'].default is False and init['prop_cov'].default is False
    assert list(init).index('bias_jac') > list(init).index('acc_cov')       # behind the covariance's keywords: positional callers keep working
    integ = inspect.signature(IMUModule.integrate).parameters
    assert list(integ) == ['self', 'st', 'end', 'init', 'motion_mode', 'init_cov']
    assert list(inspect.signature(IMUModule.integrate_both).parameters) == ['self', 'st', 'end', 'init', 'init_cov']
    est = inspect.signature(IMUModule.estimate_gyro_bias).parameters
    assert list(est) == ['self', 'st', 'end', 'ref_rots', 'weight'] and est['weight'].default is None


def test_new_kernels_do_not_spill(lib):
    """No private memory and no spilled register in any kernel of csrc/imu_bias_jac.hip; LDS of the one-wavefront kernels as imu_cov.hip's
    (64 elements of 73 doubles)."""
    from tests import test_codeobj_cpu as co
    ks = {n: b for n, b in co._kernels().items() if any(k in n for k in ('bj_frame_reduce_kernel', 'bj_scan_kernel', 'bj_carry_kernel',
                                                                        'bj_rows_kernel', 'bias_correct_kernel', 'gyro_bias_solve_kernel'))}
    assert len(ks) == 9, sorted(ks)        # three templated on the I/O type
    for n, b in ks.items():
        assert co._field(b, 'private_segment_fixed_size') == 0 and co._field(b, 'vgpr_spill_count') == 0 and co._field(b, 'sgpr_spill_count') == 0, n
        assert co._field(b, 'group_segment_fixed_size') <= 64 * 73 * 8, n


@pytest.mark.parametrize('n,d', [(1, 0.01), (10, 0.005), (200, 0.0125)])
def test_restatement_matches_the_closed_form_at_rest(n, d):
    """w = 0, a constant: dr = Jr = DR = I, so the phi rows of J take -d I per sample and nothing else: J_phig = -n d I.  The b_a
    columns see A = [.. ; 0 I 0 ; 0 dI I] only: J_va <- J_va - d I, J_pa <- J_pa + d J_va - d^2/2 I, hence J_va = -n d I and, with
    J_va = -k d I in front of sample k,  J_pa = -sum_k (k d^2 + d^2 / 2) I = -(n (n - 1) / 2 + n / 2) d^2 I = -n^2 d^2 / 2 I.
    The b_g columns of the v and p rows follow the same way from A's first column, V = -[a]x d, P = -[a]x d^2 / 2, and
    J_phig = -k d I in front of sample k:  J_vg = [a]x d^2 sum_k k = [a]x d^2 n (n - 1) / 2,
    J_pg = sum_k ( d J_vg,k + [a]x d^3 k / 2 ) = [a]x d^3 ( sum_k k (k - 1) / 2 + sum_k k / 2 ) = [a]x d^3 (n - 1) n (2 n - 1) / 12."""
    a = np.array([0.3, -1.2, 9.7])
    acc, z = np.tile(a, (n, 1)), np.zeros((n, 3))
    ax = ref._hat(a)
    for motion in (True, False):
        out = ref.jac_reference(np.full(n, d), z, acc, np.array([0, n]), motion)
        J = out[-1]
        want = np.zeros((9, 6))
        want[0:3, 0:3] = -n * d * np.eye(3)
        want[3:6, 3:6] = -n * d * np.eye(3)
        want[6:9, 3:6] = -0.5 * n * n * d * d * np.eye(3)
        want[3:6, 0:3] = ax * d * d * n * (n - 1) / 2.0
        want[6:9, 0:3] = ax * d ** 3 * (n - 1) * n * (2 * n - 1) / 12.0
        assert ref.block_error(J, want) <= 1e-13
        if not motion:
            assert out.shape == (2, 9, 6) and not out[0].any()


@pytest.mark.parametrize('seed', [0, 1])
def test_restatement_matches_finite_differences_to_second_order(seed):
    """Central differences of integrate_reference (the plain numpy integrator of the same discretisation) in the six bias components,
    step h and h / 2: (f(-h e) - f(+h e)) / 2h -- the bias is SUBTRACTED from the samples -- with the rotation taken as the right
    perturbation Log(DR^T DR(b)).  The truncation error of a central difference is O(h^2): the error against jac_reference must fall
    by a ratio between 3 and 5.  h = 0.05 (rad/s, m/s^2) over T = 0.3 s: the next term of the difference is (h T)^2 ~ 2e-4 of the h^2
    one, and rounding is ~ 1e-16 |f| / h ~ 1e-14: the test checks that the error at h / 2 stands a factor 100 above that rounding level."""
    rng = np.random.default_rng(seed)
    n = 40
    dt, gyro = rng.uniform(0.004, 0.012, n), rng.normal(0, 0.5, (n, 3))
    acc = rng.normal(0, 1.0, (n, 3)) + np.array([0, 0, 9.81])
    J = ref.jac_reference(dt, gyro, acc, np.array([0, n]), True)[0]
    R0, v0, p0 = ref.integrate_reference(dt, gyro, acc)

    def fd(h):
        out = np.zeros((9, 6))
        for c in range(6):
            b = np.zeros(6)
            b[c] = h
            plus = ref.integrate_reference(dt, gyro - b[0:3], acc - b[3:6])
            minus = ref.integrate_reference(dt, gyro + b[0:3], acc + b[3:6])
            out[0:3, c] = (ref.log_so3(R0.T @ plus[0]) - ref.log_so3(R0.T @ minus[0])) / (2 * h)
            out[3:6, c] = (plus[1] - minus[1]) / (2 * h)
            out[6:9, c] = (plus[2] - minus[2]) / (2 * h)
        return out

    h = 0.05
    e1, e2 = np.abs(fd(h) - J), np.abs(fd(h / 2) - J)
    # the b_a columns are exactly linear in b_a (no truncation error): they must agree to rounding; the b_g columns carry the h^2 term
    scale = np.abs(J).max()
    rounding = 1e-16 * max(np.abs(v0).max(), 1.0) / (h / 2)
    assert e1[:, 3:6].max() <= 100 * rounding and e2[:, 3:6].max() <= 100 * rounding
    for rows in (slice(0, 3), slice(3, 6), slice(6, 9)):
        a, b = e1[rows, 0:3].max(), e2[rows, 0:3].max()
        print('rows %s: error %.3g at h, %.3g at h/2, ratio %.3g (rounding level %.1g, |J| %.3g)' % (rows, a, b, a / b, rounding, scale))
        assert b >= 100 * rounding
        assert 3.0 < a / b < 5.0
