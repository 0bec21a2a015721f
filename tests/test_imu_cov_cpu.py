"""CPU tests of the pre-integration covariance (islam_imu_preint_cov, IMUModule(prop_cov=True)): the symbols exist and validate their
arguments on the host, the Python surface keeps the reference's signature prefix, and the numpy restatement the GPU tests compare
against (tests/test_imu_cov_gpu.py: cov_reference) reproduces the closed form of the recurrence for a sensor at rest."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import test_imu_cov_gpu as ref


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib
    for s in ('islam_imu_preint_cov_scratch_bytes', 'islam_imu_preint_cov'):
        assert s in _lib.SIGNATURES
        assert hasattr(lib._cdll, s), 'libislam_hip.so does not export %s' % s
    from islam_amd import ops
    assert callable(ops.imu_preint_cov)


def test_scratch_bytes(lib):
    f = lib.islam_imu_preint_cov_scratch_bytes
    assert f(0, 0) == 0
    prev = 0
    for n in (1, 2, 63, 64, 65, 300, 4096, 4097, 5000, 300000):
        b = f(10 * n + 1, n)
        assert b >= prev and b >= 73 * 8 * n       # at least one 28 + 45 double element per frame
        prev = b
    for n in (1, 64, 5000):
        assert f(1, n) <= f(1000, n) <= f(10 ** 9, n)
    assert f(50001, 5000) < 4 << 20


def test_bad_arguments_fail_on_the_host(lib):
    f = lib.islam_imu_preint_cov
    v = (ctypes.c_double * 3)(1e-8, 1e-8, 1e-8)
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work

    def bad(*args):
        assert f(*args) == -1
        assert b'islam_imu_preint_cov' in lib.islam_last_error()

    bad(None, None, None, None, -1, 0, 0, v, v, None, None, None, 0, one, one, 1, None)         # nframes < 0
    bad(None, None, None, None, 1, -5, 0, v, v, None, None, None, 0, one, one, 1, None)         # S < 0
    bad(one, one, one, one, 2, 10, 11, v, v, None, None, None, 0, one, one, 1, None)            # a frame longer than the slice
    bad(one, one, one, one, 2, 10, 5, None, v, None, None, None, 0, one, one, 1, None)          # no gyro variances
    bad(one, one, one, one, 2, 10, 5, v, None, None, None, None, 0, one, one, 1, None)          # no accelerometer variances
    bad(one, one, one, one, 2, 10, 5, v, v, None, None, None, 0, None, one, 1, None)            # no output
    bad(one, one, one, None, 2, 10, 5, v, v, None, None, None, 0, one, one, 1, None)            # no frame offsets
    bad(None, one, one, one, 2, 10, 5, v, v, None, None, None, 1, one, one, 1, None)            # no dt
    bad(one, None, one, one, 2, 10, 5, v, v, None, None, None, 1, one, one, 1, None)            # no gyro
    bad(one, one, None, one, 2, 10, 5, v, v, None, None, None, 1, one, one, 1, None)            # no acc
    bad(one, one, one, one, 2, 10, 5, v, v, None, None, None, 0, one, None, 1, None)            # world mode without scratch
    bad(one, one, one, one, 2, 10, 5, v, v, None, None, None, 0, one, one, 7, None)             # dtype
    neg = (ctypes.c_double * 3)(1e-8, -1e-8, 1e-8)
    bad(one, one, one, one, 2, 10, 5, neg, v, None, None, None, 0, one, one, 1, None)           # negative variance
    nan = (ctypes.c_double * 3)(1e-8, float('nan'), 1e-8)
    bad(one, one, one, one, 2, 10, 5, v, nan, None, None, None, 0, one, one, 1, None)


def test_python_surface_keeps_the_reference_prefix():
    from islam_amd.imu_integrator import IMUModule
    ref_args = ['self', 'accels', 'gyros', 'dts', 'accel_bias', 'gyro_bias', 'init', 'gravity', 'rgb2imu_sync', 'device',
                'denoise_model_name', 'denoise_accel', 'denoise_gyro', 'use_est_cov']
    init = inspect.signature(IMUModule.__init__).parameters
    assert list(init)[:len(ref_args)] == ref_args
    for k in ('prop_cov', 'gyro_cov', 'acc_cov'):
        assert k in init and list(init).index(k) >= len(ref_args)
    assert init['prop_cov'].default is False
    assert init['gyro_cov'].default == (1.6968e-4) ** 2 and init['acc_cov'].default == (2.0e-3) ** 2
    integ = inspect.signature(IMUModule.integrate).parameters
    assert list(integ)[:5] == ['self', 'st', 'end', 'init', 'motion_mode']
    assert list(integ)[-1] == 'init_cov' and integ['init_cov'].default is None
    both = inspect.signature(IMUModule.integrate_both).parameters
    assert list(both)[:4] == ['self', 'st', 'end', 'init'] and both['init_cov'].default is None


@pytest.mark.parametrize('n,d', [(1, 0.01), (10, 0.005), (200, 0.0125)])
def test_restatement_matches_the_closed_form_at_rest(n, d):
    """gyro = acc = 0: A = [I 0 0; 0 I 0; 0 dI I], so with k = n - 1 - j steps left after sample j
       Sphiphi = n sg d^2,  Svv = n sa d^2,  Spv = sa d^3 sum (1/2 + k),  Spp = sa d^4 sum (1/2 + k)^2   (each times I)."""
    sg, sa = np.array([2.0e-8, 3.0e-8, 5.0e-8]), np.array([4.0e-6, 1.0e-6, 9.0e-6])
    z = np.zeros((n, 3))
    for motion in (True, False):
        out = ref.cov_reference(np.full(n, d), z, z, np.array([0, n]), sg, sa, motion)
        S = out[-1]
        k = np.arange(n)
        want = np.zeros((9, 9))
        want[0:3, 0:3] = np.diag(n * sg * d * d)
        want[3:6, 3:6] = np.diag(n * sa * d * d)
        want[6:9, 3:6] = want[3:6, 6:9] = np.diag(sa * d ** 3 * np.sum(0.5 + k))
        want[6:9, 6:9] = np.diag(sa * d ** 4 * np.sum((0.5 + k) ** 2))
        assert ref.cs_error(S, want) <= 1e-13
        if not motion:
            assert out.shape == (2, 9, 9) and not out[0].any()
