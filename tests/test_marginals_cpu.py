"""Host-only parts of the marginal-covariance entry points (no GPU needed): workspace size, argument checks, the plan and the
Python signature."""
import ctypes
import inspect

import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_workspace_bytes_monotone_and_covers_the_solver(lib):
    assert lib.islam_pvgo_marginals_workspace_bytes(0) == 0
    prev = 0
    for N in list(range(1, 200)) + [257, 1000, 5001, 5002, 30011, 300007]:
        b = lib.islam_pvgo_marginals_workspace_bytes(N)
        assert b >= prev and b >= lib.islam_pvgo_workspace_bytes(N) > 0
        prev = b


def test_argument_errors_before_any_device_work(lib):
    sl = (ctypes.c_int * 2)(0, 0)
    nb = lib.islam_pvgo_marginals_workspace_bytes(9)
    fake = ctypes.c_void_p(4096)                  # never dereferenced: the checks run first
    assert lib.islam_pvgo_marginals(fake, fake, 0, 0, sl, fake, nb, fake, fake, None) == -1
    assert lib.islam_pvgo_marginals(fake, fake, 9, 9, sl, fake, nb, fake, fake, None) == -1
    assert b'anchor' in lib.islam_last_error()
    assert lib.islam_pvgo_marginals(fake, fake, 9, -2, sl, fake, nb, fake, fake, None) == -1
    assert lib.islam_pvgo_marginals(fake, fake, 9, 0, sl, fake, nb - 1, fake, fake, None) == -1
    assert b'workspace' in lib.islam_last_error()
    assert lib.islam_pvgo_marginals_enqueue(fake, fake, 9, 9, sl, fake, nb, fake, fake, None, None) == -1


def test_plan_small_chain_is_one_level(lib):
    from islam_amd import ops
    assert ops.pvgo_marginals_plan(9) == [(9, 9, 1)]            # one launch: the top kernel
    levels = ops.pvgo_marginals_plan(5001)
    assert 2 <= len(levels) <= 6 and levels[0][0] == 5001
    for (n, m, P), nxt in zip(levels, levels[1:]):
        assert nxt[0] == n // (m + 1) and P == (n + m) // (m + 1)


def test_python_surface():
    from islam_amd import ops, pvgo
    sig = inspect.signature(pvgo.pvgo_marginals)
    assert list(sig.parameters) == ['nodes', 'vels', 'vo_motions', 'dts', 'imu_drots', 'imu_dtrans', 'imu_dvels', 'loss_weight',
                                    'reproj', 'anchor']
    assert sig.parameters['loss_weight'].default == (1, 1, 1, 1)
    assert sig.parameters['reproj'].default is None and sig.parameters['anchor'].default == 0
    osig = inspect.signature(ops.pvgo_marginals)
    assert list(osig.parameters)[:5] == ['Hd', 'Ho', 'anchor', 'seg_len', 'workspace']
    assert osig.parameters['anchor'].default == 0 and osig.parameters['seg_len'].default == (0, 0)
    assert inspect.signature(pvgo.run_pvgo).parameters['marginals'].default is False
    for name in ('node_cov', 'cross', 'pose_cov', 'vel_cov'):
        assert hasattr(pvgo.PvgoMarginals, name) or name in inspect.signature(pvgo.PvgoMarginals.__init__).parameters
