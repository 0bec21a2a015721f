"""CPU tests of the camera-IMU extrinsic-rotation solve (islam_imu_extrinsic_rot_solve, ops.imu_extrinsic_rot_solve,
IMUModule.estimate_extrinsic_rotation): the symbols exist and validate their arguments on the host, the Python surface refuses to run
without a GPU, the new kernels use no private memory, and the numpy restatement the GPU tests compare against
(tests/test_imu_extrinsic_gpu.py: extrinsic_reference) recovers the planted mount and shows the gain of the Huber rounds."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import test_imu_extrinsic_gpu as ref

SYMBOLS = ('islam_imu_extrinsic_rot_solve_scratch_bytes', 'islam_imu_extrinsic_rot_solve')


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
    sig = inspect.signature(ops.imu_extrinsic_rot_solve).parameters
    assert list(sig) == ['rot_imu', 'rot_cam', 'weight', 'delta', 'rounds']
    assert sig['weight'].default is None and sig['delta'].default is None and sig['rounds'].default == 4
    est = inspect.signature(IMUModule.estimate_extrinsic_rotation).parameters
    assert list(est) == ['self', 'st', 'end', 'cam_rots', 'weight', 'delta', 'rounds', 'min_gap']
    assert est['weight'].default is None and est['delta'].default is None and est['rounds'].default == 4 and est['min_gap'].default is None
    doc = IMUModule.estimate_extrinsic_rotation.__doc__
    assert 'rgb2imu_pose' in doc and 'estimate_gyro_bias' in doc and 'lever arm' in doc and 'time offset' in doc


def test_scratch_bytes(lib):
    f = lib.islam_imu_extrinsic_rot_solve_scratch_bytes
    assert f(0) > 0 and f(0) == f(-3)                      # the status words and the estimate alone
    prev = 0
    for n in (0, 1, 2, 3, 64, 257, 1024, 1025, 1100, 5000, 70001, 300007):
        b = f(n)
        assert b >= prev and b >= 8 * 11 * n               # at least the 10 terms and the excluded flag of every pair
        prev = b
    assert f(1) > f(0) and f(300007) < 64 << 20


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    name = 'islam_imu_extrinsic_rot_solve'
    # rot_imu, rot_cam, weight, rows, delta, rounds, out_q, out_eig, out_res, scratch, dtype, stream
    good = [one, one, None, 4, 0.0, 4, one, one, None, one, 1, None]

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        assert getattr(lib, name)(*a) == -1
        assert name.encode() in lib.islam_last_error()

    bad(a3=-1)                           # rows < 0
    bad(a10=7)                           # dtype
    bad(a10=-1)
    bad(a4=-1e-3)                        # a negative threshold
    bad(a4=float('nan'))
    bad(a4=float('inf'))
    bad(a5=-1)                           # rounds < 0, with and without a threshold
    bad(a5=-1, a4=1e-3)
    for k in (0, 1, 6, 7, 9):            # rot_imu, rot_cam, out_q, out_eig, scratch
        bad(**{'a%d' % k: None})
    bad(a6=None, a3=0)                   # the outputs are required whatever rows is
    bad(a9=None, a3=0)


def test_python_surface_refuses_to_run_without_a_gpu(lib):
    import torch
    from islam_amd import ops
    from islam_amd.imu_integrator import IMUModule
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_extrinsic_rot_solve(z(5, 4), z(5, 4))
    with pytest.raises(RuntimeError, match='no CPU path'):
        ops.imu_extrinsic_rot_solve(z(5, 4), z(5, 4), z(5), 1e-3, 2)
    with pytest.raises(RuntimeError):
        IMUModule(torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(5), device='cpu')


def test_new_kernels_use_no_private_memory(lib):
    """No scratch memory and no spilled register in any kernel of csrc/imu_extrinsic.hip; the 4x4 of the solve lives in LDS."""
    from tests import test_codeobj_cpu as co
    ks = {n: b for n, b in co._kernels().items() if any(k in n for k in ('ex_pair_kernel', 'ex_partial_kernel', 'ex_solve_kernel', 'ex_res_kernel'))}
    assert len(ks) == 6, sorted(ks)        # two templated on the I/O type
    for n, b in ks.items():
        assert co._field(b, 'private_segment_fixed_size') == 0 and co._field(b, 'vgpr_spill_count') == 0 and co._field(b, 'sgpr_spill_count') == 0, n
        assert co._field(b, 'group_segment_fixed_size') <= 4096, n


@pytest.mark.parametrize('n,sigma', [(2, 0.05), (3, 0.05), (70, 0.05), (1100, 0.02), (5000, 0.05)])
def test_restatement_recovers_the_planted_mount(n, sigma):
    """The restatement against the planted q_true: under 10 x its own sensitivity to the order of summation, with the floor of the
    first-order perturbation bound (16 roundings of |A| over the eigenvalue gap)."""
    m = ref.measured(n, sigma=sigma)
    bound = max(10.0 * m['e_ord'], ref.angle_floor(m['eig']))
    print('%d pairs (sigma %g): restatement vs planted %.3g, forward vs backward %.3g, floor %.3g, eig %s, l1 / l3 = %.3g, largest residual %.3g'
          % (n, sigma, m['e_ref'], m['e_ord'], ref.angle_floor(m['eig']), m['eig'], m['eig'][1] / m['eig'][3], m['res'].max()))
    assert m['bad'] == 0 and m['e_ref'] <= bound
    assert m['res'].max() <= 2.0 * bound                  # consistent data: the residuals (rotation angles) are rounding as well
    assert m['eig'][1] >= 0.05 * m['eig'][3]              # the gap is healthy: rotations about more than one axis
    # the sign of an input is invisible: the same bits without the negated half
    qb = np.where(ref.planted(n, sigma)[0][:, 3:4] < 0, -ref.planted(n, sigma)[0], ref.planted(n, sigma)[0])
    assert np.array_equal(ref.extrinsic_reference(qb, m['qc'])[0], m['q'])
    if n == 1100:                                         # the vectorised restatement of the 70 001 case agrees with the loop
        qv, lv, rv = ref.extrinsic_reference_vec(m['qb'], m['qc'])
        assert ref.qangle(qv, m['q']) <= bound and np.abs(lv - m['eig']).max() <= 1e-9 * m['eig'][3] and np.abs(rv - m['res']).max() <= 2.0 * bound


def test_restatement_one_axis_is_degenerate():
    qb, qc = ref.planted(50, axis=(0.3, -0.5, 0.8))
    _, lam, _, bad = ref.extrinsic_reference(qb, qc)
    print('one axis, 50 pairs: eig %s' % lam)
    assert bad == 0 and (lam[1] - lam[0]) / lam[3] <= 1e-9 and lam[2] > 0.1 * lam[3]


def test_restatement_huber_gain():
    """300 pairs, 2e-4 rad of noise on every body rotation, every tenth corrupted by Exp(N(0, 0.05^2)), delta = 1e-3: four rounds bring
    the restatement at least 10 x closer to the planted mount, and the rounds settle."""
    plain = ref.measured(300, **ref.HUBER)
    e = [plain['e_ref']] + [ref.measured(300, delta=1e-3, rounds=K, **ref.HUBER)['e_ref'] for K in (1, 2, 4)]
    print('restatement vs planted after 0, 1, 2, 4 rounds: %s' % e)
    assert 10.0 * e[3] <= e[0]
    assert ref.measured(300, delta=1e-3, rounds=4, **ref.HUBER)['bad'] == 0


def test_restatement_weights_and_exclusion():
    qb, qc = ref.planted(70)
    w = np.ones(70)
    w[4] = 0.0
    qn = qb.copy()
    qn[4, 0] = np.nan
    clean, dirty = ref.extrinsic_reference(qb, qc, w), ref.extrinsic_reference(qn, qc, w)
    assert clean[3] == 0 and dirty[3] == 0 and np.array_equal(clean[0], dirty[0]) and np.isnan(dirty[2][4]) and np.isfinite(clean[2][4])
    assert ref.extrinsic_reference(qn, qc)[3] == 1 and np.array_equal(ref.extrinsic_reference(qn, qc)[0], clean[0])
    w[5] = -2.0
    assert ref.extrinsic_reference(qb, qc, w)[3] == 1
    none = ref.extrinsic_reference(qb, qc, np.zeros(70))
    assert not none[0].any() and not none[1].any() and not none[2].any()
