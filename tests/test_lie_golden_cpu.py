"""What tests/golden/lie_cases.npz is worth (no GPU): the rounding floor of the lie_dev.h formulas in float64, the tolerance of
tests/test_lie_gpu.py derived from it, a mutation check of that tolerance, and the staleness of the committed references.

The reference (tests/golden/make_lie_golden.py) is 60-digit mp arithmetic that uses none of the closed-form coefficients.  The floor of
a quantity is the largest error, over the cases, of tests/lie_f64.py -- the kernels' formulas in NumPy float64 -- against it, with the
error of a case = max|x - ref| / max(1, max|ref|).  The GPU tolerance is 16 floors: device sincos / atan / sqrt differ from libm by an ulp
or two and hipcc contracts multiply-adds; carried through a handful of chained products that is one order of magnitude, no more.
Every tolerance has to come out at or below 1e-11, or the second term of the so3_Jl_inv series (1.4e-11 just below 1e-2 rad) could
hide under it."""
import numpy as np
import pytest

from tests import lie_f64
from tests.golden import make_lie_golden as gen

# what each mutant of tests/lie_f64.py is
MUTANTS = {
    'exp_imag_t2': 'so3_exp series, imaginary part: -th^2/48 dropped',
    'exp_real_t2': 'so3_exp series, real part: -th^2/8 dropped',
    'log_t2': 'so3_log series: -x^2/3 dropped',
    'jlinv_t2': 'so3_Jl_inv series: +th^2/720 dropped',
    'jl_c1_t2': 'so3_Jl series, c1: -th^2/24 dropped',
    'jl_c2_t2': 'so3_Jl series, c2: -th^2/120 dropped',
    'q_c1_t2': 'se3_Q series, c1: -th^2/120 dropped',
    'q_c2_t2': 'se3_Q series, c2: -th^2/720 dropped',
    'q_c3_t2': 'se3_Q series, c3: -th^2/2520 dropped',
    'q_swap_c1_c2': 'se3_Q closed forms: c1 and c2 exchanged',
    'q_swap_c2_c3': 'se3_Q closed forms: c2 and c3 exchanged',
    'log_atan2': 'so3_log: atan2(vn, w) for atan(vn / w) (leaves the principal value when w < 0)',
    'jlinv_half_sign': 'so3_Jl_inv: +K/2 for -K/2',
}
# Mutants below float64 resolution on this case set, with the bound that shows it: {name: (quantity, bound on its effect)}.  None: with
# se3_Q's series reaching up to 0.1 rad, even the second term of c3 is worth th^2/2520 * 2 th^3 |rho| = 4e-8 at th = 0.1, |rho| = 5.
INERT = {}


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(gen.PATH))


@pytest.fixture(scope='module')
def tol(gold):
    return dict(zip(gold['quantities'], gold['tolerances']))


def test_case_set(gold):
    z = gold
    M = len(z['poses'])
    assert 200 <= M <= 300 and M % 64 != 0 and M + len(z['edges']) <= 400
    assert set(z['vo_angle']) == set(gen.ANGLES) == set(z['imu_angle'])
    assert np.abs(z['nodes'][:, :3]).max() <= 10 and np.abs(z['vels']).max() <= 5 and 0.05 <= z['dts'].min() and z['dts'].max() <= 0.2
    # the residuals are what they were chosen to be: angles on the sweep (VO and IMU independently), translations up to 5 m
    L = z['lin_ref']
    np.testing.assert_allclose(np.linalg.norm(L[3:6], axis=0), z['vo_angle'], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(L[24:27], axis=0), z['imu_angle'], rtol=1e-9, atol=1e-15)
    assert 4.99 < np.linalg.norm(L[0:3], axis=0).max() < 5.01 and (z['vo_angle'] != z['imu_angle']).mean() > 0.8
    # double cover: a third of the links compose to w < 0, small angles (w ~ -1, the series branch of so3_log) among them
    qe = lie_f64.qmul(lie_f64.qmul(lie_f64.qinv(z['poses'][:, 3:]), lie_f64.qinv(z['nodes'][:-1, 3:])), z['nodes'][1:, 3:])
    neg = qe[:, 3] < 0
    assert 0.3 < neg.mean() < 0.37 and (neg & (z['vo_angle'] < 2e-3) & (z['vo_angle'] > 0)).any() and (neg & (z['vo_angle'] > 3)).any()
    e = z['edges']
    assert (e[:, 0] > e[:, 1]).any() and (e[:, 1] == e[:, 0] + 1).any() and (np.abs(e[:, 0] - e[:, 1]) >= 40).any()
    assert set(np.round(np.linalg.norm(z['dx'][:, 3:6], axis=1), 12)) == set(np.round(gen.DX_ANGLES, 12))


def test_floors_and_tolerances(gold, tol):
    errs = gen.case_errors(gold, gen.transcription_outputs(gold))
    stored = dict(zip(gold['quantities'], gold['floors']))
    assert tuple(gold['quantities']) == gen.QUANTITIES
    for q in gen.QUANTITIES:
        floor = errs[q].max()
        print('%-14s floor %.3e (stored %.3e)  tolerance %.3e' % (q, floor, stored[q], tol[q]))
        assert tol[q] == 16.0 * stored[q] and tol[q] <= 1e-11, q
        # measured here against measured when the file was written: the same up to libm's last bit
        assert floor <= 2.0 * stored[q] and stored[q] <= 2.0 * floor, (q, floor, stored[q])


@pytest.mark.parametrize('name', lie_f64.MUTANTS)
def test_mutant_is_seen(gold, tol, name):
    assert name in MUTANTS
    with lie_f64.mutant(name):
        errs = gen.case_errors(gold, gen.transcription_outputs(gold))
    over = {q: float(errs[q].max() / tol[q]) for q in gen.QUANTITIES if errs[q].max() > tol[q]}
    print(name, MUTANTS[name], {q: '%.1e x tolerance' % v for q, v in over.items()})
    if name in INERT:
        q, bound = INERT[name]
        assert not over and bound < tol[q], 'no longer inert: take it off the list'
    else:
        assert over, '%s (%s) passes every tolerance' % (name, MUTANTS[name])


def test_committed_references_reproduce(gold):
    """A fixed subset of every family, recomputed with mpmath: bit for bit what the file holds."""
    pytest.importorskip('mpmath')
    z = gold
    M, N, E = len(z['poses']), len(z['nodes']), len(z['edges'])
    n = 0
    for k in range(0, M, 13):                                  # 16 links: every angle of the sweep
        col, _ = gen.ref_link(z, k)
        assert np.array_equal(gen._out(col), z['lin_ref'][:, k]), k
        n += 1
    for k in range(5, M, 50):
        assert np.array_equal(gen._out(gen.ref_trial_link(z, k)), z['trial_link_ref'][k]), k
        n += 1
    for e in range(0, E, 6):
        rec, loss, g = gen.ref_edge(z, e)
        assert np.array_equal(gen._out(rec), z['edge_lin_ref'][:, e]) and np.array_equal(gen._out(loss), z['vo_loss_ref'][e])
        assert np.array_equal(gen._out(g), z['vo_grad_ref'][e]), e
        n += 1
    for i in range(0, N, 29):                                  # 7 nodes: every rotation of the retraction sweep
        assert np.array_equal(gen._out(gen.ref_retract(z, i, 1)), z['retract_pos_ref'][i]), i
        n += 1
    for i in range(3, gen.N_PARTIAL, 17):
        assert np.array_equal(gen._out(gen.ref_retract(z, i, -1)), z['retract_neg_ref'][i]), i
        assert np.array_equal(gen._out(gen.ref_align(z, i)), z['align_ref'][i]), i
        n += 2
    assert n >= 32
