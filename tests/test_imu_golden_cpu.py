"""What tests/golden/imu_cases.npz is worth (no GPU): that its streams hold the angles they were built for, the rounding floor of the
IMU derivative kernels' formulas in float64, the tolerances of tests/test_imu_golden_gpu.py derived from it, a mutation check of
those tolerances, the accuracy of the forward's bit-exact restatement at large angles, and the staleness of the committed references.

The reference (tests/golden/make_imu_golden.py) is 60-digit mp arithmetic that uses none of the closed-form coefficients.  The floor of
a quantity is the error of tests/imu_f64.py -- the kernels' formulas in NumPy float64, folded one sample after the other -- against
it, in the measure of the kernel's own GPU test.  The GPU tolerance is 16 floors, the rule of tests/test_lie_golden_cpu.py: device
sincos / atan2 / sqrt differ from libm by an ulp or two, hipcc contracts multiply-adds, and the kernels join the same elements in
another association order (lane chunks, scan trees); carried through a handful of chained products that is one order of magnitude.
Every float64 tolerance comes out at or below 2e-13, against 1e-9 and 1e-10 in the older tests of the same kernels.

With c1 = (1 - cos th) / th^2 in JlT (imu_preint.hip before this file existed; mutant jlt_c1_one_minus_cos) the floor of the gyro
gradient was 2.3e-13 / 1.9e-13 (motion / world rows of stream B) and 1.2e-13 on stream C, against 7.5e-15 / 5.1e-15 and 1.0e-16 with
the half-angle form."""
import numpy as np
import pytest

from tests import imu_f64
from tests.golden import make_imu_golden as gen

# what each mutant of tests/imu_f64.py is
MUTANTS = {
    'A_t2': 'sample_element / sample_rot series, A = sin th / th: -th^2/6 dropped',
    'B_t2': 'sample_element / sample_rot series, B = (1 - cos th) / th^2: -th^2/24 dropped',
    'C_t2': 'sample_element / sample_rot series, C = (th - sin th) / th^3: -th^2/120 dropped',
    'jr_jl': 'Jr -> Jl: +B K for -B K',
    'jlt_c1_t2': 'JlT series, c1: -th^2/24 dropped',
    'jlt_c2_t2': 'JlT series, c2: -th^2/120 dropped',
    'jlt_swap_c1_c2': 'JlT: c1 and c2 exchanged',
    'jlt_c1_one_minus_cos': 'JlT closed form, c1 = (1 - cos th) / th^2 for 2 sin^2(th/2) / th^2 (what the kernel used to do)',
    'bc_im_t2': "bias_correct_kernel's Exp series, imaginary part: -th^2/48 dropped",
    'bc_re_t2': "bias_correct_kernel's Exp series, real part: -th^2/8 dropped",
    'log_atan': 'gyro_bias_solve_kernel: atan(vn / qw) for atan2(vn, qw) and no flip to qw >= 0 (0 / 0 on an unchanged, negated row)',
    'log_no_flip': 'gyro_bias_solve_kernel: no flip to qw >= 0 (the rotation the long way round)',
    'init_jac_block': 'the (dphi, b_a) block of init_jac carried along',
}
# Mutants below float64 resolution on this case set, with the bound that shows it: {name: (quantity, bound on its effect)}.
# jlt_c2_t2: the series runs for th <= 1e-4 and c2 multiplies w x (w x u), so the dropped term moves Jl^T u by at most
# th^4 / 120 |u| = 8.4e-19 |u|: a hundredth of an ulp.
INERT = {'jlt_c2_t2': ('bwd_gyro_single', 1e-16 / 120.0)}
ULP = 2.220446049250313e-16


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(gen.PATH))


@pytest.fixture(scope='module')
def tol(gold):
    return dict(zip(gold['quantities'], gold['tolerances']))


def _angles(dt, gyro, dtype=np.float64):
    return np.linalg.norm(np.asarray(gyro, dtype).astype(np.float64), axis=1) * np.asarray(dt, dtype).astype(np.float64)


def _same_side(a, b):
    """both sets of angles on the same side of every switch: 1e-4 (JlT, bias_correct), 1e-3 (covariance, bias Jacobians), pi/2 (the
    forward's half angle against pi/4)"""
    return all(np.array_equal(a > s, b > s) for s in (2.220446049250313e-16, 1e-4, 1e-3, gen.PI / 2))


def test_case_set(gold):
    z = gold
    A, na = np.array(gen.ANGLES), len(gen.ANGLES)
    assert {0.0, 1e-12, 1e-8, 3e-5, 1.5e-4, 2e-4, 1e-2, 0.1, 0.6, 1.0, 2.0, 3.0, gen.PI - 1e-6, 4.0, 6.0} <= set(gen.ANGLES)
    for s in (1e-4, 1e-3, gen.PI / 2):
        assert s * (1 - 1e-3) in gen.ANGLES and s * (1 + 1e-3) in gen.ANGLES
    # stream A
    seg, dt = z['a_seg'], z['a_dt']
    counts = np.diff(seg)
    S = len(dt)
    assert len(counts) == gen.A_FRAMES == 110 and S == seg[-1] <= 700 and set(counts) == set(gen.COUNTS)
    assert np.all(counts[:na] == 1) and counts[63] == 0 and counts[64] == 0 and counts[-1] == 0 and counts[62] > 0 and counts[65] > 0
    want = A[[s if s < na else (s - na) % na for s in range(S)]]
    th = _angles(dt, z['a_gyro'])
    np.testing.assert_allclose(th, want, rtol=1e-12, atol=0)
    th32 = _angles(dt, z['a_gyro'], np.float32)
    np.testing.assert_allclose(th32, want, rtol=1e-6, atol=0)
    assert _same_side(th, want) and _same_side(th32, want)
    for i in np.nonzero(counts >= 64)[0]:                          # the long frames hold every angle
        assert set(want[seg[i]:seg[i + 1]]) == set(gen.ANGLES)
    assert 0.004 <= dt.min() and dt.max() <= 0.012 and 8.0 < np.linalg.norm(z['a_acc'], axis=1).mean() < 12.0
    assert np.abs(z['init_jac'][0:3, 3:6]).min() > 0 and np.linalg.eigvalsh(0.5 * (z['init_cov'] + z['init_cov'].T)).min() > 0
    assert z['cov_world_f64_ref'].shape == (111, 45) and z['jac_motion_f32_ref'].shape == (110, 9, 6)
    # stream B: more frames than the backward kernel has lanes
    seg = z['b_seg']
    counts = np.diff(seg)
    assert len(counts) == gen.B_FRAMES > 256 and sorted(set(counts)) == [0, 1, 2, gen.B_LONG] and (counts == gen.B_LONG).sum() == 1
    assert counts[255] > 0 and counts[256] > 0 and (counts == 0).sum() > 50
    th = _angles(z['b_dt'], z['b_gyro'])
    want = A[[(s + 3) % na for s in range(len(th))]]
    np.testing.assert_allclose(th, want, rtol=1e-12, atol=0)
    assert _same_side(th, want)
    assert z['b_wr_world'].shape == (gen.B_FRAMES + 1, 3) and z['b_wp_motion'].shape == (gen.B_FRAMES, 3)
    # stream C: one sample per angle
    np.testing.assert_allclose(_angles(z['c_dt'], z['c_gyro']), A, rtol=1e-12, atol=0)
    assert _same_side(_angles(z['c_dt'], z['c_gyro']), A) and np.array_equal(z['c_seg'], np.arange(na + 1))
    # bias correction: call k turns row k by BC_ANGLES[k]
    J = z['jac_motion_f64_ref'][:gen.BC_ROWS]
    got = np.array([np.linalg.norm(J[k, 0:3, 0:3] @ z['bc_dbg'][k]) for k in range(len(gen.BC_ANGLES))])
    np.testing.assert_allclose(got, gen.BC_ANGLES, rtol=1e-9, atol=0)
    assert np.array_equal(got > 1e-4, np.array(gen.BC_ANGLES) > 1e-4) and {0.0, 1e-12, 1e-8, 1e-2, 1.0, 3.0} <= set(gen.BC_ANGLES)
    assert max(gen.BC_ANGLES[:gen.BC_SMALL]) == 1e-2 and 1e-4 * (1 - 1e-3) in gen.BC_ANGLES and 1e-4 * (1 + 1e-3) in gen.BC_ANGLES
    # gyro-bias solve: a second, partial pass of 256 rows; the residual angles; a third of the rows negated
    n = len(z['s_rot_imu'])
    assert n == gen.SOLVE_ROWS and 256 < n < 512
    assert {0.0, 1e-12, 2e-8 * (1 - 1e-2), 2e-8 * (1 + 1e-2), 1e-3, 1.0, 3.0, gen.PI - 1e-6} == set(gen.SOLVE_ANGLES) == set(z['s_angle'])
    assert np.abs(z['s_angle_ref'] - z['s_angle']).max() <= 1e-15
    q = imu_f64.qmul(imu_f64.conj(z['s_rot_imu']), z['s_rot_ref'])
    neg = q[:, 3] < 0
    assert np.array_equal(neg, z['s_negated']) and 0.3 < neg.mean() < 0.37
    for a in gen.SOLVE_ANGLES:                                     # every angle with w < 0 and with w > 0, the small ones among them
        assert (neg & (z['s_angle'] == a)).any() and (~neg & (z['s_angle'] == a)).any()
    qa = np.where(neg[:, None], -q, q)
    series = ~(np.linalg.norm(qa[:, :3], axis=1) > 1e-8 * qa[:, 3])
    assert np.array_equal(series, z['s_angle'] < 2e-8)             # 2e-8 (1 - 1e-2) takes the series branch, 2e-8 (1 + 1e-2) does not
    w = z['s_weight']
    assert 10 <= (w == 0).sum() <= 60 and w[w != 0].min() >= 0.2 and (w[256:] != 0).any()
    assert np.abs(gen.solve_jac(z)[:, 0:3, 0:3]).max(axis=(1, 2)).min() > 0


def test_floors_and_tolerances(gold, tol):
    errs = gen.errors(gold, gen.transcription_outputs(gold))
    stored = dict(zip(gold['quantities'], gold['floors']))
    assert tuple(gold['quantities']) == gen.QUANTITIES
    for q in gen.QUANTITIES:
        floor = errs[q]
        print('%-16s floor %.3e (stored %.3e)  tolerance %.3e' % (q, floor, stored[q], tol[q]))
        assert tol[q] == 16.0 * stored[q] and tol[q] <= (1e-6 if q.endswith('f32') else 2e-13), q
        # measured here against measured when the file was written: the same up to libm's last bit (a floor of one ulp can only move by
        # whole ulps: one of them is allowed on top)
        assert floor <= 2.0 * stored[q] + ULP and stored[q] <= 2.0 * floor + ULP, (q, floor, stored[q])
    # float32 I/O of the correction: the floor is the rounding of the outputs to float32, half an ulp of increments of size <= 1
    assert all(stored[q] < 6e-8 for q in gen.QUANTITIES if q.endswith('f32'))


def test_forward_restatement_accuracy(gold):
    """oracle.cwrap.imu_integrate -- what islam_imu_preint equals bit for bit -- against the mp integrator on stream A: the accuracy of
    the forward at per-sample angles up to 6 rad, per output and input type.  Measured and recorded, the contract is the bit-equality;
    1e-12 and 1e-4 only say that float64 and float32 do what their precision allows over 625 samples."""
    errs = gen.errors(gold, gen.forward_outputs(gold))
    stored = dict(zip(gold['forward_names'], gold['forward_errors']))
    assert tuple(gold['forward_names']) == gen.FORWARD
    for q in gen.FORWARD:
        print('%-24s error %.3e (stored %.3e)' % (q, errs[q], stored[q]))
        assert errs[q] <= 2.0 * stored[q] and stored[q] <= 2.0 * errs[q], q
        assert stored[q] <= (1e-4 if q.endswith('f32') else 1e-12), q


@pytest.mark.parametrize('name', imu_f64.MUTANTS)
def test_mutant_is_seen(gold, tol, name):
    assert name in MUTANTS
    with imu_f64.mutant(name):
        errs = gen.errors(gold, gen.transcription_outputs(gold))
    over = {q: float(errs[q] / tol[q]) for q in gen.QUANTITIES if not errs[q] <= tol[q]}
    print(name, MUTANTS[name], {q: '%.1e x tolerance' % v for q, v in over.items()})
    if name in INERT:
        q, bound = INERT[name]
        assert not over and bound < min(ULP / 2, tol[q]), 'no longer inert: take it off the list'
    else:
        assert over, '%s (%s) passes every tolerance' % (name, MUTANTS[name])


def test_committed_references_reproduce(gold):
    """A fixed subset of every family, recomputed with mpmath: bit for bit what the file holds."""
    pytest.importorskip('mpmath')
    z = gold
    n = 0
    for name in gen.DTYPES:
        st = gen.stream_a(z, name, frames=24)
        parts = {j: gen.sample_parts(st.dt[j], st.gyro[j]) for j in range(st.seg[24])}
        for i in list(range(0, 21, 4)) + [21, 22, 23]:             # single samples across the sweep, and the first ragged frames
            cov, jac = gen.ref_cov_jac(parts, st.dt, st.acc, st.seg[i:i + 2], 1, True)
            assert np.array_equal(cov[0], z['cov_motion_%s_ref' % name][i]) and np.array_equal(jac[0], z['jac_motion_%s_ref' % name][i]), i
            n += 1
        cov, jac = gen.ref_cov_jac(parts, st.dt, st.acc, st.seg, 4, False, z['init_cov'], z['init_jac'])
        assert np.array_equal(cov, z['cov_world_%s_ref' % name][:5]) and np.array_equal(jac, z['jac_world_%s_ref' % name][:5])
        for motion, mode in ((True, 'motion'), (False, 'world')):
            for k, a in zip(('pos', 'rot', 'vel'), st.forward(motion)):
                assert np.array_equal(a, z['fwd_%s_%s_%s_ref' % (k, mode, name)][:len(a)]), (k, mode, name)
        n += 3
        for k in range(len(gen.BC_ANGLES)):
            inc = [np.asarray(z['fwd_%s_motion_f64_ref' % c][k], dtype=gen.DTYPES[name]).astype(np.float64) for c in ('rot', 'vel', 'pos')]
            out = gen.ref_bias_correct(gen._mat(z['jac_motion_f64_ref'][k]), *[gen._f(a) for a in inc], gen._f(z['bc_dbg'][k]), gen._f(z['bc_dba'][k]))
            for c, a in zip(('rot', 'vel', 'pos'), out):
                assert np.array_equal(gen._out(a), z['bc_%s_%s_ref' % (c, name)][k, k]), (c, name, k)
            n += 1
    x, H, ang = gen.ref_solve(gen.solve_jac(z), z['s_rot_imu'], z['s_rot_ref'], z['s_weight'])
    assert np.array_equal(x, z['solve_x_ref']) and np.array_equal(H, z['solve_H_ref']) and np.array_equal(ang, z['s_angle_ref'])
    for s in (0, 5, 10, 20):
        assert np.array_equal(gen.ref_single(z, s), z['bwd_gyro_single_ref'][s]), s
        n += 1
    st, cot = gen.Stream(z['b_dt'], z['b_gyro'], z['b_acc'], z['b_seg'], gen.GRAVITY), gen.cotangents(z)
    for s in (0, int(z['b_seg'][100]) + 35, len(z['b_dt']) - 1):    # the first sample, one inside the long frame, the last one
        for motion, mode in ((True, 'motion'), (False, 'world')):
            g = gen._out(st.grad(motion, s, cot[motion]))
            assert np.array_equal(g[:3], z['bwd_gyro_%s_ref' % mode][s]) and np.array_equal(g[3:], z['bwd_acc_%s_ref' % mode][s]), (s, mode)
            n += 1
    assert n >= 36
