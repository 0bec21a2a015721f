"""The IMU derivative kernels over the full range of per-sample rotation angles, against the 60-digit reference in
tests/golden/imu_cases.npz (tests/golden/make_imu_golden.py): angles |gyro| dt from 0 across every series / closed-form switch to 6 rad
about general axes, single-sample frames that lay every coefficient bare, ragged and empty frames around the 64-frame scan block,
float64 and float32 inputs, 260 frames through the 256 lanes of the backward, 300 rows through the 256 of the gyro-bias solve with a
third of the trusted rotations negated.  The error measures are those of the kernels' older GPU tests (make_imu_golden.errors); the
tolerance per quantity is stored in the file: 16 x the rounding floor of the same formulas in NumPy float64, measured and
mutation-checked by tests/test_imu_golden_cpu.py (1.6e-15 .. 1.9e-13 for float64 outputs).  The forward has a harder contract: bit
for bit the plain-C restatement.  Every call is made twice: the same bits.  All inputs come from the file; every test is a few small
launches."""
import numpy as np
import pytest
import torch

from tests.golden import make_imu_golden as gen

pytestmark = pytest.mark.gpu
TORCH = {'f64': torch.float64, 'f32': torch.float32}
MODES = [(True, 'motion'), (False, 'world')]


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(gen.PATH))


def _t(a, cuda, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=cuda)


def _stream(z, cuda, s, name='f64'):
    seg = np.ascontiguousarray(z[s + '_seg'], dtype=np.int64)
    return (_t(z[s + '_dt'], cuda, TORCH[name]), _t(z[s + '_gyro'], cuda, TORCH[name]), _t(z[s + '_acc'], cuda, TORCH[name]),
            torch.tensor(seg, device=cuda), seg)


def _check(z, out, names):
    errs = gen.errors(z, out)
    tol = dict(zip(z['quantities'], z['tolerances']))
    bad = {}
    for q in names:
        print('%-16s error %.3e  tolerance %.3e' % (q, errs[q], tol[q]))
        if not errs[q] <= tol[q]:
            bad[q] = (errs[q], float(tol[q]))
    assert not bad, bad


@pytest.mark.parametrize('name', list(gen.DTYPES))
@pytest.mark.parametrize('motion,mode', MODES)
def test_covariance(cuda, gold, name, motion, mode):
    from islam_amd import ops
    a = _stream(gold, cuda, 'a', name)
    ic = None if motion else _t(gold['init_cov'], cuda)
    out = ops.imu_preint_cov(*a, gen.GYRO_COV, gen.ACC_COV, motion, ic)
    assert torch.equal(out, ops.imu_preint_cov(*a, gen.GYRO_COV, gen.ACC_COV, motion, ic))
    out = out.cpu().numpy()
    assert np.array_equal(out, np.swapaxes(out, -1, -2))
    _check(gold, {'cov_%s_%s' % (mode, name): out}, ('cov_' + mode,) + (('cov_single',) if motion else ()))


@pytest.mark.parametrize('name', list(gen.DTYPES))
@pytest.mark.parametrize('motion,mode', MODES)
def test_bias_jacobians(cuda, gold, name, motion, mode):
    """World rows start from an init_jac whose (dphi, b_a) block is not zero: it has to be dropped."""
    from islam_amd import ops
    a = _stream(gold, cuda, 'a', name)
    ij = None if motion else _t(gold['init_jac'], cuda)
    out = ops.imu_preint_bias_jac(*a, motion, ij)
    assert torch.equal(out, ops.imu_preint_bias_jac(*a, motion, ij))
    out = out.cpu().numpy()
    assert not out[:, 0:3, 3:6].any()
    _check(gold, {'jac_%s_%s' % (mode, name): out}, ('jac_' + mode,) + (('jac_single',) if motion else ()))


@pytest.mark.parametrize('name', list(gen.DTYPES))
@pytest.mark.parametrize('motion,mode', MODES)
def test_forward_is_the_restatement_bit_for_bit(cuda, gold, name, motion, mode):
    """islam_imu_preint == oracle.cwrap.imu_integrate on stream A (the sincos argument reduction is crossed at pi/2 (1 -+ 1e-3)); its
    distance to the mp integrator is printed: it is that of the restatement, which tests/test_imu_golden_cpu.py records."""
    from islam_amd import ops
    from oracle import cwrap
    dt = TORCH[name]
    a = _stream(gold, cuda, 'a', name)
    init = (_t(gen.INIT_POS, cuda, dt), _t(gen.INIT_ROT, cuda, dt), _t(gen.INIT_VEL, cuda, dt))
    got = ops.imu_preint(*a, *init, gen.GRAVITY, motion)
    again = ops.imu_preint(*a, *init, gen.GRAVITY, motion)
    want = cwrap.imu_integrate(gold['a_dt'], gold['a_gyro'], gold['a_acc'], gold['a_seg'], gen.INIT_POS, gen.INIT_ROT, gen.INIT_VEL, gen.GRAVITY,
                               motion, gen.DTYPES[name])
    out = {}
    for k, g, g2, w in zip(('pos', 'rot', 'vel'), got, again, want):
        assert g.dtype == dt and torch.equal(g, g2)
        assert np.array_equal(g.cpu().numpy(), w), k
        out['fwd_%s_%s_%s' % (k, mode, name)] = g.double().cpu().numpy()
    for q, e in gen.errors(gold, out).items():
        print('%-24s distance to the mp integrator %.3e' % (q, e))


def _backward(z, cuda, s, motion, gravity, cot):
    from islam_amd import ops
    dt, gyro, acc, segt, seg = _stream(z, cuda, s)
    gyro, acc = gyro.requires_grad_(True), acc.requires_grad_(True)
    init = (_t(gen.INIT_POS, cuda), _t(gen.INIT_ROT, cuda), _t(gen.INIT_VEL, cuda))
    pos, rot, vel = ops.imu_preint(dt, gyro, acc, segt, seg, *init, gravity, motion)
    go = tuple(_t(c, cuda) for c in cot)
    g = torch.autograd.grad((pos, rot, vel), (gyro, acc), grad_outputs=go, retain_graph=True)
    g2 = torch.autograd.grad((pos, rot, vel), (gyro, acc), grad_outputs=go)
    assert torch.equal(g[0], g2[0]) and torch.equal(g[1], g2[1])
    return g[0].cpu().numpy(), g[1].cpu().numpy()


@pytest.mark.parametrize('motion,mode', MODES)
def test_backward(cuda, gold, motion, mode):
    """Stream B through autograd: random cotangents on pos, vel and rot (left tangent [wr, 0]), against central differences of the mp
    integrator."""
    gg, ga = _backward(gold, cuda, 'b', motion, gen.GRAVITY, gen.bwd_cotangents(gold, motion))
    assert np.abs(gg).max(1).min() > 0                          # (every sample belongs to a frame: no row is left at zero)
    _check(gold, {'bwd_gyro_' + mode: gg, 'bwd_acc_' + mode: ga}, ('bwd_gyro_' + mode, 'bwd_acc_' + mode))


def test_backward_of_single_samples(cuda, gold):
    """Stream C: one sample per angle, no gravity, a rotation cotangent alone: g_gyro = d Jl(w d)^T wr, JlT with nothing around it."""
    na = len(gen.ANGLES)
    cot = (np.zeros((na, 3)), np.concatenate([gold['c_wr'], np.zeros((na, 1))], 1), np.zeros((na, 3)))
    gg, ga = _backward(gold, cuda, 'c', True, 0.0, cot)
    assert not ga.any()
    _check(gold, {'bwd_gyro_single': gg}, ('bwd_gyro_single',))


@pytest.mark.parametrize('name', list(gen.DTYPES))
def test_bias_correct(cuda, gold, name):
    """One call per angle of BC_ANGLES = |J_phig dbg| of the call's own row, 0 .. 3 rad across the switch of the kernel's Exp."""
    from islam_amd import ops
    z, n, dt = gold, gen.BC_ROWS, TORCH[name]
    jac = _t(z['jac_motion_f64_ref'][:n], cuda)
    inc = [_t(z['fwd_%s_motion_f64_ref' % k][:n], cuda, dt) for k in ('rot', 'vel', 'pos')]
    calls = []
    for k in range(len(gen.BC_ANGLES)):
        got = ops.imu_bias_correct(jac, *inc, z['bc_dbg'][k], z['bc_dba'][k])
        again = ops.imu_bias_correct(jac, *inc, z['bc_dbg'][k], z['bc_dba'][k])
        assert all(g.dtype == dt and torch.equal(g, g2) for g, g2 in zip(got, again))
        calls.append([g.double().cpu().numpy() for g in got])
    out = {'bc_%s_%s' % (key, name): np.stack([c[i] for c in calls]) for i, key in enumerate(('rot', 'vel', 'pos'))}
    _check(z, out, tuple('bc_%s_%s' % (key, name) for key in ('rot', 'vel', 'pos')) + (('bc_rot_small_f64',) if name == 'f64' else ()))


def test_gyro_bias_solve(cuda, gold):
    """300 rows (a second, partial pass of the 256 lanes), residual angles 0 .. pi - 1e-6 across the vn > 1e-8 qw switch, a third of
    rot_ref negated (the qw < 0 flip), weights with zeros: x and H against the normal equations solved in mp."""
    from islam_amd import ops
    z = gold
    a = (_t(gen.solve_jac(z), cuda), _t(z['s_rot_imu'], cuda), _t(z['s_rot_ref'], cuda), _t(z['s_weight'], cuda))
    x, H, bad = ops.imu_gyro_bias_solve(*a)
    x2, H2, bad2 = ops.imu_gyro_bias_solve(*a)
    assert bad == 0 and bad2 == 0 and torch.equal(x, x2) and torch.equal(H, H2)
    H = H.cpu().numpy()
    assert np.array_equal(H, H.T)
    _check(z, dict(solve_x=x.cpu().numpy(), solve_H=H), ('solve_x', 'solve_H'))
