"""The reduced-arithmetic Lie formulas of lie_dev.h (tests/lie_f64_fast.py: skew_sq, the vector form of se3_Q, the shared half-angle
se3_exp, Jl^-1 reused from se3_log) on the CPU, no GPU:

(a) against the 50-digit reference of tests/golden/lie_cases.npz: every quantity's worst error within 2 x the floor stored in the file
    (the floor is the matrix forms' own worst error; 2 x is the slack test_lie_golden_cpu.py gives libm, 8 x below the GPU tolerance);
(b) function by function against the matrix forms they replaced (tests/lie_f64.py) on the file's angle sweep with |rho| up to 5:
    within 16 x the OLD form's own float64 error against np.longdouble on the same inputs -- the floor is measured here, from the old
    form and not from the code under test;
(c) mutants of the new forms, each of which must exceed a tolerance of (a)."""
import numpy as np
import pytest

from tests import lie_f64, lie_f64_fast
from tests.golden import make_lie_golden as gen

MUTANTS = {
    'q_u_sign': 'se3_Q: -(u phi^T - phi u^T) for +(u phi^T - phi u^T)',
    'q_c2_c1_swap': 'se3_Q: (c1 - c2) s [phi]x for (c2 - c1) s [phi]x',
    'q_no_2sI': 'se3_Q: the -2 s I of c1 (rho phi^T + phi rho^T - 2 s I) dropped',
    'jl_sin2': 'so3_Jl: c1 = sin^2(th/2) / th^2 for 2 sin^2(th/2) / th^2',
}


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(gen.PATH))


def test_golden_cases_within_twice_the_stored_floor(gold):
    errs = gen.case_errors(gold, lie_f64_fast.transcription_outputs(gold))
    stored = dict(zip(gold['quantities'], gold['floors']))
    assert set(errs) == set(gen.QUANTITIES)
    bad = {}
    for q in gen.QUANTITIES:
        worst = float(errs[q].max())
        print('%-14s worst %.3e  stored floor %.3e' % (q, worst, stored[q]))
        if not worst <= 2.0 * stored[q]:
            bad[q] = (worst, float(stored[q]))
    assert not bad, bad


# ------------------------------------------------------------------ (b) new forms against the old ones
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.fixture(scope='module')
def sweep():
    """Rotation vectors on the file's two angle sweeps about random axes (32 axes per angle) and translations with |rho| in (0, 5],
    every fourth one exactly 5."""
    rng = np.random.default_rng(7)
    ang = np.repeat(np.array(sorted(set(gen.ANGLES) | set(gen.DX_ANGLES))), 32)
    n = len(ang)
    phi = _unit(rng, n) * ang[:, None]
    rho = _unit(rng, n) * np.where(np.arange(n) % 4 == 0, 5.0, rng.uniform(0, 5, n))[:, None]
    return rho, phi


def _ld(x):
    return np.asarray(x, dtype=np.longdouble)


def _skew_ld(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _coef_ld(th2, closed, series, cut):
    """closed form above `cut` (in th^2), Taylor series to the longdouble's rounding below it -- the reference's own choice of branch"""
    big = th2 > cut
    t2 = np.where(big, th2, _ld(1.0))
    return np.where(big, closed(t2, np.sqrt(t2)), series(th2))


def _series(coefs):
    def f(th2):
        acc = _ld(0.0) * th2
        for c in reversed(coefs):
            acc = acc * th2 + c
        return acc
    return f


def _fact(n):
    out = _ld(1.0)
    for i in range(2, n + 1):
        out = out * i
    return out


# longdouble references: the closed forms where they are well conditioned in 64-bit-mantissa arithmetic, 12-term series below 0.5 rad
_A = _series([(-1) ** k / _fact(2 * k + 2) for k in range(12)])                  # (1 - cos t) / t^2
_B = _series([(-1) ** k / _fact(2 * k + 3) for k in range(12)])                  # (t - sin t) / t^3
_C2 = _series([(-1) ** k / _fact(2 * k + 4) for k in range(12)])                 # (t^2 + 2 cos t - 2) / 2 t^4  = sum (-1)^k t^2k / (2k+4)!
_C3 = _series([(-1) ** k * (k + 1) / _fact(2 * k + 5) for k in range(12)])       # (2t - 3 sin t + t cos t) / 2 t^5
_CUT = _ld(0.25)


def _ref_Jl(phi):
    phi = _ld(phi)
    th2 = (phi * phi).sum(-1)
    c1 = _coef_ld(th2, lambda t2, t: (1 - np.cos(t)) / t2, _A, _CUT)
    c2 = _coef_ld(th2, lambda t2, t: (t - np.sin(t)) / (t2 * t), _B, _CUT)
    K = _skew_ld(phi)
    return np.eye(3, dtype=np.longdouble) + c1[..., None, None] * K + c2[..., None, None] * (K @ K)


def _ref_Jl_inv(phi):
    phi = _ld(phi)
    th2 = (phi * phi).sum(-1)
    # (1 - (t/2) cot(t/2)) / t^2 = 1/12 + t^2/720 + t^4/30240 + t^6/1209600 + t^8/47900160 + 691 t^10/1307674368000 + ...
    ser = _series([_ld(1) / 12, _ld(1) / 720, _ld(1) / 30240, _ld(1) / 1209600, _ld(1) / 47900160, _ld(691) / _ld(1307674368000),
                   _ld(1) / _ld(74724249600), _ld(3617) / _ld(10670622842880000)])
    c = _coef_ld(th2, lambda t2, t: (1 - t * np.cos(t / 2) / (2 * np.sin(t / 2))) / t2, ser, _ld(0.01))
    K = _skew_ld(phi)
    return np.eye(3, dtype=np.longdouble) - K / 2 + c[..., None, None] * (K @ K)


def _ref_Q(rho, phi):
    rho, phi = _ld(rho), _ld(phi)
    th2 = (phi * phi).sum(-1)
    c1 = _coef_ld(th2, lambda t2, t: (t - np.sin(t)) / (t2 * t), _B, _CUT)
    c2 = _coef_ld(th2, lambda t2, t: (t2 + 2 * np.cos(t) - 2) / (2 * t2 * t2), _C2, _CUT)
    c3 = _coef_ld(th2, lambda t2, t: (2 * t - 3 * np.sin(t) + t * np.cos(t)) / (2 * t2 * t2 * t), _C3, _CUT)
    Tm, P = _skew_ld(rho), _skew_ld(phi)
    PT, TP = P @ Tm, Tm @ P
    PTP = PT @ P
    b = lambda c: c[..., None, None]
    return Tm / 2 + b(c1) * (PT + TP + PTP) + b(c2) * (P @ PT + TP @ P - 3 * PTP) + b(c3) * (PTP @ P + P @ PTP)


def _ref_exp(rho, phi):
    phi = _ld(phi)
    th = np.sqrt((phi * phi).sum(-1))
    half = _coef_ld(th * th, lambda t2, t: np.sin(t / 2) / t, _series([(-1) ** k / (_fact(2 * k + 1) * _ld(2) ** (2 * k + 1)) for k in range(12)]), _CUT)
    t = (_ref_Jl(phi) @ _ld(rho)[..., None])[..., 0]
    return np.concatenate([t, phi * half[..., None], np.cos(th / 2)[..., None]], -1)


def _err(x, ref):
    """per case: max|x - ref| / max(1, max|ref|) -- case_errors' measure"""
    x, ref = _ld(x).reshape(len(ref), -1), _ld(ref).reshape(len(ref), -1)
    return (np.abs(x - ref).max(1) / np.maximum(1.0, np.abs(ref).max(1))).astype(np.float64)


@pytest.mark.skipif(np.finfo(np.longdouble).eps > 2e-19, reason='np.longdouble is no wider than float64 here')
@pytest.mark.parametrize('name', ['se3_Q', 'so3_Jl', 'so3_Jl_inv', 'se3_exp'])
def test_new_form_within_16_floors_of_the_old_form(sweep, name):
    rho, phi = sweep
    args, ref = {'se3_Q': ((rho, phi), _ref_Q(rho, phi)), 'so3_Jl': ((phi,), _ref_Jl(phi)), 'so3_Jl_inv': ((phi,), _ref_Jl_inv(phi)),
                 'se3_exp': ((rho, phi), _ref_exp(rho, phi))}[name]
    old, new = getattr(lie_f64, name)(*args), getattr(lie_f64_fast, name)(*args)
    floor = float(_err(old, ref).max())              # the old form's own float64 error on these inputs
    e_new, diff = float(_err(new, ref).max()), float(_err(new, old).max())
    print('%-10s floor (old vs longdouble) %.3e  new vs longdouble %.3e  new vs old %.3e' % (name, floor, e_new, diff))
    assert 0.0 < floor < 1e-13, floor                # the reference resolves the old form's rounding, and nothing coarser
    assert e_new <= 16.0 * floor, (e_new, floor)
    assert diff <= 16.0 * floor, (diff, floor)


def test_vector_form_of_q_is_the_matrix_form_on_normal_inputs():
    """the identities themselves, on N(0,1) inputs: a few ulps of the entries' size"""
    rng = np.random.default_rng(3)
    rho, phi = rng.normal(size=(4096, 3)), rng.normal(size=(4096, 3))
    d = np.abs(lie_f64_fast.se3_Q(rho, phi) - lie_f64.se3_Q(rho, phi)).max()
    print('max |Q_vector - Q_matrix| = %.2e' % d)
    assert d <= 8 * np.finfo(np.float64).eps * 4.0      # |Q| entries reach ~|rho| = 4 here


# ------------------------------------------------------------------ (c) mutants
@pytest.mark.parametrize('name', lie_f64_fast.MUTANTS)
def test_mutant_is_seen(gold, name):
    assert name in MUTANTS
    stored = dict(zip(gold['quantities'], gold['floors']))
    with lie_f64_fast.mutant(name):
        errs = gen.case_errors(gold, lie_f64_fast.transcription_outputs(gold))
    over = {q: float(errs[q].max() / (2.0 * stored[q])) for q in gen.QUANTITIES if errs[q].max() > 2.0 * stored[q]}
    print(name, MUTANTS[name], {q: '%.1e x bound' % v for q, v in over.items()})
    assert over, '%s (%s) passes every bound of (a)' % (name, MUTANTS[name])
