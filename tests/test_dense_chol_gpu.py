"""GPU tests of the dense fp64 Cholesky (islam_dense_chol_factor / islam_dense_chol_solve, csrc/dense_chol.hip, DESIGN.md section
3.17) through the C ABI, and of the LM that uses it (run_pvgo(general_solver='dense_hip')).

Error bounds (N. J. Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.), u = 2^-53, gamma_k = k u / (1 - k u):
  Theorem 10.3   |A - L L^T| <= gamma_{n+1} |L| |L^T| componentwise, whatever the order of the sums
  Theorem 10.4   |A x - b|   <= gamma_{3n+1} |L| |L^T| |x| componentwise
Both are asserted first for LAPACK's factor / solve of the same input (which shows the input is a fair one), then for the device's."""
import numpy as np
import pytest
import torch

from oracle import lie, pvgo as opvgo
from tests.helpers import chain_problem, se3_log_err

pytestmark = pytest.mark.gpu
LW = (1, 0.1, 10, 0.1)
U = 2.0 ** -53
SIZES = (18, 63, 72, 135, 261, 585)      # one partial block | one short of 64 | just past it | ragged multi-panel, up to 10 panels
CONDS = (1e2, 1e8)


def gamma(k):
    return k * U / (1 - k * U)


def spd_matrix(n, cond, seed=0):
    """A = Q diag(s) Q^T, Q orthogonal from a seeded normal matrix, s log-spaced from 1 down to 1 / cond; symmetrised."""
    rng = np.random.default_rng(1000 * seed + n)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    s = np.logspace(0, -np.log10(cond), n)
    A = (Q * s) @ Q.T
    return 0.5 * (A + A.T)


def device_input(A, dev, diag=None):
    """What the factorisation is given: the strict upper triangle of A, NaN on and below the diagonal, the diagonal as a vector."""
    M = np.triu(A, 1) + np.tril(np.full_like(A, np.nan))
    d = np.diag(A).copy() if diag is None else diag
    return torch.tensor(M, device=dev), torch.tensor(d, device=dev)


def factor(M, d, ws):
    from islam_amd._lib import c_size_t, lib, ptr, stream_ptr
    info = torch.full((1,), -77, dtype=torch.int32, device=M.device)
    rc = lib().islam_dense_chol_factor(ptr(M), ptr(d), M.shape[0], ptr(ws[0]), c_size_t(ws[1]), ptr(info), stream_ptr(M.device))
    assert rc == 0, lib().islam_last_error()
    return info


def solve(M, b, x, ws):
    from islam_amd._lib import c_size_t, lib, ptr, stream_ptr
    rc = lib().islam_dense_chol_solve(ptr(M), M.shape[0], ptr(b), ptr(x), ptr(ws[0]), c_size_t(ws[1]), stream_ptr(M.device))
    assert rc == 0, lib().islam_last_error()


def factor_ratio(A, L):
    n = A.shape[0]
    return (np.abs(A - L @ L.T) / (gamma(n + 1) * (np.abs(L) @ np.abs(L).T))).max()


def solve_ratio(A, L, x, b):
    n = A.shape[0]
    return (np.abs(A @ x - b) / (gamma(3 * n + 1) * (np.abs(L) @ (np.abs(L).T @ np.abs(x))))).max()


_CASES = {}


def case(n, cond, dev):
    """One factorisation + solve per (n, cond), shared by the tests below and left unchanged by them."""
    key = (n, cond)
    if key not in _CASES:
        from islam_amd import ops
        A = spd_matrix(n, cond)
        b = np.random.default_rng(n).normal(size=n)
        M, d = device_input(A, dev)
        M0, d0 = M.clone(), d.clone()
        ws = ops.dense_chol_workspace(n, dev)
        info = factor(M, d, ws)
        bd = torch.tensor(b, device=dev)
        x = torch.empty_like(bd)
        solve(M, bd, x, ws)
        xa = bd.clone()
        solve(M, xa, xa, ws)                       # x aliasing b
        _CASES[key] = dict(A=A, b=b, M0=M0.cpu().numpy(), d0=d0.cpu().numpy(), M=M.cpu().numpy(), d=d.cpu().numpy(), info=int(info.item()),
                           x=x.cpu().numpy(), x_alias=xa.cpu().numpy(), b_after=bd.cpu().numpy())
    return _CASES[key]


def test_fragment_map_with_exact_integer_data(cuda):
    """A = L L^T with a small-integer L: every product, sum, square root and quotient of the factorisation is exact in float64, so the
    device must return L to the bit.  A wrong MFMA fragment map (the f32 row formula puts 3 of 4 results in the wrong row) cannot."""
    from islam_amd import ops
    n = 135
    rng = np.random.default_rng(3)
    L = np.tril(rng.integers(-2, 3, (n, n)).astype(np.float64), -1) + np.diag(rng.integers(1, 4, n).astype(np.float64))
    A = L @ L.T
    M, d = device_input(A, cuda)
    info = factor(M, d, ops.dense_chol_workspace(n, cuda))
    assert int(info.item()) == 0
    np.testing.assert_array_equal(np.tril(M.cpu().numpy()), L)


@pytest.mark.parametrize('cond', CONDS)
@pytest.mark.parametrize('n', SIZES)
def test_factorisation_error(cuda, n, cond):
    c = case(n, cond, cuda)
    ref = factor_ratio(c['A'], np.linalg.cholesky(c['A']))
    assert ref <= 1.0                                # the input is fair: LAPACK meets the bound on it
    assert c['info'] == 0
    L = np.tril(c['M'])
    assert np.isfinite(L).all()
    got = factor_ratio(c['A'], L)
    print('n=%d cond=%g: |A - L L^T| / (gamma_{n+1} |L||L^T|) = %.4f (numpy %.4f)' % (n, cond, got, ref))
    assert got <= 1.0


@pytest.mark.parametrize('cond', CONDS)
@pytest.mark.parametrize('n', SIZES)
def test_solve_backward_error(cuda, n, cond):
    from scipy.linalg import cho_factor, cho_solve
    c = case(n, cond, cuda)
    cf = cho_factor(c['A'], lower=True)
    ref = solve_ratio(c['A'], np.tril(cf[0]), cho_solve(cf, c['b']), c['b'])
    assert ref <= 1.0
    L = np.tril(c['M'])
    got = solve_ratio(c['A'], L, c['x'], c['b'])
    print('n=%d cond=%g: max_i |A x - b|_i / (gamma_{3n+1} |L||L^T||x|)_i = %.4f (scipy %.4f)' % (n, cond, got, ref))
    assert np.isfinite(c['x']).all() and got <= 1.0
    np.testing.assert_array_equal(c['x_alias'], c['x'])             # x aliasing b: the same bits
    np.testing.assert_array_equal(c['b_after'], c['b'])             # and b itself is left alone otherwise


@pytest.mark.parametrize('cond', CONDS)
@pytest.mark.parametrize('n', SIZES)
def test_storage_contract_and_determinism(cuda, n, cond):
    from islam_amd import ops
    c = case(n, cond, cuda)
    iu = np.triu_indices(n, 1)
    assert c['info'] == 0
    assert np.array_equal(c['M'][iu].view(np.int64), c['M0'][iu].view(np.int64))         # the strict upper triangle: bitwise unchanged
    assert np.array_equal(c['d'].view(np.int64), c['d0'].view(np.int64))                 # diag: bitwise unchanged
    M, d = device_input(c['A'], cuda)                                                    # a second call on a fresh copy
    ws = ops.dense_chol_workspace(n, cuda)
    assert int(factor(M, d, ws).item()) == 0
    x = torch.empty(n, dtype=torch.float64, device=cuda)
    solve(M, torch.tensor(c['b'], device=cuda), x, ws)
    il = np.tril_indices(n)
    assert np.array_equal(M.cpu().numpy()[il].view(np.int64), c['M'][il].view(np.int64))
    assert np.array_equal(x.cpu().numpy().view(np.int64), c['x'].view(np.int64))


@pytest.mark.parametrize('n,k,val', [(72, 0, -1.0), (72, 40, -1.0), (72, 70, -1.0), (261, 0, -1.0), (261, 64, -1.0), (261, 200, -1.0),
                                     (261, 64, float('nan'))])
def test_not_positive_definite(cuda, n, k, val):
    """A plain non-PD input: info is the 1-based index of the first failing pivot, as LAPACK numbers it; the remaining launches and a solve
    on the failed array return; the workspace serves a valid factorisation afterwards."""
    from islam_amd import ops
    A = spd_matrix(n, 1e2)
    diag = np.diag(A).copy()
    diag[k] = val
    Abad = A.copy()
    Abad[k, k] = val
    assert int(torch.linalg.cholesky_ex(torch.tensor(Abad))[1]) == k + 1          # LAPACK on the host, the NaN pivot included
    ws = ops.dense_chol_workspace(n, cuda)
    M, d = device_input(A, cuda, diag)
    info = factor(M, d, ws)
    x = torch.empty(n, dtype=torch.float64, device=cuda)
    solve(M, torch.ones(n, dtype=torch.float64, device=cuda), x, ws)          # values unspecified; it must return
    torch.cuda.synchronize()
    assert int(info.item()) == k + 1
    iu = np.triu_indices(n, 1)
    assert np.array_equal(M.cpu().numpy()[iu], A[iu])
    M, d = device_input(A, cuda)                                              # the same workspace, a valid matrix
    info = factor(M, d, ws)
    assert int(info.item()) == 0
    assert factor_ratio(A, np.tril(M.cpu().numpy())) <= 1.0


def test_workspace_too_small_is_an_argument_error(cuda):
    from islam_amd._lib import c_size_t, lib, ptr, stream_ptr
    n = 72
    need = lib().islam_dense_chol_workspace_bytes(n)
    M, d = device_input(spd_matrix(n, 1e2), cuda)
    M0 = M.clone()
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    info = torch.full((1,), -77, dtype=torch.int32, device=cuda)
    assert lib().islam_dense_chol_factor(ptr(M), ptr(d), n, ptr(ws), c_size_t(need - 1), ptr(info), stream_ptr(cuda)) == -1
    assert b'islam_dense_chol_factor' in lib().islam_last_error()
    b = torch.ones(n, dtype=torch.float64, device=cuda)
    assert lib().islam_dense_chol_solve(ptr(M), n, ptr(b), ptr(b), ptr(ws), c_size_t(need - 1), stream_ptr(cuda)) == -1
    assert b'islam_dense_chol_solve' in lib().islam_last_error()
    torch.cuda.synchronize()
    assert int(info.item()) == -77 and torch.equal(torch.triu(M, 1), torch.triu(M0, 1)) and bool((b == 1).all())      # nothing ran


def test_ops_wrappers(cuda):
    from islam_amd import ops
    n = 135
    A = spd_matrix(n, 1e2, seed=1)
    M, d = device_input(A, cuda)
    info = ops.dense_chol_factor(M, d)
    assert info.dtype == torch.int32 and info.is_cuda and int(info.item()) == 0
    b = torch.tensor(np.arange(n, dtype=np.float64), device=cuda)
    x = ops.dense_chol_solve(M, b)
    np.testing.assert_allclose(x.cpu().numpy(), np.linalg.solve(A, np.arange(n, dtype=np.float64)), rtol=1e-10)
    with pytest.raises(RuntimeError):
        ops.dense_chol_factor(M.cpu(), d.cpu())


# --------------------------------------------------------------------------------------------------------------- the LM on top of it
def _loop_closure_problem():
    """The 21-frame loop-closure problem of tests/test_surface_gpu.py::test_run_pvgo_general_topology_matches_oracle."""
    F = 21
    prob, tr = chain_problem(F)
    links = prob['links'].copy()
    vo = prob['vo_motions'].copy()
    gt = np.concatenate([tr['gt_pos'], tr['gt_quat']], 1)
    rng = np.random.default_rng(5)
    for e, (i, j) in {3: (0, 9), 11: (4, 17), 19: (20, 2)}.items():      # replace three chain edges by long-range ones
        links[e] = (i, j)
        rel = lie.se3_mul(lie.se3_inv(gt[i]), gt[j])
        vo[e] = lie.se3_mul(rel, lie.se3_exp(rng.normal(0, 0.01, 6)))
    return dict(prob, links=links, vo_motions=vo)


def _run(p2, **kw):
    from islam_amd import lietensor as pp
    from islam_amd.pvgo import run_pvgo
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return run_pvgo(pp.SE3(t(p2['init_nodes'])), t(p2['init_vels']), pp.SE3(t(p2['vo_motions']).to('cuda')), torch.tensor(p2['links']),
                    t(p2['dts']), pp.SO3(t(p2['imu_drots'])), t(p2['imu_dtrans']), t(p2['imu_dvels']), device='cuda', loss_weight=LW,
                    return_info=True, **kw)


def _same_lm(h, d):
    assert h[5]['steps'] == d[5]['steps'] and h[5]['trials'] == d[5]['trials']
    assert [bool(t[2]) for t in h[5]['trace']] == [bool(t[2]) for t in d[5]['trace']]
    np.testing.assert_allclose([t[0] for t in h[5]['trace']], [t[0] for t in d[5]['trace']], rtol=1e-9)
    np.testing.assert_allclose(h[2].tensor().numpy(), d[2].tensor().numpy(), atol=1e-9)
    np.testing.assert_allclose(h[3].numpy(), d[3].numpy(), atol=1e-9)


def test_lm_dense_hip_equals_dense_and_oracle(cuda):
    p2 = _loop_closure_problem()
    h, d = _run(p2, general_solver='dense_hip'), _run(p2, general_solver='dense')
    assert h[5]['trials'] > 0
    _same_lm(h, d)
    otl, orl, on, ov, _ = opvgo.run_pvgo(**p2, loss_weight=LW, mode='dense')
    err = se3_log_err(h[2].tensor().numpy(), on)
    ref = np.maximum(np.linalg.norm(lie.se3_log(on), axis=-1), 1e-6)
    assert (err / ref).max() < 1e-6
    np.testing.assert_allclose(h[3].numpy(), ov, atol=1e-7)
    np.testing.assert_allclose(h[0].cpu().numpy(), otl, rtol=1e-6, atol=1e-10)


def test_lm_dense_hip_equals_dense_under_huber(cuda):
    """delta and tolerances of tests/test_robust_gpu.py::test_loop_closure_solvers_match_restatement_and_each_other."""
    from islam_amd.robust import Huber
    from tests.test_robust_cpu import corrupt
    bad = corrupt(_loop_closure_problem(), edges=(11, 16))
    h, d = _run(bad, general_solver='dense_hip', kernel=Huber(0.1)), _run(bad, general_solver='dense', kernel=Huber(0.1))
    assert h[5]['trials'] > 0
    _same_lm(h, d)


def test_lm_dense_hip_breaks_the_step_like_dense(cuda, monkeypatch, capsys):
    """An indefinite normal matrix from a negative information scalar on the velocity factor, as in
    tests/test_pvgo_gpu.py::test_lm_solver_failure_breaks_the_step_like_pypose: every solve fails, PyPose's message is printed, the
    plateau counter ends the loop after three steps and the iterate does not move -- with either Cholesky, and with band + PCG, whose
    chain solver reports the non-positive pivot as an error status (its info dict has the three PCG entries more)."""
    from islam_amd import ops
    info = (1.0, -0.5, 100.0, 0.01)
    real = ops.pvgo_build_normal
    monkeypatch.setattr(ops, 'pvgo_build_normal', lambda lin, dts, N, w, *a, **kw: real(lin, dts, N, (0.0, info[1], info[2], info[3]), *a, **kw))
    p2 = _loop_closure_problem()
    out = {}
    for how in ('dense', 'dense_hip', 'band_pcg'):
        capsys.readouterr()
        out[how] = _run(p2, general_solver=how)
        out[how + '_text'] = capsys.readouterr().out
    d = out['dense']
    assert d[5]['steps'] == 3 and d[5]['trials'] == 3              # StopOnPlateau(patience=3): no decrease three times, one failed solve each
    assert out['dense_text'].count('Linear solver failed. Breaking optimization step...') == 3
    for how in ('dense_hip', 'band_pcg'):
        h = out[how]
        assert h[5]['steps'] == d[5]['steps'] and h[5]['trials'] == d[5]['trials'] and len(h[5]['trace']) == len(d[5]['trace']) == 3
        for th, td in zip(h[5]['trace'], d[5]['trace']):            # a failed solve is traced as (NaN, damping, rejected)
            assert np.isnan(th[0]) and np.isnan(td[0]) and th[1:] == td[1:] and th[2] is False
        assert h[5]['loss'] == d[5]['loss']
        assert out[how + '_text'] == out['dense_text']
        np.testing.assert_array_equal(h[2].tensor().numpy(), d[2].tensor().numpy())
        np.testing.assert_array_equal(h[3].numpy(), d[3].numpy())
    assert set(out['dense_hip'][5]) == set(d[5])
    assert set(out['band_pcg'][5]) == set(d[5]) | {'pcg_iterations', 'pcg_worst_relative_residual', 'off_band_edges'}
