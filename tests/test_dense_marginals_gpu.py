"""GPU tests of the in-place inverse of the dense Cholesky factor and the covariance blocks read from it (islam_dense_chol_invert_factor,
islam_pvgo_dense_cov_blocks, csrc/dense_inverse.hip), and of the marginal covariances of loop-closure graphs
built on them (pvgo_dense.marginals_dense, pvgo.pvgo_marginals_general, run_pvgo(general_solver='dense_hip', marginals=True)).

Accuracy is measured against a reference that is far more accurate than either contestant (mpmath at 50 digits for n <= 72, one
Newton step in long double above) and compared with LAPACK's error on the same input: required is
    device error <= 4 x max(LAPACK's error, n 2^-53)
with error = max over the requested blocks of |S_hat - S|_F / |S|_F.  (4: a numpy model of this blocking sat at 0.9 - 2.5 x LAPACK's
error on these inputs; the device's ratios are in DESIGN.md section 3.18.)"""
import numpy as np
import pytest
import torch

from oracle import lie
from tests.helpers import chain_problem, reproj_inputs
from tests.test_dense_marginals_cpu import exact_integer_factor, spd_matrix

pytestmark = pytest.mark.gpu
LW = (1, 0.1, 10, 0.1)
LW5 = (1, 0.1, 10, 0.1, 2.0)
T_IL = np.array([0.1, -0.05, 0.02, 0.5, -0.5, 0.5, -0.5])
U = 2.0 ** -53
SIZES = (18, 63, 72, 135, 261, 585)      # one partial block | one short of 64 | just past it | past one 128-row tile | past two | ten ragged panels
CONDS = (1e2, 1e8)
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def device_input(A, dev):
    """What the factorisation is given: the strict upper triangle of A, NaN on and below the diagonal, the diagonal as a vector."""
    M = np.triu(A, 1) + np.tril(np.full_like(A, np.nan))
    return torch.tensor(M, device=dev), torch.tensor(np.diag(A).copy(), device=dev)


def factor(M, d):
    from islam_amd import ops
    from islam_amd._lib import c_size_t, lib, ptr, stream_ptr
    ws = ops.dense_chol_workspace(M.shape[0], M.device)
    info = torch.full((1,), -77, dtype=torch.int32, device=M.device)
    rc = lib().islam_dense_chol_factor(ptr(M), ptr(d), M.shape[0], ptr(ws[0]), c_size_t(ws[1]), ptr(info), stream_ptr(M.device))
    assert rc == 0, lib().islam_last_error()
    return int(info.item())


def invert(M):
    from islam_amd._lib import c_size_t, lib, ptr, stream_ptr
    n = M.shape[0]
    need = lib().islam_dense_chol_inverse_workspace_bytes(n)
    ws = torch.empty(need, dtype=torch.uint8, device=M.device)
    rc = lib().islam_dense_chol_invert_factor(ptr(M), n, ptr(ws), c_size_t(need), stream_ptr(M.device))
    assert rc == 0, lib().islam_last_error()


def cov_blocks(M, anchor, pairs):
    from islam_amd._lib import c_void_p, lib, ptr, stream_ptr
    n = M.shape[0]
    N, P = n // 9, len(pairs)
    ph = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    node = torch.full((N, 9, 9), np.nan, dtype=torch.float64, device=M.device)
    pair = torch.full((P, 9, 9), np.nan, dtype=torch.float64, device=M.device)
    rc = lib().islam_pvgo_dense_cov_blocks(ptr(M), n, anchor, c_void_p(ph.ctypes.data if P else 0), P, ptr(node), ptr(pair) if P else c_void_p(0),
                                           stream_ptr(M.device))
    assert rc == 0, lib().islam_last_error()
    return node.cpu().numpy(), pair.cpu().numpy()


def nan_upper_(M):
    n = M.shape[0]
    iu = torch.triu_indices(n, n, 1, device=M.device)
    M[iu[0], iu[1]] = float('nan')


def request(N):
    k = (N - 1) // 2
    return [(0, N - 1), (N - 1, 0), (k, min(k + 1, N - 1)), (k, k)]


def run_device(A, dev):
    """factor, NaN into the strict upper triangle, invert, blocks: (host copy of the array, node_cov, pair_cov)"""
    M, d = device_input(A, dev)
    assert factor(M, d) == 0
    nan_upper_(M)
    invert(M)
    node, pair = cov_blocks(M, -1, request(A.shape[0] // 9))
    return M.cpu().numpy(), node, pair


def reference_inverse(A):
    """A^-1 in long double, far more accurate than double: mpmath at 50 digits for n <= 72, above that one Newton step X + X (I - A X) in
    long double from LAPACK's inverse (error about cond 2^-64)."""
    n = A.shape[0]
    if n <= 72:
        import mpmath as mp
        with mp.workdps(50):
            X = mp.matrix(A.tolist()) ** -1
            out = np.empty((n, n), dtype=LD)
            for i in range(n):
                for j in range(n):
                    hi = float(X[i, j])
                    out[i, j] = LD(hi) + LD(float(X[i, j] - hi))
        return out
    X0 = np.linalg.inv(A).astype(LD)
    Al = A.astype(LD)
    return X0 + X0 @ (np.eye(n, dtype=LD) - Al @ X0)


def block_error(node, pair, pairs, S):
    """max over the blocks of |S_hat - S|_F / |S|_F, in long double"""
    worst = LD(0)
    blocks = [(k, k, node[k]) for k in range(node.shape[0])] + [(a, b, pair[p]) for p, (a, b) in enumerate(pairs)]
    for a, b, got in blocks:
        ref = S[9 * a:9 * a + 9, 9 * b:9 * b + 9]
        worst = max(worst, np.linalg.norm((got.astype(LD) - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))
    return float(worst)


_CASES = {}


def case(n, cond, dev):
    """One device run and one reference per (n, cond), shared by the tests below and left unchanged by them."""
    key = (n, cond)
    if key not in _CASES:
        A = spd_matrix(n, cond)
        M, node, pair = run_device(A, dev)
        _CASES[key] = dict(A=A, M=M, node=node, pair=pair, pairs=request(n // 9))
    return _CASES[key]


def test_exact_integer_inverse(cuda):
    """L = D (I - M), M block-nilpotent, D powers of two (tests/test_dense_marginals_cpu.py shows the construction is exact in float64):
    every product and sum of the blocked inverse is exact, so the device must return (I + M + M^2) D^-1 to the bit.  The blocks of M
    straddle the panel boundaries 64 and 128 and the wave boundaries of the update; a wrong fragment map, a wrong K range or an
    unmasked diagonal tile cannot pass.  NaN in the strict upper triangle stays NaN and reaches nothing."""
    L, W = exact_integer_factor()
    n = L.shape[0]
    M = torch.tensor(np.tril(L) + np.triu(np.full_like(L, np.nan), 1), device=cuda)
    invert(M)
    out = M.cpu().numpy()
    assert np.isnan(out[np.triu_indices(n, 1)]).all()
    got = np.tril(out)
    assert np.array_equal(got, W), 'first mismatch at %s' % (np.argwhere(got != W)[:1],)


def test_exact_integer_inverse_past_the_column_split_threshold(cuda):
    """n = 8280: the first block column has 8216 rows below it, more than the 8192 above which the update takes 32 columns per workgroup
    instead of 16, so both instances of the kernel run.  The same kind of exact construction, built sparsely on the device (no n x n host
    array): L = D (I - M), M = B1 + B2 with B1 in rows [100, n) x 16 columns spread over the four 16-column groups of block column 0, B2 in
    four bands of four rows (the last rows among them) x columns [100, 5000).  B1 B1 = B1 B2 = B2 B2 = 0 (no column index of one is a row
    index of the other), so M^2 = B2 B1, M^3 = 0 and L^-1 = (I + M + M^2) D^-1: sums of up to 4900 products, exact in float64."""
    n = 8280
    rng = np.random.default_rng(11)
    d = 2.0 ** rng.integers(-2, 3, n)
    C1 = np.r_[0:4, 20:24, 40:44, 60:64]
    R2 = np.concatenate([np.arange(b, b + 4) for b in (5000, 6500, 8200, n - 4)])
    B1 = rng.integers(-2, 3, (n - 100, 16)).astype(np.float64)
    B2 = rng.integers(-2, 3, (16, 4900)).astype(np.float64)
    M2 = B2 @ B1[:4900]                                                  # rows R2 x columns C1
    assert np.abs(M2).max() > 50
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=cuda)
    c1, r2 = t(C1), t(R2)
    L = torch.zeros((n, n), dtype=torch.float64, device=cuda)
    L.diagonal().copy_(t(d))
    L[100:, c1] = t(-d[100:, None] * B1)
    L[r2, 100:5000] = t(-d[R2][:, None] * B2)
    E = torch.zeros((n, n), dtype=torch.float64, device=cuda)
    E.diagonal().copy_(t(1.0 / d))
    E[100:, c1] = t(B1 / d[C1][None, :])
    E[r2, 100:5000] = t(B2 / d[100:5000][None, :])
    E[r2[:, None], c1[None, :]] = t((B1[R2 - 100] + M2) / d[C1][None, :])
    upper = torch.ones((n, n), dtype=torch.bool, device=cuda).triu(1)
    L.masked_fill_(upper, float('nan'))
    invert(L)
    assert bool(torch.isnan(L[upper]).all())
    L.masked_fill_(upper, 0.0)
    bad = (L != E).nonzero()
    assert bad.shape[0] == 0, 'first mismatches at %s' % (bad[:4].tolist(),)


@pytest.mark.parametrize('cond', CONDS)
@pytest.mark.parametrize('n', SIZES)
def test_covariance_block_accuracy(cuda, n, cond):
    if n > 72 and np.finfo(LD).eps > 2e-19:
        pytest.skip('long double is not an extended format here')
    c = case(n, cond, cuda)
    N = n // 9
    S = reference_inverse(c['A'])
    X = np.linalg.inv(c['A'])
    Xn = np.stack([X[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(N)])
    Xp = np.stack([X[9 * a:9 * a + 9, 9 * b:9 * b + 9] for a, b in c['pairs']])
    ref = block_error(Xn, Xp, c['pairs'], S)
    got = block_error(c['node'], c['pair'], c['pairs'], S)
    cap = 4 * max(ref, n * U)
    print('n=%d cond=%g: block error device %.3e, LAPACK %.3e, ratio %.2f (cap %.3e)' % (n, cond, got, ref, got / max(ref, n * U), cap))
    assert np.isfinite(c['node']).all() and np.isfinite(c['pair']).all()
    assert got <= cap
    # (a, b) and (b, a) form the same products in the same order: transposes of each other to the bit
    assert c['pairs'][0] == (0, N - 1) and c['pairs'][1] == (N - 1, 0)
    assert np.array_equal(c['pair'][0], c['pair'][1].T)
    assert np.array_equal(c['node'], c['node'].transpose(0, 2, 1))


@pytest.mark.parametrize('cond', CONDS)
@pytest.mark.parametrize('n', SIZES)
def test_storage_contract_and_determinism(cuda, n, cond):
    """The strict upper triangle was overwritten with NaN after the factorisation: it is still NaN (never written) and the inverse and
    the blocks are finite (never read as data).  A second run on a fresh copy gives the same bits."""
    c = case(n, cond, cuda)
    iu, il = np.triu_indices(n, 1), np.tril_indices(n)
    assert np.isnan(c['M'][iu]).all()
    assert np.isfinite(c['M'][il]).all() and np.isfinite(c['node']).all() and np.isfinite(c['pair']).all()
    M, node, pair = run_device(c['A'], cuda)
    assert np.array_equal(M[il].view(np.int64), c['M'][il].view(np.int64))
    assert np.array_equal(node.view(np.int64), c['node'].view(np.int64)) and np.array_equal(pair.view(np.int64), c['pair'].view(np.int64))


def test_null_outputs_and_no_pairs(cuda):
    """P = 0 with pairs = NULL, node_cov or pair_cov NULL: the other output is written and equals the full call's."""
    from islam_amd._lib import c_void_p, lib, ptr, stream_ptr
    c = case(135, 1e2, cuda)
    M = torch.tensor(c['M'], device=cuda)
    N = 15
    node = torch.empty((N, 9, 9), dtype=torch.float64, device=cuda)
    assert lib().islam_pvgo_dense_cov_blocks(ptr(M), 135, -1, c_void_p(0), 0, ptr(node), c_void_p(0), stream_ptr(cuda)) == 0
    assert np.array_equal(node.cpu().numpy(), c['node'])
    ph = np.asarray(c['pairs'], dtype=np.int64)
    pair = torch.empty((len(ph), 9, 9), dtype=torch.float64, device=cuda)
    assert lib().islam_pvgo_dense_cov_blocks(ptr(M), 135, -1, c_void_p(ph.ctypes.data), len(ph), c_void_p(0), ptr(pair), stream_ptr(cuda)) == 0
    assert np.array_equal(pair.cpu().numpy(), c['pair'])
    # more pairs than one launch carries (384): every block lands in its own slot
    many = np.array([(a, b) for a in range(N) for b in range(N)] * 2, dtype=np.int64)
    assert len(many) > 384
    _, got = cov_blocks(M, -1, many)
    S = np.tril(c['M']).T @ np.tril(c['M'])
    for p in (0, 1, 200, 383, 384, 385, len(many) - 1):
        a, b = many[p]
        np.testing.assert_allclose(got[p], S[9 * a:9 * a + 9, 9 * b:9 * b + 9], rtol=0, atol=1e-12 * np.abs(S).max())
    assert np.array_equal(got[:N * N], got[N * N:])


def test_failed_factor_terminates(cuda):
    """A factor that holds NaN (a failed pivot): every launch of the inverse and of the blocks returns."""
    A = spd_matrix(261, 1e2)
    A[70, 70] = -1.0
    M, d = device_input(A, cuda)
    assert factor(M, d) == 71
    invert(M)
    cov_blocks(M, 0, request(29))
    torch.cuda.synchronize()
    assert np.array_equal(np.triu(M.cpu().numpy(), 1), np.triu(A, 1))


# ------------------------------------------------------------------------------------------------------------------ anchor
def _anchored_inverse(A, N, anchor):
    """The construction of tests/test_marginals_gpu.py: the inverse of A with the anchor's six pose rows and columns deleted."""
    keep = np.ones(9 * N, dtype=bool)
    if anchor is not None:
        keep[9 * anchor:9 * anchor + 6] = False
    S = np.zeros_like(A)
    idx = np.nonzero(keep)[0]
    S[np.ix_(idx, idx)] = np.linalg.inv(A[np.ix_(idx, idx)])
    return S


def _worst_block_error(node, pairs, pair, S):
    """max |error| / (largest entry of the column of Sigma), the measure of tests/test_marginals_gpu.py::_check_against_dense, over the
    diagonal blocks and the requested pairs (rows node a, columns node b)."""
    N = node.shape[0]
    col = np.maximum(np.abs(S).max(axis=0).reshape(N, 9), 1e-300)
    worst = max(np.max(np.abs(node[k] - S[9 * k:9 * k + 9, 9 * k:9 * k + 9]) / col[k][None, :]) for k in range(N))
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2)):
        worst = max(worst, np.max(np.abs(pair[p] - S[9 * a:9 * a + 9, 9 * b:9 * b + 9]) / col[b][None, :]))
    return worst


@pytest.mark.parametrize('anchor', [None, 0, 7, 14])
def test_anchor(cuda, anchor):
    """Both inverses carry a forward error of at most c n u cond (Higham, section 14): rtol = 64 n u cond relative to the column's largest
    entry.  The anchored rows and columns are exactly zero."""
    from islam_amd import ops
    from islam_amd.pvgo_dense import fix_gauge
    n, N, cond = 135, 15, 1e2
    A = spd_matrix(n, cond, seed=2)
    M = torch.tensor(A, device=cuda)
    d = fix_gauge(M, anchor)
    il = torch.tril_indices(n, n, device=cuda)
    M[il[0], il[1]] = float('nan')                            # the factorisation reads the strict upper triangle and d only
    assert int(ops.dense_chol_factor(M, d).item()) == 0
    ops.dense_chol_invert_factor(M)
    pairs = [(a, b) for a in (0, 7, 14) for b in (0, 6, 7, 8, 14)]
    node, pair = ops.pvgo_dense_cov_blocks(M, anchor=anchor, pairs=pairs)
    node, pair = node.cpu().numpy(), pair.cpu().numpy()
    S = _anchored_inverse(A, N, anchor)
    worst = _worst_block_error(node, pairs, pair, S)
    print('anchor=%s: worst error / column scale = %.3e' % (anchor, worst))
    assert worst <= 64 * n * U * cond
    if anchor is not None:
        assert not node[anchor][:6, :].any() and not node[anchor][:, :6].any()
        for p, (a, b) in enumerate(pairs):
            assert a != anchor or not pair[p][:6, :].any()
            assert b != anchor or not pair[p][:, :6].any()
        assert node[anchor][6:, 6:].all()
    else:
        assert node.all() and pair.all()


# ------------------------------------------------------------------------------------------------------------------ graphs
def _loop_closure_problem(extra=()):
    """The 21-frame loop-closure problem of tests/test_dense_chol_gpu.py: edges (0,9), (4,17), (20,2) replace three chain edges; `extra`
    edges are appended with VO motions of the same kind."""
    F = 21
    prob, tr = chain_problem(F)
    links = prob['links'].copy()
    vo = prob['vo_motions'].copy()
    gt = np.concatenate([tr['gt_pos'], tr['gt_quat']], 1)
    rng = np.random.default_rng(5)
    rel = lambda i, j: lie.se3_mul(lie.se3_mul(lie.se3_inv(gt[i]), gt[j]), lie.se3_exp(rng.normal(0, 0.01, 6)))
    for e, (i, j) in {3: (0, 9), 11: (4, 17), 19: (20, 2)}.items():
        links[e] = (i, j)
        vo[e] = rel(i, j)
    for (i, j) in extra:
        links = np.concatenate([links, [[i, j]]])
        vo = np.concatenate([vo, rel(i, j)[None]])
    return dict(prob, links=links, vo_motions=vo), tr


def _dev(prob, cuda):
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    return dict(nodes=t(prob['init_nodes']), vels=t(prob['init_vels']), vo_motions=t(prob['vo_motions']),
                links=torch.tensor(np.asarray(prob['links']), dtype=torch.int64, device=cuda), dts=t(prob['dts']), imu_drots=t(prob['imu_drots']),
                imu_dtrans=t(prob['imu_dtrans']), imu_dvels=t(prob['imu_dvels']))


def _host_matrix(d, lw, rp=None):
    from islam_amd.pvgo_dense import gauss_newton_matrix
    A = gauss_newton_matrix(d['nodes'], d['vels'], d['links'], d['vo_motions'], d['imu_drots'], d['imu_dtrans'], d['imu_dvels'], d['dts'], lw, rp)
    A = A.cpu().numpy()
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()             # symmetric up to the rounding of the reprojection blocks
    return np.triu(A) + np.triu(A, 1).T                                 # what the factorisation reads: the upper triangle and the diagonal


@pytest.mark.parametrize('F', [9, 21])
def test_general_matches_chain_selected_inversion(cuda, F):
    """Two implementations of the same covariances on a canonical chain -- the block-tridiagonal selected inversion (pvgo_marginals) and
    the dense inverse (pvgo_marginals_general) -- against each other and against numpy's inverse of the assembled matrix."""
    from islam_amd import pvgo
    prob, _ = chain_problem(F)
    d = _dev(prob, cuda)
    ch = pvgo.pvgo_marginals(d['nodes'], d['vels'], d['vo_motions'], d['dts'], d['imu_drots'], d['imu_dtrans'], d['imu_dvels'], loss_weight=LW)
    ge = pvgo.pvgo_marginals_general(**d, loss_weight=LW)
    assert isinstance(ge, pvgo.PvgoGraphMarginals) and ge.anchor == 0
    assert ge.pairs.cpu().tolist() == np.asarray(prob['links']).tolist()              # pairs=None: the graph's own links
    S = _anchored_inverse(_host_matrix(d, LW), F, 0)
    pairs = np.asarray(prob['links'])
    gn, gp, cn, cc = ge.node_cov.cpu().numpy(), ge.pair_cov.cpu().numpy(), ch.node_cov.cpu().numpy(), ch.cross.cpu().numpy()
    e_g, e_c = _worst_block_error(gn, pairs, gp, S), _worst_block_error(cn, pairs, cc, S)
    col = np.maximum(np.abs(S).max(axis=0).reshape(F, 9), 1e-300)
    e_x = max(np.max(np.abs(gn - cn) / col[:, None, :]), np.max(np.abs(gp - cc) / col[1:, None, :]))
    print('F=%d: dense vs numpy %.3e, chain vs numpy %.3e, dense vs chain %.3e (relative to the column scale)' % (F, e_g, e_c, e_x))
    assert e_g <= 1e-9 and e_c <= 1e-9 and e_x <= 1e-9
    assert not gn[0][:6, :].any() and not gn[0][:, :6].any()
    assert ge.pose_cov.shape == (F, 6, 6) and ge.vel_cov.shape == (F, 3, 3)
    assert torch.equal(ge.pose_cov, ge.node_cov[:, :6, :6]) and torch.equal(ge.vel_cov, ge.node_cov[:, 6:, 6:])


def _reproj(tr, cuda):
    from islam_amd import dense_ba, lietensor as pp
    inp = reproj_inputs(tr, 40, T_IL)
    th = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return dense_ba.SparseReprojectionLoss(th(inp['points2d']), th(inp['depth']), th(inp['flow']), inp['fx'], inp['fy'], inp['cx'], inp['cy'],
                                           pp.SE3(th(T_IL)), device=cuda)


@pytest.mark.parametrize('with_reproj', [False, True])
def test_loop_closures_against_numpy(cuda, with_reproj):
    from islam_amd import pvgo
    prob, tr = _loop_closure_problem()
    d = _dev(prob, cuda)
    lw = LW5 if with_reproj else LW
    hip = _reproj(tr, cuda) if with_reproj else None
    F = 21
    pairs = [tuple(l) for l in np.asarray(prob['links']).tolist()] + [(9, 0), (20, 0), (5, 5), (0, 20)]
    for anchor in (0, 10):
        mg = pvgo.pvgo_marginals_general(**d, loss_weight=lw, reproj=hip, anchor=anchor, pairs=pairs)
        S = _anchored_inverse(_host_matrix(d, lw, pvgo._reproj_struct(hip, lw, cuda)), F, anchor)
        worst = _worst_block_error(mg.node_cov.cpu().numpy(), pairs, mg.pair_cov.cpu().numpy(), S)
        print('loop closures, reproj=%s, anchor=%d: worst error / column scale = %.3e' % (with_reproj, anchor, worst))
        assert worst <= 1e-9
        assert mg.pairs.shape == (len(pairs), 2) and not mg.pose_cov[anchor].any()
    if with_reproj:                   # the factor changes the answer (a dropped term would go unnoticed otherwise)
        without = pvgo.pvgo_marginals_general(**d, loss_weight=lw, anchor=10, pairs=pairs)
        assert not torch.allclose(without.node_cov, mg.node_cov, rtol=1e-3, atol=0)


def test_information_monotonicity(cuda):
    """One more closure (0, 20) at the same state adds a positive semi-definite term to A, so no marginal covariance may grow: every
    eigenvalue of Sigma_before,kk - Sigma_after,kk is >= -1e-9 |Sigma_before,kk| (spectral norm)."""
    from islam_amd import pvgo
    before, _ = _loop_closure_problem()
    after, _ = _loop_closure_problem(extra=[(0, 20)])
    assert len(after['links']) == 21 and np.array_equal(after['links'][:20], before['links'])
    Sb = pvgo.pvgo_marginals_general(**_dev(before, cuda), loss_weight=LW).node_cov.cpu().numpy()
    Sa = pvgo.pvgo_marginals_general(**_dev(after, cuda), loss_weight=LW).node_cov.cpu().numpy()
    gain = 0.0
    for k in range(21):
        D = Sb[k] - Sa[k]
        ev = np.linalg.eigvalsh(0.5 * (D + D.T))
        assert ev.min() >= -1e-9 * np.linalg.norm(Sb[k], 2), (k, ev.min())
        gain = max(gain, ev.max() / max(np.linalg.norm(Sb[k], 2), 1e-300))
    assert gain > 1e-3                                      # and the closure does pull the far end's uncertainty down


# ------------------------------------------------------------------------------------------------------------------ surface
def _run(p2, **kw):
    from islam_amd import lietensor as pp
    from islam_amd.pvgo import run_pvgo
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return run_pvgo(pp.SE3(t(p2['init_nodes'])), t(p2['init_vels']), pp.SE3(t(p2['vo_motions']).to('cuda')), torch.tensor(p2['links']),
                    t(p2['dts']), pp.SO3(t(p2['imu_drots'])), t(p2['imu_dtrans']), t(p2['imu_dvels']), device='cuda', loss_weight=LW,
                    return_info=True, **kw)


def _plain(x):
    from islam_amd import lietensor as pp
    return pp._plain(x).detach().cpu()


def test_run_pvgo_surface(cuda):
    from islam_amd import pvgo
    from islam_amd.robust import Huber
    p2, _ = _loop_closure_problem()
    base = _run(p2, general_solver='dense_hip')
    out = _run(p2, general_solver='dense_hip', marginals=True)
    assert len(out) == len(base) + 1
    for a, b in zip(base[:4], out[:4]):
        assert torch.equal(_plain(a), _plain(b))
    mg = out[-1]
    assert isinstance(mg, pvgo.PvgoGraphMarginals) and mg.anchor == 0
    assert mg.node_cov.shape == (21, 9, 9) and mg.pair_cov.shape == (20, 9, 9) and mg.pairs.cpu().tolist() == p2['links'].tolist()
    assert not mg.pose_cov[0].any()
    assert torch.isfinite(mg.node_cov).all() and torch.isfinite(mg.pair_cov).all()
    assert (torch.diagonal(mg.node_cov[1:], dim1=1, dim2=2) > 0).all()
    # computed at the aligned fp64 state the caller receives
    d = _dev(p2, cuda)
    d['nodes'], d['vels'] = _plain(out[2]).to(cuda, torch.float64), out[3].to(cuda, torch.float64)
    ref = pvgo.pvgo_marginals_general(**d, loss_weight=LW)
    assert torch.equal(ref.node_cov, mg.node_cov) and torch.equal(ref.pair_cov, mg.pair_cov)
    for how in ('auto', 'dense', 'band_pcg'):
        with pytest.raises(pvgo.UnsupportedGraphError):
            _run(p2, general_solver=how, marginals=True)
    with pytest.raises(NotImplementedError):
        _run(p2, general_solver='dense_hip', marginals=True, kernel=Huber(0.1))


def test_indefinite_matrix_raises(cuda, monkeypatch):
    """The negative information scalar of tests/test_dense_chol_gpu.py::test_lm_dense_hip_breaks_the_step_like_dense."""
    from islam_amd import ops, pvgo
    from islam_amd._lib import IslamHipError
    info = (1.0, -0.5, 100.0, 0.01)
    real = ops.pvgo_build_normal
    monkeypatch.setattr(ops, 'pvgo_build_normal', lambda lin, dts, N, w, *a, **kw: real(lin, dts, N, (0.0, info[1], info[2], info[3]), *a, **kw))
    p2, _ = _loop_closure_problem()
    with pytest.raises(IslamHipError) as e:
        pvgo.pvgo_marginals_general(**_dev(p2, cuda), loss_weight=LW)
    assert e.value.code == -3 and 'not positive definite' in str(e.value)


def test_cpu_tensors_raise(cuda):
    from islam_amd import ops, pvgo
    p2, _ = _loop_closure_problem()
    d = {k: v.cpu() for k, v in _dev(p2, cuda).items()}
    with pytest.raises(RuntimeError):
        pvgo.pvgo_marginals_general(**d, loss_weight=LW)
    A = torch.eye(18, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.dense_chol_invert_factor(A)
    with pytest.raises(RuntimeError):
        ops.pvgo_dense_cov_blocks(A)
    with pytest.raises(ValueError):
        ops.pvgo_dense_cov_blocks(torch.eye(20, dtype=torch.float64, device=cuda))
