"""GPU tests of the marginal covariances of loop-closure graphs from the band form: the columns of B_a^-1
(islam_pvgo_band_inverse_columns), the fragment map of the projection and the block kernels on exact integers
(islam_pvgo_band_cov_blocks), pvgo_marginals_general(method='band') against numpy's anchored inverse and against method='dense',
run_pvgo(marginals='band'), and a 3000-frame graph that no dense array could serve within the asserted memory.

Tolerance: the project's 1e-9 of the column scale (tests/test_dense_marginals_gpu.py); a numpy model of the formula sits at or below
4e-13 of numpy's inverse on the graphs used here (tests/test_band_marginals_cpu.py asserts 1e-11), all with N <= 65."""
import functools

import numpy as np
import pytest
import torch

from tests.closure_graphs import CASES, LW, UNIT, case, closure_graph, sizes
from tests.test_band_marginals_cpu import anchored_inverse, oracle_matrix

pytestmark = pytest.mark.gpu
ENOTPD = -3
F65_CLOSURES = ((0, 64), (10, 50), (33, 3))


def _dev(prob):
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    return dict(nodes=t(prob['init_nodes']), vels=t(prob['init_vels']), vo_motions=t(prob['vo_motions']),
                links=torch.tensor(np.asarray(prob['links']), dtype=torch.int64, device='cuda'), dts=t(prob['dts']),
                imu_drots=t(prob['imu_drots']), imu_dtrans=t(prob['imu_dtrans']), imu_dvels=t(prob['imu_dvels']))


@functools.lru_cache(maxsize=None)
def _f65(with_closures=True):
    return closure_graph(65, F65_CLOSURES if with_closures else ())


def _worst(mg, S):
    from tests.test_dense_marginals_gpu import _worst_block_error
    return _worst_block_error(mg.node_cov.cpu().numpy(), mg.pairs.cpu().numpy(), mg.pair_cov.cpu().numpy(), S)


def _between(a, b, S):
    """worst |a - b| / column scale of S over the node and pair blocks of two PvgoGraphMarginals with the same pairs"""
    N = a.node_cov.shape[0]
    col = torch.tensor(np.maximum(np.abs(S).max(axis=0).reshape(N, 9), 1e-300), device='cuda')
    e = ((a.node_cov - b.node_cov).abs() / col[:, None, :]).max()
    if a.pairs.shape[0]:
        e = torch.maximum(e, ((a.pair_cov - b.pair_cov).abs() / col[a.pairs[:, 1]][:, None, :]).max())
    return float(e)


def _anchor_is_zero(mg):
    k = mg.anchor
    assert not mg.node_cov[k][:6, :].any() and not mg.node_cov[k][:, :6].any()
    for p, (a, b) in enumerate(mg.pairs.cpu().tolist()):
        assert a != k or not mg.pair_cov[p][:6, :].any()
        assert b != k or not mg.pair_cov[p][:, :6].any()


# ------------------------------------------------------------------------------------------------------------------ columns
def _band(prob, ridge=0.0):
    """(Hd, Ho) of islam_pvgo_band_assemble at the initial state and the block-tridiagonal matrix they stand for.  ridge: that fraction
    of the largest diagonal entry added to every diagonal entry (without a gauge fix the band of a PVGO graph is singular: a common
    translation of all nodes changes no residual)."""
    from tests.test_added_edges_gpu import _band_assembly, _device_pieces
    N = prob['init_nodes'].shape[0]
    _, _, _, (Hd, Ho, _, _, _) = _band_assembly(*_device_pieces(prob), N, LW)
    if ridge:
        Hd = Hd + ridge * float(Hd.diagonal(dim1=1, dim2=2).max()) * torch.eye(9, dtype=torch.float64, device='cuda')
    hd, ho = Hd.cpu().numpy(), Ho.cpu().numpy()
    B = np.zeros((9 * N, 9 * N))
    for k in range(N):
        B[9 * k:9 * k + 9, 9 * k:9 * k + 9] = hd[k]
        if k < N - 1:
            B[9 * k:9 * k + 9, 9 * k + 9:9 * k + 18] = ho[k]
            B[9 * k + 9:9 * k + 18, 9 * k:9 * k + 9] = ho[k].T
    return Hd.contiguous(), Ho, B


@pytest.mark.parametrize('name', ['n3e4', 'more17', 'f65'])
def test_inverse_columns_against_numpy(cuda, name):
    from islam_amd import ops
    from islam_amd.pvgo_dense import band_columns
    prob = _f65() if name == 'f65' else case(name)
    N = prob['init_nodes'].shape[0]
    for anchor in (None, 0, N // 2):
        Hd, Ho, B = _band(prob, ridge=1e-6 if anchor is None else 0.0)
        keep = (Hd.clone(), Ho.clone())
        cols, _ = band_columns(N, prob['links'], anchor, np.concatenate([prob['links'], [[0, N - 1], [N - 1, 0]]]))
        assert cols.size >= 9
        status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
        Y = ops.pvgo_band_inverse_columns(Hd, Ho, cols, anchor, status=status)
        assert int(status.item()) == 0 and Y.shape == (9 * N, cols.size)
        S = anchored_inverse(0.5 * (B + B.T), anchor)[:, cols]
        got = Y.cpu().numpy()
        err = np.max(np.abs(got - S) / np.abs(S).max(axis=0)[None, :])
        print('%s anchor=%s: R=%d, worst |Y - inverse| / column scale = %.3e' % (name, anchor, cols.size, err))
        assert err <= 1e-9
        if anchor is not None:
            assert not got[9 * anchor:9 * anchor + 6].any()
        assert torch.equal(Hd, keep[0]) and torch.equal(Ho, keep[1])               # the inputs are left alone
        assert torch.equal(ops.pvgo_band_inverse_columns(Hd, Ho, cols, anchor), Y)    # the same bits again


def test_indefinite_band_sets_the_status(cuda):
    from islam_amd import ops
    Hd, Ho, _ = _band(case('more17'))
    Hd[5, 7, 7] = -1.0
    status = torch.zeros((1,), dtype=torch.int32, device='cuda')
    ops.pvgo_band_inverse_columns(Hd, Ho, [9, 10, 11], 0, status=status)
    assert int(status.item()) == ENOTPD


# ------------------------------------------------------------------------------------------------------------------ fragment map
def _integer_case(N, Rc, anchor=0, seed=0):
    """Small-integer Y, G (symmetric), Sd (symmetric), So and a valid column list whose first Rc entries are pose DoF: every product and
    sum below stays an integer far under 2^53 (or a half of one, where two entries are averaged), so the host arithmetic is exact."""
    rng = np.random.default_rng(100 * N + Rc + seed)
    pose = [9 * k + c for k in range(N) if k != anchor for c in range(6)]
    closure = pose[:Rc]
    assert len(closure) == Rc
    extra = [9 * b + c for b in (0, N - 1) for c in range(9) if not (b == anchor and c < 6) and 9 * b + c not in closure]
    cols = np.array(closure + extra, dtype=np.int64)
    Y = rng.integers(-2, 3, (9 * N, cols.size)).astype(np.float64)
    Y[9 * anchor:9 * anchor + 6] = 0.0
    G = rng.integers(-2, 3, (Rc, Rc)).astype(np.float64)
    G = np.triu(G) + np.triu(G, 1).T
    Sd = rng.integers(-9, 10, (N, 9, 9)).astype(np.float64)
    Sd = Sd + Sd.transpose(0, 2, 1)
    So = rng.integers(-9, 10, (N - 1, 9, 9)).astype(np.float64)
    pairs = np.array([(1, 1), (0, 0), (0, 1), (1, 0), (N - 2, N - 1), (N - 1, N - 2), (0, N - 1), (N - 1, 0), (1, N - 1), (N - 1, N - 1),
                      (N - 2, 0)])                         # (node N - 2 has no velocity columns: formed directly, not as a transpose)
    return cols, Y, G, Sd, So, pairs


def _integer_reference(cols, Rc, Y, G, Sd, So, pairs, anchor):
    N = Sd.shape[0]
    V = Y[:, :Rc] @ G
    C = V @ Y[:, :Rc].T
    where = {int(c): r for r, c in enumerate(cols)}
    blk = lambda a, b: C[9 * a:9 * a + 9, 9 * b:9 * b + 9]

    def fix(X, a, b):
        X = X.copy()
        if a == anchor:
            X[:6, :] = 0.0
        if b == anchor:
            X[:, :6] = 0.0
        return X

    sym = lambda X: 0.5 * (X + X.T)
    node = np.stack([fix(sym(Sd[k] - blk(k, k)), k, k) for k in range(N)])
    holds = lambda n: all(9 * n + c in where for c in range(6 if n == anchor else 0, 9))
    pair = []
    for a, b in pairs:
        if a - b > 1 and holds(a):                          # formed as block (b, a), stored transposed
            X = np.zeros((9, 9))
            for c in range(9):
                if 9 * a + c in where:
                    X[:, c] = Y[9 * b:9 * b + 9, where[9 * a + c]]
            pair.append(fix(X - blk(b, a), b, a).T)
            continue
        if a == b:
            base = Sd[a]
        elif b == a + 1:
            base = So[a]
        elif a == b + 1:
            base = So[b].T
        else:
            base = np.zeros((9, 9))
            for c in range(9):
                if 9 * b + c in where:
                    base[:, c] = Y[9 * a:9 * a + 9, where[9 * b + c]]
        X = base - blk(a, b)
        pair.append(fix(sym(X) if a == b else X, a, b))
    return node, np.stack(pair)


@pytest.mark.parametrize('N,Rc', [(3, 6), (17, 30), (15, 64), (29, 66), (29, 130)])
def test_fragment_map_on_exact_integers(cuda, N, Rc):
    """Below one 16-column chunk | ragged | exactly one 64-column workgroup | just past it | past two 128-row tiles and two column
    workgroups.  Bit-equal to integer arithmetic on the host; two calls give the same bits."""
    from islam_amd import ops
    cols, Y, G, Sd, So, pairs = _integer_case(N, Rc)
    d = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    args = (d(Sd), d(So), d(Y), cols, Rc, d(G), 0, pairs)
    node, pair = ops.pvgo_band_cov_blocks(*args, status=status)
    want_node, want_pair = _integer_reference(cols, Rc, Y, G, Sd, So, pairs, 0)
    assert np.array_equal(node.cpu().numpy(), want_node)
    assert np.array_equal(pair.cpu().numpy(), want_pair)
    assert np.abs(want_pair[6][:, 6:]).max() > 0 and np.abs(want_pair[7][6:, :]).max() > 0       # the far pairs with the anchor carry data
    bad = any(not want_node[k][i, i] > 0 for k in range(N) for i in range(9) if not (k == 0 and i < 6))
    assert int(status.item()) == (ENOTPD if bad else 0)
    node2, pair2 = ops.pvgo_band_cov_blocks(*args)
    assert torch.equal(node, node2) and torch.equal(pair, pair2)


def test_no_closure_copies_the_chain_blocks(cuda):
    from islam_amd import ops
    cols, Y, _, Sd, So, pairs = _integer_case(5, 0)
    d = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    Sd = Sd + 100.0 * np.eye(9)[None]
    node, pair = ops.pvgo_band_cov_blocks(d(Sd), d(So), d(Y), cols, 0, None, 0, pairs, status=status)
    want_node, want_pair = _integer_reference(cols, 0, Y, np.zeros((0, 0)), Sd, So, pairs, 0)
    assert np.array_equal(node.cpu().numpy(), want_node) and np.array_equal(pair.cpu().numpy(), want_pair)
    assert int(status.item()) == 0
    assert np.array_equal(want_node[2], Sd[2]) and np.array_equal(want_pair[4], So[3])


def test_more_pairs_than_one_launch(cuda):
    """Every block lands in its own slot when the pairs fill several launches (160 pairs, or 48 distinct far second nodes, each)."""
    from islam_amd import ops
    N, Rc = 60, 20
    rng = np.random.default_rng(4)
    closure = [9 * k + c for k in range(1, 5) for c in range(6)][:Rc]
    cols = np.array(closure + [c for c in range(6, 9 * N) if c not in closure], dtype=np.int64)      # every DoF but the anchor's pose
    Y = rng.integers(-2, 3, (9 * N, cols.size)).astype(np.float64)
    G = rng.integers(-2, 3, (Rc, Rc)).astype(np.float64)
    G = np.triu(G) + np.triu(G, 1).T
    Sd = rng.integers(-9, 10, (N, 9, 9)).astype(np.float64)
    Sd = Sd + Sd.transpose(0, 2, 1)
    So = rng.integers(-9, 10, (N - 1, 9, 9)).astype(np.float64)
    pairs = np.array([(a, b) for a in (0, 7, 59) for b in range(N)] + [(a, a + 1) for a in range(N - 1)] * 3)
    assert len(pairs) > 2 * 160 and len(set(pairs[:100, 1])) > 48
    d = lambda a: torch.tensor(a, dtype=torch.float64, device='cuda')
    _, pair = ops.pvgo_band_cov_blocks(d(Sd), d(So), d(Y), cols, Rc, d(G), 0, pairs)
    assert np.array_equal(pair.cpu().numpy(), _integer_reference(cols, Rc, Y, G, Sd, So, pairs, 0)[1])


# ------------------------------------------------------------------------------------------------------------------ references
def _extra_pairs(prob):
    N = prob['init_nodes'].shape[0]
    far = [(N - 1, 0), (0, N - 1), (N // 2, N // 2)] + ([(N // 2, 0), (1, N - 1)] if N > 3 else [])
    return [tuple(l) for l in np.asarray(prob['links']).tolist()] + far


@pytest.mark.parametrize('name', sorted(CASES))
def test_band_against_numpy_and_dense_on_the_closure_graphs(cuda, name):
    from islam_amd import pvgo
    prob = case(name)
    N = sizes(name)[0]
    A = oracle_matrix(name)
    pairs = _extra_pairs(prob)
    for anchor in (0, N // 2):
        band = pvgo.pvgo_marginals_general(**_dev(prob), loss_weight=LW, anchor=anchor, pairs=pairs, method='band')
        dense = pvgo.pvgo_marginals_general(**_dev(prob), loss_weight=LW, anchor=anchor, pairs=pairs)
        assert band.method == 'band' and dense.method == 'dense' and band.anchor == anchor and torch.equal(band.pairs, dense.pairs)
        S = anchored_inverse(A, anchor)
        e_np, e_dense = _worst(band, S), _between(band, dense, S)
        print('%s anchor=%d: band vs numpy %.3e, band vs dense %.3e, dense vs numpy %.3e (of the column scale)'
              % (name, anchor, e_np, e_dense, _worst(dense, S)))
        assert e_np <= 1e-9 and e_dense <= 1e-9
        _anchor_is_zero(band)


def test_band_under_per_factor_information(cuda):
    from islam_amd import pvgo
    from tests.test_added_edges_cpu import info_omegas
    from tests.test_added_edges_gpu import _reference_for
    from tests.test_info_cpu import pvgo_info
    prob, N = case('more17'), 17
    A = _reference_for('more17', 'info')[0]
    info = pvgo_info(info_omegas('more17'))
    pairs = _extra_pairs(prob)
    band = pvgo.pvgo_marginals_general(**_dev(prob), loss_weight=UNIT, anchor=0, pairs=pairs, info=info, method='band')
    dense = pvgo.pvgo_marginals_general(**_dev(prob), loss_weight=UNIT, anchor=0, pairs=pairs, info=info)
    S = anchored_inverse(0.5 * (A + A.T), 0)
    e_np, e_dense = _worst(band, S), _between(band, dense, S)
    print('more17 with info: band vs numpy %.3e, band vs dense %.3e' % (e_np, e_dense))
    assert e_np <= 1e-9 and e_dense <= 1e-9


@pytest.mark.parametrize('with_reproj', [False, True])
def test_band_on_the_21_frame_problem(cuda, with_reproj):
    """The loop-closure problem of tests/test_dense_marginals_gpu.py against numpy's anchored inverse of gauss_newton_matrix and against
    method='dense', with and without the reprojection factor."""
    from islam_amd import pvgo
    from tests.test_dense_marginals_gpu import LW5, _anchored_inverse, _dev as dev21, _host_matrix, _loop_closure_problem, _reproj
    prob, tr = _loop_closure_problem()
    d = dev21(prob, cuda)
    lw = LW5 if with_reproj else LW
    hip = _reproj(tr, cuda) if with_reproj else None
    pairs = [tuple(l) for l in np.asarray(prob['links']).tolist()] + [(9, 0), (20, 0), (5, 5), (0, 20)]
    for anchor in (0, 10):
        band = pvgo.pvgo_marginals_general(**d, loss_weight=lw, reproj=hip, anchor=anchor, pairs=pairs, method='band')
        dense = pvgo.pvgo_marginals_general(**d, loss_weight=lw, reproj=hip, anchor=anchor, pairs=pairs)
        S = _anchored_inverse(_host_matrix(d, lw, pvgo._reproj_struct(hip, lw, cuda)), 21, anchor)
        e_np, e_dense = _worst(band, S), _between(band, dense, S)
        print('21 frames, reproj=%s, anchor=%d: band vs numpy %.3e, band vs dense %.3e' % (with_reproj, anchor, e_np, e_dense))
        assert e_np <= 1e-9 and e_dense <= 1e-9
        _anchor_is_zero(band)
    if with_reproj:                   # the factor changes the answer (a dropped term would go unnoticed otherwise)
        without = pvgo.pvgo_marginals_general(**d, loss_weight=lw, anchor=10, pairs=pairs, method='band')
        assert not torch.allclose(without.node_cov, band.node_cov, rtol=1e-3, atol=0)


def test_f65_against_dense_and_information_monotonicity(cuda):
    """65 frames with the closures (0, 64), (10, 50), (33, 3) added: band against dense, and against the same chain without the closures
    (there the band path has no correction to make): added factors add a positive semi-definite term to A, so no eigenvalue of
    Sigma_without,kk - Sigma_with,kk lies below -1e-9 |Sigma_without,kk|."""
    from islam_amd import pvgo
    prob = _f65()
    band = pvgo.pvgo_marginals_general(**_dev(prob), loss_weight=LW, method='band')
    dense = pvgo.pvgo_marginals_general(**_dev(prob), loss_weight=LW)
    S = np.zeros((585, 585))
    for k in range(65):
        S[9 * k:9 * k + 9, 9 * k:9 * k + 9] = dense.node_cov[k].cpu().numpy()
    for p, (a, b) in enumerate(dense.pairs.cpu().tolist()):                       # the column scale from the blocks the dense path returned
        S[9 * a:9 * a + 9, 9 * b:9 * b + 9] = dense.pair_cov[p].cpu().numpy()
    e = _between(band, dense, S)
    print('F=65, 3 closures: band vs dense %.3e of the column scale' % e)
    assert e <= 1e-9
    without = pvgo.pvgo_marginals_general(**_dev(_f65(False)), loss_weight=LW, method='band').node_cov.cpu().numpy()
    Sw = band.node_cov.cpu().numpy()
    gain = 0.0
    for k in range(65):
        D = without[k] - Sw[k]
        ev = np.linalg.eigvalsh(0.5 * (D + D.T))
        scale = np.linalg.norm(without[k], 2)
        assert ev.min() >= -1e-9 * scale, (k, ev.min(), scale)
        gain = max(gain, ev.max() / max(scale, 1e-300))
    assert gain > 1e-3                                      # and the closures do pull the uncertainty down


# ------------------------------------------------------------------------------------------------------------------ surface
def _run(prob, **kw):
    from islam_amd import lietensor as pp
    from islam_amd.pvgo import run_pvgo
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    return run_pvgo(pp.SE3(t(prob['init_nodes'])), t(prob['init_vels']), pp.SE3(t(prob['vo_motions']).to('cuda')), torch.tensor(prob['links']),
                    t(prob['dts']), pp.SO3(t(prob['imu_drots'])), t(prob['imu_dtrans']), t(prob['imu_dvels']), device='cuda', loss_weight=LW,
                    **kw)


def _plain(x):
    from islam_amd import lietensor as pp
    return pp._plain(x).detach().cpu()


@pytest.mark.parametrize('how', ['auto', 'band_pcg', 'dense_hip'])
def test_run_pvgo_band_marginals(cuda, how):
    from islam_amd import pvgo
    prob = case('more17')
    base = _run(prob, general_solver=how)
    out = _run(prob, general_solver=how, marginals='band')
    assert len(out) == len(base) + 1
    for a, b in zip(base[:4], out[:4]):
        assert torch.equal(_plain(a), _plain(b))
    mg = out[-1]
    assert isinstance(mg, pvgo.PvgoGraphMarginals) and mg.method == 'band' and mg.anchor == 0
    assert mg.pairs.cpu().tolist() == prob['links'].tolist() and mg.node_cov.shape == (17, 9, 9) and mg.pair_cov.shape == (21, 9, 9)
    d = _dev(prob)
    d['nodes'], d['vels'] = _plain(out[2]).to('cuda', torch.float64), out[3].to('cuda', torch.float64)
    ref = pvgo.pvgo_marginals_general(**d, loss_weight=LW, method='band')
    assert torch.equal(ref.node_cov, mg.node_cov) and torch.equal(ref.pair_cov, mg.pair_cov)


def test_run_pvgo_band_marginals_on_a_chain_and_refusals(cuda, monkeypatch):
    from islam_amd import ops, pvgo
    from islam_amd._lib import IslamHipError
    from islam_amd.robust import Huber
    chain = closure_graph(17, ())
    a, b = _run(chain, marginals=True)[-1], _run(chain, marginals='band')[-1]
    assert isinstance(b, pvgo.PvgoMarginals) and torch.equal(a.node_cov, b.node_cov) and torch.equal(a.cross, b.cross)
    with pytest.raises(NotImplementedError):
        _run(case('more17'), marginals='band', kernel=Huber(0.1))
    with pytest.raises(ValueError):
        _run(case('more17'), marginals='nope')
    # the negative information scalar of tests/test_dense_marginals_gpu.py::test_indefinite_matrix_raises
    info = (1.0, -0.5, 100.0, 0.01)
    real = ops.pvgo_build_normal
    monkeypatch.setattr(ops, 'pvgo_build_normal', lambda lin, dts, N, w, *a, **kw: real(lin, dts, N, (0.0, info[1], info[2], info[3]), *a, **kw))
    with pytest.raises(IslamHipError) as e:
        pvgo.pvgo_marginals_general(**_dev(case('more17')), loss_weight=LW, method='band')
    assert e.value.code == ENOTPD and 'not positive definite' in str(e.value)


# ------------------------------------------------------------------------------------------------------------------ long graph
def test_long_graph_without_a_dense_matrix(cuda):
    """The 3000-frame, six-closure graph of tests/test_surface_gpu.py at its initial state."""
    from islam_amd import pvgo
    from tests.test_surface_gpu import _loop_closure_problem
    F = 3000
    closures = {100: (0, 2900), 700: (350, 2100), 1300: (1299, 40), 1900: (2500, 600), 2400: (10, 1500), 2800: (2999, 1)}
    d = _dev(_loop_closure_problem(F, closures, seed=9))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    mg = pvgo.pvgo_marginals_general(**d, loss_weight=LW, pairs=[(350, 2100), (2100, 350)], method='band')
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print('N=3000, 6 closures: peak device memory %.1f MB (a dense matrix: %.0f MB)' % (peak / 1e6, (9 * F) ** 2 * 8 / 1e6))
    assert peak < 0.1 * (9 * F) ** 2 * 8
    assert torch.isfinite(mg.node_cov).all() and torch.isfinite(mg.pair_cov).all()
    assert (torch.diagonal(mg.node_cov[1:], dim1=1, dim2=2) > 0).all() and (torch.diagonal(mg.node_cov[0], 0)[6:] > 0).all()
    ab, ba = mg.pair_cov[0], mg.pair_cov[1].t()
    assert float((ab - ba).abs().max()) <= 1e-12 * float(ab.abs().max())
