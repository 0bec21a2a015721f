"""The block-tridiagonal solver, its selected inverse, the dense fp64 Cholesky path and the band (Woodbury) path on REAL anchored PVGO
matrices at F = 200 and F = 513 (condition numbers 1e10 ... 1e12), against the double-double reference of tests/dd_ref.py
(tests/test_dd_ref_cpu.py checks that reference against mpmath).  The random SPD matrices of the other solver tests have a condition
number of a few hundred; np.linalg.inv, the reference of the other real-matrix tests, is itself at their tolerance beyond F = 65.

The reference is always computed from the float64 matrix the device path inverts, read back from the device; assembly is not under
test here.  States: the initial state of chain_problem(F); for F = 200 also the chain's LM solution (for the closure graphs: that same
state, which is a state like any other for them).

Tolerance (dd_ref.rule): nothing is fixed in advance.  err_j = the device's error in checked column j over every block entry the call
returned in that column, relative to the reference column's largest entry; floor_j = the same measure for LAPACK's float64 Cholesky
solve of the same matrix (for the band path: the float64 numpy model of its formula, woodbury_model).  Required:
    max_j err_j <= 10 max_j floor_j     and     median_j err_j <= 10 median_j floor_j.
Every test prints err, floor and their ratio; the measured figures are in DESIGN.md sections 3.9 and 3.21."""
import numpy as np
import pytest
import torch

from tests import dd_ref
from tests.closure_graphs import LW, closure_graph
from tests.test_dd_ref_cpu import CLOSURES, checked_columns, checked_nodes, entry_errors as _errors

pytestmark = pytest.mark.gpu

CASES = [(200, 'initial'), (200, 'solution'), (513, 'initial')]
SEGS = [(0, 0), (7, 5)]
W4 = [float(x) ** 2 for x in LW]


@pytest.fixture(scope='module')
def cache():
    """Matrices read back from the device and their references, built once per matrix and left unchanged by the tests."""
    return {}


def _memo(cache, key, build):
    if key not in cache:
        cache[key] = build()
    return cache[key]


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _state(cache, F, state):
    """(problem with the closures of CLOSURES[F], nodes, vels) -- the chain is the same problem without its last len(CLOSURES[F]) links"""
    def build():
        from islam_amd import ops
        prob = closure_graph(F, CLOSURES[F])
        nodes, vels = _t(prob['init_nodes']), _t(prob['init_vels'])
        if state == 'solution':                      # tests/test_marginals_gpu.py::_solution
            ops.pvgo_run_chain(nodes, vels, _t(prob['vo_motions'][:F - 1]), _t(prob['imu_drots']), _t(prob['imu_dtrans']), _t(prob['imu_dvels']),
                               _t(prob['dts']), ops.pvgo_default_params(LW))
        return prob, nodes, vels
    return _memo(cache, ('state', F, state), build)


def _chain_normal(cache, F, state, clamped):
    """Hd, Ho, rhs of the chain on the device (pvgo_linearize + pvgo_build_normal; clamped: its defaults, else vmin = 0, vmax = inf as
    pvgo._marginals_at builds them) and their host copies."""
    def build():
        from islam_amd import ops
        prob, nodes, vels = _state(cache, F, state)
        dts = _t(prob['dts']).reshape(-1)
        lin, _ = ops.pvgo_linearize(nodes, vels, _t(prob['vo_motions'][:F - 1]), _t(prob['imu_drots']), _t(prob['imu_dtrans']), _t(prob['imu_dvels']), dts)
        kw = {} if clamped else dict(vmin=0.0, vmax=float('inf'))
        Hd, Ho, rhs = ops.pvgo_build_normal(lin, dts, F, W4, **kw)
        return dict(Hd=Hd, Ho=Ho, rhs=rhs, hd=Hd.cpu().numpy(), ho=Ho.cpu().numpy(), g=rhs.cpu().numpy())
    return _memo(cache, ('normal', F, state, clamped), build)


def _boundaries(N):
    """the level-0 segment boundaries m0 - 1, m0, m0 + 1 of both segmentations"""
    from islam_amd import ops
    out = set()
    for seg in SEGS:
        m0 = ops.pvgo_marginals_plan(N, seg)[0][1]
        out |= {m0 - 1, m0, m0 + 1}
    return out


def _report(err, floor, what, single=False):
    ok, text = dd_ref.rule(err, floor, what, single)
    assert ok, text


# ------------------------------------------------------------------------------------------------------------------ a. chain selected inverse
def _chain_reference(cache, F, state, anchor):
    def build():
        c = _chain_normal(cache, F, state, False)
        cols = checked_columns(checked_nodes(F, anchor, boundaries=_boundaries(F)), anchor)
        return cols, dd_ref.refine_band(c['hd'], c['ho'], dd_ref.unit_columns(9 * F, cols), anchor=anchor)
    return _memo(cache, ('chain ref', F, state, anchor), build)


def _tridiagonal_pieces(Sd, So, cols):
    N = Sd.shape[0]
    for q, j in enumerate(cols):
        k, i = divmod(int(j), 9)
        yield q, 9 * k, Sd[k][:, i]
        if k > 0:
            yield q, 9 * k - 9, So[k - 1][:, i]
        if k + 1 < N:
            yield q, 9 * k + 9, So[k][i, :]


@pytest.mark.parametrize('seg', SEGS)
@pytest.mark.parametrize('anchor_at', ['first', 'middle'])
@pytest.mark.parametrize('F,state', CASES)
def test_chain_selected_inverse(cuda, cache, F, state, anchor_at, seg):
    from islam_amd import ops
    anchor = 0 if anchor_at == 'first' else F // 2
    c = _chain_normal(cache, F, state, False)
    cols, (xh, xl, x0) = _chain_reference(cache, F, state, anchor)
    Sd, So = ops.pvgo_marginals(c['Hd'], c['Ho'], anchor=anchor, seg_len=seg)
    assert np.array_equal(c['Hd'].cpu().numpy(), c['hd']) and np.array_equal(c['Ho'].cpu().numpy(), c['ho'])       # inputs untouched
    Sd, So = Sd.cpu().numpy(), So.cpu().numpy()
    assert np.all(Sd[anchor][:6, :] == 0) and np.all(Sd[anchor][:, :6] == 0)
    if anchor > 0:
        assert np.all(So[anchor - 1][:, :6] == 0)
    if anchor < F - 1:
        assert np.all(So[anchor][:6, :] == 0)
    err, floor = _errors(_tridiagonal_pieces(Sd, So, cols), xh, xl, x0)
    _report(err, floor, 'pvgo_marginals F=%d %s anchor=%d seg_len=%s (%d columns)' % (F, state, anchor, seg, cols.size))


# ------------------------------------------------------------------------------------------------------------------ b. the LM's linear solve
@pytest.mark.parametrize('seg', SEGS)
@pytest.mark.parametrize('lam', [1e-4, 1e-6, 2e-8])
@pytest.mark.parametrize('F,state', CASES)
def test_lm_linear_solve(cuda, cache, F, state, lam, seg):
    """islam_pvgo_solve_chain on the clamped, unanchored matrix with its real right-hand side.  The solver damps the diagonal of Hd in
    place (v + v * damping), so the matrix it factored is read back from the array it was given."""
    from islam_amd import ops
    c = _chain_normal(cache, F, state, True)
    Hd = c['Hd'].clone()
    dx = ops.pvgo_solve_chain(Hd, c['Ho'], c['rhs'], lam, seg).cpu().numpy()
    damped = Hd.cpu().numpy()
    diag = np.arange(9)
    want = c['hd'][:, diag, diag] * (1.0 + lam)
    assert np.all(np.abs(damped[:, diag, diag] - want) <= 2 * np.spacing(want))
    off = damped.copy()
    off[:, diag, diag] = c['hd'][:, diag, diag]
    assert np.array_equal(off, c['hd']) and np.array_equal(c['Ho'].cpu().numpy(), c['ho'])
    xh, xl, x0 = _memo(cache, ('solve ref', F, state, lam, damped.tobytes()),
                       lambda: dd_ref.refine_band(damped, c['ho'], c['g'].reshape(-1, 1)))
    err, floor = _errors([(0, 0, dx.reshape(-1))], xh, xl, x0)
    _report(err, floor, 'pvgo_solve_chain F=%d %s damping=%g seg_len=%s' % (F, state, lam, seg), single=True)


# ------------------------------------------------------------------------------------------------------------------ c, d. closure graphs
def _graph(cache, F, state):
    """The closure graph on the device, the matrix the dense path factors (gauss_newton_matrix, read back), the requested pairs, the
    checked columns and their reference."""
    def build():
        from tests.test_dense_marginals_gpu import _host_matrix
        prob, nodes, vels = _state(cache, F, state)
        d = dict(nodes=nodes, vels=vels, vo_motions=_t(prob['vo_motions']), links=torch.tensor(prob['links'], dtype=torch.int64, device='cuda'),
                 dts=_t(prob['dts']), imu_drots=_t(prob['imu_drots']), imu_dtrans=_t(prob['imu_dtrans']), imu_dvels=_t(prob['imu_dvels']))
        A = _host_matrix(d, LW)
        pairs = [tuple(l) for l in np.asarray(prob['links']).tolist()] + [(F - 1, 0), (0, F - 1), (F // 2, 0)]
        cols = checked_columns(checked_nodes(F, 0, CLOSURES[F]), 0)
        return dict(d=d, A=A, pairs=pairs, cols=cols, ref=dd_ref.refine_dense(A, dd_ref.unit_columns(9 * F, cols), anchor=0), links=prob['links'])
    return _memo(cache, ('graph', F, state), build)


def _graph_pieces(mg, cols):
    node, pair, pairs = mg.node_cov.cpu().numpy(), mg.pair_cov.cpu().numpy(), mg.pairs.cpu().numpy()
    for q, j in enumerate(cols):
        k, i = divmod(int(j), 9)
        yield q, 9 * k, node[k][:, i]
        for p in np.nonzero(pairs[:, 1] == k)[0]:                  # block (a, k): rows of node a, column i
            yield q, 9 * int(pairs[p, 0]), pair[p][:, i]
        for p in np.nonzero(pairs[:, 0] == k)[0]:                  # block (k, b): by symmetry row i holds column j at the rows of node b
            yield q, 9 * int(pairs[p, 1]), pair[p][i, :]


def _graph_errors(cache, F, state, method):
    def build():
        from islam_amd import pvgo
        g = _graph(cache, F, state)
        mg = pvgo.pvgo_marginals_general(**g['d'], loss_weight=LW, anchor=0, pairs=g['pairs'], method=method)
        assert mg.method == method and not mg.node_cov[0][:6, :].any() and not mg.node_cov[0][:, :6].any()
        xh, xl, x0 = g['ref']
        return mg, _errors(_graph_pieces(mg, g['cols']), xh, xl, x0)
    return _memo(cache, ('graph errors', F, state, method), build)


@pytest.mark.parametrize('F,state', CASES)
def test_dense_path(cuda, cache, F, state):
    """n = 1800 and 4617: also the first real-matrix, multi-tile sizes of the fp64 MFMA Cholesky, its in-place inverse and
    pvgo_dense_cov_blocks."""
    _, (err, floor) = _graph_errors(cache, F, state, 'dense')
    _report(err, floor, "method='dense' F=%d + %d closures, %s (%d columns)" % (F, len(CLOSURES[F]), state, err.size))


@pytest.mark.parametrize('F,state', CASES)
def test_band_path(cuda, cache, F, state):
    """The floor is the formula's own: woodbury_model (float64 numpy) of the same matrix against the same reference, over the same
    entries."""
    from islam_amd.pvgo_dense import band_columns
    from tests.test_band_marginals_cpu import woodbury_model
    g = _graph(cache, F, state)
    mg, (err, _) = _graph_errors(cache, F, state, 'band')
    _, (err_dense, floor_dense) = _graph_errors(cache, F, state, 'dense')
    bc, Rc = band_columns(F, g['links'], 0, np.asarray(g['pairs']))
    model = woodbury_model(g['A'], F, bc, Rc, 0)[:, g['cols']]
    xh, xl, _ = g['ref']
    _, floor = _errors(_graph_pieces(mg, g['cols']), xh, xl, model)
    print("F=%d + %d closures, %s: band err max %.3e | dense err max %.3e | LAPACK Cholesky floor max %.3e | Woodbury model floor max %.3e"
          % (F, len(CLOSURES[F]), state, err.max(), err_dense.max(), floor_dense.max(), floor.max()))
    _report(err, floor, "method='band' F=%d + %d closures, %s (%d columns)" % (F, len(CLOSURES[F]), state, err.size))


# ------------------------------------------------------------------------------------------------------------------ e. column solves
def test_band_inverse_columns(cuda, cache):
    """islam_pvgo_band_inverse_columns on the band of the F = 513 closure graph (anchor 0) at the pose columns of the closure ends:
    every entry of every column against the band-layout reference."""
    from islam_amd import ops
    from islam_amd.pvgo_dense import band_columns
    from tests.test_band_marginals_gpu import _band
    F = 513
    prob = closure_graph(F, CLOSURES[F])
    Hd, Ho, _ = _band(prob)
    bc, Rc = band_columns(F, prob['links'], 0, prob['links'])
    cols = bc[:Rc]
    assert Rc == 6 * 11                                                    # twelve distinct closure ends, node 0 is the anchor
    hd, ho = Hd.cpu().numpy(), Ho.cpu().numpy()
    status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    Y = ops.pvgo_band_inverse_columns(Hd, Ho, cols, 0, status=status)
    assert int(status.item()) == 0 and Y.shape == (9 * F, Rc)
    assert np.array_equal(Hd.cpu().numpy(), hd) and np.array_equal(Ho.cpu().numpy(), ho)
    Y = Y.cpu().numpy()
    assert not Y[:6].any()
    xh, xl, x0 = dd_ref.refine_band(hd, ho, dd_ref.unit_columns(9 * F, cols), anchor=0)
    err, floor = _errors([(q, 0, Y[:, q]) for q in range(Rc)], xh, xl, x0)
    _report(err, floor, 'pvgo_band_inverse_columns F=513 anchor=0 (%d columns)' % Rc)
