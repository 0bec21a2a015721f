"""The double-double reference of tests/dd_ref.py is itself checked here, on the CPU: against mpmath at 60 digits on small real PVGO
matrices; that it converges (within its six rounds) on the matrices the GPU tests of tests/test_real_matrix_accuracy_gpu.py use, with
LAPACK's float64 floors printed; and that the tolerance rule of those tests, fed with these floors, rejects a LAPACK solve of a matrix
in which one 9 x 9 block was scaled by 1 + 1e-10.

The matrices are J^T W J of the oracle's Jacobian at the initial state of chain_problem(F) / closure_graph(F, ...), LW = (1, 0.1, 10,
0.1), in the solver's node-major ordering."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import pvgo as opvgo
from tests import dd_ref
from tests.closure_graphs import LW, closure_graph

CLOSURES = {200: ((0, 199), (20, 150), (100, 3), (60, 180)),
            513: ((0, 512), (40, 400), (300, 7), (128, 256), (500, 100), (250, 260))}
DOFS = (0, 4, 8)


# ------------------------------------------------------------------------------------------------------------------ shared with the GPU tests
def checked_nodes(N, anchor, closures=(), boundaries=()):
    """Nodes 1, 2, N//4, N//2, N-2, N-1, the anchor's neighbours, every closure end and the given segment boundaries."""
    nodes = {1, 2, N // 4, N // 2, N - 2, N - 1} | {n for e in closures for n in e} | set(boundaries)
    if anchor is not None:
        nodes |= {anchor - 1, anchor + 1}
    return sorted(k for k in nodes if 0 <= k < N)


def checked_columns(nodes, anchor):
    """DoF 0, 4, 8 of the nodes, without the anchor's pose DoF (those columns of the covariance are zero)."""
    return np.array([9 * k + i for k in nodes for i in DOFS if not (k == anchor and i < 6)], dtype=np.int64)


def column_error(X, ref_hi, ref_lo, where=None):
    """per column: max |X - (ref_hi + ref_lo)| over the rows ``where`` (all rows by default) / the largest entry of the column"""
    scale = np.maximum(np.abs(ref_hi).max(axis=0), 1e-300)
    D = np.abs((X - ref_hi) - ref_lo)
    if where is not None:
        D = np.where(where, D, 0.0)
    return D.max(axis=0) / scale


def entry_errors(pieces, xh, xl, x0):
    """pieces: (q, first row, values) -- consecutive entries of checked column q that the device returned.  Per column: the largest
    |values - reference| and the largest |x0 - reference| over the same entries, each over the reference column's largest entry."""
    m = xh.shape[1]
    scale = np.abs(xh).max(axis=0)
    err, floor, seen = np.zeros(m), np.zeros(m), np.zeros(m, dtype=bool)
    for q, r0, v in pieces:
        rows = slice(r0, r0 + len(v))
        err[q] = max(err[q], np.abs((np.asarray(v) - xh[rows, q]) - xl[rows, q]).max())
        floor[q] = max(floor[q], np.abs((x0[rows, q] - xh[rows, q]) - xl[rows, q]).max())
        seen[q] = True
    assert seen.all()
    return err / scale, floor / scale


def oracle_system_of(prob):
    """(J^T W J, -J^T W r) of the oracle's dense Jacobian and residuals at the initial state (the construction of
    tests/test_band_marginals_cpu.py::oracle_matrix)."""
    N, E = prob['init_nodes'].shape[0], len(prob['links'])
    res = opvgo.residuals(prob['init_nodes'], prob['init_vels'], prob['links'], prob['vo_motions'], prob['imu_drots'], prob['imu_dtrans'],
                          prob['imu_dvels'], prob['dts'])
    Ae, Bk = opvgo.jac_blocks(prob['init_nodes'], prob['links'], prob['vo_motions'], prob['imu_drots'], res[0], res[2])
    J10 = opvgo.jacobian_dense(N, prob['links'], Ae, Bk, prob['dts'])
    order = np.concatenate([np.concatenate([7 * k + np.arange(6), 7 * N + 3 * k + np.arange(3)]) for k in range(N)])
    J = J10[:, order]
    w = opvgo.weight_vector(E, N - 1, LW, np.float64)
    A = (J.T * w) @ J
    return 0.5 * (A + A.T), -(J.T * w) @ np.concatenate([np.asarray(r, np.float64).ravel() for r in res])


def band_pieces(A):
    """(Hd, Ho, extra) of a symmetric 9N x 9N matrix: its block-tridiagonal part and the non-zero blocks (i, j, S), j > i + 1."""
    N = A.shape[0] // 9
    blk = lambda i, j: A[9 * i:9 * i + 9, 9 * j:9 * j + 9]
    Hd = np.stack([blk(k, k) for k in range(N)])
    Ho = np.stack([blk(k, k + 1) for k in range(N - 1)] + [np.zeros((9, 9))])
    nz = np.abs(A).reshape(N, 9, N, 9).max(axis=(1, 3)) > 0
    extra = [(i, j, blk(i, j).copy()) for i, j in zip(*np.nonzero(np.triu(nz, 2)))]
    return Hd, Ho, extra


@functools.lru_cache(maxsize=None)
def chain_system(F):
    return oracle_system_of(closure_graph(F, ()))


def chain_matrix(F):
    return chain_system(F)[0]


@functools.lru_cache(maxsize=None)
def closure_matrix(F):
    return oracle_system_of(closure_graph(F, CLOSURES[F]))[0]


# ------------------------------------------------------------------------------------------------------------------ against mpmath
def _mp_inverse(A, keep, cols=None):
    """(hi, lo) of the inverse of A[keep][:, keep] from mpmath at 60 digits, zero elsewhere.  cols: only these columns of it (one LU
    factorisation and a solve per column instead of the whole inverse); the others stay zero."""
    import mpmath as mp
    idx = np.nonzero(keep)[0]
    hi, lo = np.zeros(A.shape), np.zeros(A.shape)
    with mp.workdps(60):
        Am = mp.matrix(A[np.ix_(idx, idx)].tolist())
        if cols is None:
            X, at = Am ** -1, idx
        else:
            at = np.asarray(cols)
            LU, perm = mp.mp.LU_decomp(Am)
            X = mp.zeros(idx.size, at.size)
            for b, j in enumerate(at):
                e = mp.zeros(idx.size, 1)
                e[int(np.searchsorted(idx, j))] = 1
                x = mp.mp.U_solve(LU, mp.mp.L_solve(LU, e, perm))
                for a in range(idx.size):
                    X[a, b] = x[a]
        for a, i in enumerate(idx):
            for b, j in enumerate(at):
                h = float(X[a, b])
                hi[i, j], lo[i, j] = h, float(X[a, b] - h)
    return hi, lo


def _against_mp(got, hi, lo, what, bound=1e-25):
    xh, xl, x0 = got
    err = np.abs(((xh - hi) + (xl - lo))).max(axis=0) / np.abs(hi).max(axis=0)
    print('%s: %d rounds (%s), |x_hi + x_lo - mpmath| / column scale = %.2e, float64 floor %.2e'
          % (what, len(got.history), ' -> '.join('%.1e' % h for h in got.history), err.max(), column_error(x0, hi, lo).max()))
    assert err.max() <= bound
    assert np.all(np.abs(xl) <= 2.0 ** -52 * np.abs(xh))                          # a normalised double-double


def test_chain_f9_against_mpmath():
    A = chain_matrix(9)
    Hd, Ho, extra = band_pieces(A)
    assert not extra
    keep = dd_ref._keep(81, 0)
    hi, lo = _mp_inverse(A, keep)
    E = np.eye(81)[:, keep]
    _against_mp(dd_ref.refine_band(Hd, Ho, E, anchor=0), hi[:, keep], lo[:, keep], 'chain F=9, band layout, anchor 0')
    _against_mp(dd_ref.refine_dense(A, E, anchor=0), hi[:, keep], lo[:, keep], 'chain F=9, dense layout, anchor 0')
    assert not dd_ref.refine_band(Hd, Ho, E, anchor=0)[0][:6].any()
    # the LM's solve: unanchored (singular without damping), the diagonal times 1 + 1e-10, the real right-hand side.  The damped diagonal
    # is no float64 number; mpmath gets it exactly.  Bound: this system is some 1e8 times closer to singular than the anchored one, so
    # the 1e-25 of the anchored cases is out of a double-double's reach; what the refinement promises is its stopping size, 1e-22 (the
    # corrections shrink by orders of magnitude per round, so the error left is below the last correction)
    import mpmath as mp
    lam, g = 1e-10, chain_system(9)[1]
    with mp.workdps(60):
        Am = mp.matrix(A.tolist())
        for i in range(81):
            Am[i, i] = mp.mpf(A[i, i]) * (mp.mpf(1.0) + mp.mpf(lam))
        x = mp.lu_solve(Am, mp.matrix(g.tolist()))
        hi = np.array([[float(x[i])] for i in range(81)])
        lo = np.array([[float(x[i] - mp.mpf(hi[i, 0]))] for i in range(81)])
    _against_mp(dd_ref.refine_band(Hd, Ho, g, damping=lam), hi, lo, 'chain F=9, band layout, no anchor, damping 1e-10, real right-hand side',
                bound=dd_ref.STOP)


def test_more17_against_mpmath():
    from tests.test_band_marginals_cpu import oracle_matrix
    A = oracle_matrix('more17')
    Hd, Ho, extra = band_pieces(A)
    assert sorted((i, j) for i, j, _ in extra) == [(0, 9), (2, 16), (4, 15)]
    keep = dd_ref._keep(153, 0)
    cols = checked_columns(checked_nodes(17, 0, ((0, 9), (4, 15), (16, 2))), 0)          # 12 nodes, 34 columns of the inverse
    hi, lo = _mp_inverse(A, keep, cols)
    E = dd_ref.unit_columns(153, cols)
    _against_mp(dd_ref.refine_dense(A, E, anchor=0), hi[:, cols], lo[:, cols], 'more17, dense layout, anchor 0')
    _against_mp(dd_ref.refine_band(Hd, Ho, E, extra=extra, anchor=0), hi[:, cols], lo[:, cols], 'more17, band layout + off-band blocks, anchor 0')
    # the dense layout reads the upper triangle only
    B = A.copy()
    B[np.tril_indices(153, -1)] = np.nan
    again = dd_ref.refine_dense(B, E, anchor=0)
    assert np.array_equal(again[0], dd_ref.refine_dense(A, E, anchor=0)[0])


def test_refinement_that_stalls_raises():
    """A residual that is not accurate enough (here: the matrix of the residual differs from the factored one) must raise, not return."""
    A = chain_matrix(9)
    Hd, Ho, _ = band_pieces(A)
    rows = dd_ref._Rows(81, *dd_ref.band_triplets(Hd, Ho))
    fac = sla.cho_factor(A + 1e-3 * np.diag(np.diag(A)), lower=True)
    with pytest.raises(ArithmeticError):
        dd_ref._refine(rows, lambda b: sla.cho_solve(fac, b) * 0.5, np.eye(81)[:, 6:9])


# ------------------------------------------------------------------------------------------------------------------ floors
@functools.lru_cache(maxsize=None)
def chain_reference(F):
    """The chain matrix anchored at 0, its checked columns and their reference."""
    A = chain_matrix(F)
    Hd, Ho, extra = band_pieces(A)
    assert not extra
    cols = checked_columns(checked_nodes(F, 0), 0)
    return Hd, Ho, cols, dd_ref.refine_band(Hd, Ho, dd_ref.unit_columns(9 * F, cols), anchor=0)


@pytest.mark.parametrize('F', [200, 513])
def test_chain_floors(F):
    Hd, Ho, cols, ref = chain_reference(F)
    xh, xl, x0 = ref
    floor = column_error(x0, xh, xl)
    print('chain F=%d: %d columns, %d rounds (%s); LAPACK banded Cholesky floor max %.2e median %.2e'
          % (F, cols.size, len(ref.history), ' -> '.join('%.1e' % h for h in ref.history), floor.max(), np.median(floor)))
    assert len(ref.history) <= dd_ref.MAX_ITER and ref.history[-1] <= dd_ref.STOP
    # the clamped, unanchored matrix of the LM's solve under its smallest dampings converges too
    rhs = chain_system(F)[1]
    for lam in (1e-4, 2e-8, 1e-10):
        r = dd_ref.refine_band(Hd, Ho, rhs, damping=lam)
        print('chain F=%d, no anchor, damping %g: %d rounds, floor %.2e' % (F, lam, len(r.history), column_error(r[2], r[0], r[1]).max()))
        assert r.history[-1] <= dd_ref.STOP


@pytest.mark.parametrize('F', [200, 513])
def test_closure_graph_floors(F):
    from islam_amd.pvgo_dense import band_columns
    from tests.test_band_marginals_cpu import woodbury_model
    A = closure_matrix(F)
    links = closure_graph(F, CLOSURES[F])['links']
    cols = checked_columns(checked_nodes(F, 0, CLOSURES[F]), 0)
    ref = dd_ref.refine_dense(A, dd_ref.unit_columns(9 * F, cols), anchor=0)
    xh, xl, x0 = ref
    assert ref.history[-1] <= dd_ref.STOP
    keep = dd_ref._keep(9 * F, 0)
    inv = np.zeros_like(A)
    inv[np.ix_(keep, keep)] = np.linalg.inv(A[np.ix_(keep, keep)])
    bc, Rc = band_columns(F, links, 0, links)
    wb = woodbury_model(A, F, bc, Rc, 0)
    f = [column_error(x, xh, xl) for x in (x0, inv[:, cols], wb[:, cols])]
    print('F=%d + %d closures: %d columns, %d rounds; floors max (median): Cholesky solve %.2e (%.2e), np.linalg.inv %.2e (%.2e), '
          'Woodbury model %.2e (%.2e)' % (F, len(CLOSURES[F]), cols.size, len(ref.history), f[0].max(), np.median(f[0]), f[1].max(),
                                         np.median(f[1]), f[2].max(), np.median(f[2])))
    # the band layout with the closures as off-band blocks is the same matrix: the same solution to the last bit of x_hi or so
    Hd, Ho, extra = band_pieces(A)
    assert len(extra) == len(CLOSURES[F])
    if F == 200:
        alt = dd_ref.refine_band(Hd, Ho, dd_ref.unit_columns(9 * F, cols[:6]), extra=extra, anchor=0)
        assert column_error(alt[0], xh[:, :6], xl[:, :6] - alt[1]).max() <= 1e-20


# ------------------------------------------------------------------------------------------------------------------ separation
@pytest.mark.parametrize('F', [200, 513])
def test_rule_rejects_a_block_scaled_by_1e_minus_10(F):
    """LAPACK's solve of the chain matrix with Ho[F // 2] scaled by 1 + 1e-10 -- a relative change of 1e-10 in 81 of the matrix's entries
    -- must fail the rule of the GPU tests; the unperturbed solve passes it, and so must the same float64 Cholesky run from the other end
    of the chain (the "second backward-stable elimination in another order" the factor 10 stands for)."""
    Hd, Ho, cols, ref = chain_reference(F)
    xh, xl, x0 = ref
    floor = column_error(x0, xh, xl)
    keep = dd_ref._keep(9 * F, 0)
    E = dd_ref.unit_columns(9 * F, cols)[keep]

    def banded(Ho_used, lower_only):
        n, r, c, v = dd_ref._reduced(9 * F, keep, *dd_ref.band_triplets(Hd, Ho_used))
        u = int(np.abs(r - c).max())
        if lower_only:
            ab = np.zeros((u + 1, n))
            m = r >= c
            ab[r[m] - c[m], c[m]] = v[m]
            return ab
        ab = np.zeros((2 * u + 1, n))
        ab[u + r - c, c] = v
        return ab, u

    def full(x):
        out = np.zeros((9 * F, cols.size))
        out[keep] = x
        return out

    # the same matrix eliminated from the other end (Cholesky of the reversed ordering) and by LU with partial pivoting
    low = banded(Ho, True)
    n = low.shape[1]
    rev = np.zeros_like(low)
    for d in range(low.shape[0]):
        rev[d, :n - d] = low[d, :n - d][::-1]
    xr = sla.cho_solve_banded((sla.cholesky_banded(rev, lower=True), True), E[::-1])[::-1]
    ok, text = dd_ref.rule(column_error(full(xr), xh, xl), floor, 'chain F=%d, banded Cholesky from the other end' % F)
    ab, u = banded(Ho, False)
    dd_ref.rule(column_error(full(sla.solve_banded((u, u), ab, E)), xh, xl), floor, 'chain F=%d, banded LU (not asserted)' % F)
    assert ok, text
    assert dd_ref.rule(floor, floor, 'chain F=%d, the Cholesky solve itself' % F)[0]
    mutant = Ho.copy()
    mutant[F // 2] *= 1.0 + 1e-10
    xm = full(sla.cho_solve_banded((sla.cholesky_banded(banded(mutant, True), lower=True), True), E))
    err = column_error(xm, xh, xl)
    ok, text = dd_ref.rule(err, floor, 'chain F=%d, Ho[%d] scaled by 1 + 1e-10' % (F, F // 2))
    assert not ok, text
    assert err.max() > dd_ref.FACTOR * floor.max()
    # and under the measure of the GPU tests, which see the entries of the three blocks around the diagonal only
    window = lambda X: [(q, max(9 * (j // 9) - 9, 0), X[max(9 * (j // 9) - 9, 0):9 * (j // 9) + 18, q]) for q, j in enumerate(cols)]
    err, floor = entry_errors(window(xm), xh, xl, x0)
    ok, text = dd_ref.rule(err, floor, 'chain F=%d, Ho[%d] scaled by 1 + 1e-10, block entries' % (F, F // 2))
    assert not ok and err.max() > dd_ref.FACTOR * floor.max(), text
    err, floor = entry_errors(window(full(xr)), xh, xl, x0)
    ok, text = dd_ref.rule(err, floor, 'chain F=%d, banded Cholesky from the other end, block entries' % F)
    assert ok, text
