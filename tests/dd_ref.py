"""A reference for symmetric positive definite solves that is far more accurate than float64: iterative refinement in which the
residual and the solution are held in double-double (an unevaluated sum of two float64, about 106 bits).  Tests only; numpy + scipy.

    x0 = LAPACK's float64 Cholesky solve of A x = b                      (the case's float64 floor is |x0 - x| / scale)
    r  = b - A (x_hi + x_lo)    in double-double (two_prod of every product, double-double accumulation)
    d  = LAPACK solve of A d = r,   (x_hi, x_lo) += d
    until max|d| <= STOP * (largest entry of the column of x0); at most MAX_ITER rounds, else ArithmeticError.

Nothing here depends on a fused multiply-add: two_prod uses the Veltkamp split (2^27 + 1).  np.longdouble is no substitute: with an
80-bit residual the refinement of the PVGO matrices stalls at 1e-14 ... 1e-12 of the column scale.

Two layouts, one core.  Every matrix is turned into rows of (column index, value) pairs padded to the longest row; a padded entry
has value 0 and contributes an exact 0.  Entries that fall on the same (row, column) stay separate terms of the sum, so nothing is
rounded while the matrix is put together.

    refine_band(Hd, Ho, B, extra=(), anchor=None, damping=0.0)   the block-tridiagonal pair of the chain solver
    refine_dense(A, B, anchor=None)                               a dense symmetric matrix read from its upper triangle

Both return (x_hi, x_lo, x0), each of the shape of B, rows of the anchor's pose DoF zero; the tuple's ``history`` attribute lists the
size of every correction over the column scale."""
import numpy as np
import scipy.linalg as sla

SPLITTER = 134217729.0            # 2^27 + 1
STOP = 1e-22
MAX_ITER = 6


# ------------------------------------------------------------------------------------------------------------------ arithmetic
def two_sum(a, b):
    """s + e = a + b exactly, s = fl(a + b)"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fast_two_sum(a, b):
    """two_sum for |a| >= |b| (or a = 0)"""
    s = a + b
    return s, b - (s - a)


def split(a):
    """a = hi + lo with 26 significant bits each (Veltkamp)"""
    t = SPLITTER * a
    hi = t - (t - a)
    return hi, a - hi


def two_prod(a, b):
    """p + e = a * b exactly, p = fl(a * b) (Dekker; no overflow or underflow assumed)"""
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def dd_add(ah, al, bh, bl):
    """(ah + al) + (bh + bl) as a normalised double-double, relative error about 2^-105"""
    s, e = two_sum(ah, bh)
    t, f = two_sum(al, bl)
    s, e = fast_two_sum(s, e + t)
    return fast_two_sum(s, e + f)


# ------------------------------------------------------------------------------------------------------------------ the matrix as rows
class _Rows:
    """A = sum of the triplets (row, col, hi + lo), stored row by row, padded to the longest row."""

    def __init__(self, n, rows, cols, hi, lo=None):
        rows, cols, hi = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(hi, np.float64)
        lo = np.zeros_like(hi) if lo is None else np.asarray(lo, np.float64)
        nz = (hi != 0.0) | (lo != 0.0)
        rows, cols, hi, lo = rows[nz], cols[nz], hi[nz], lo[nz]
        order = np.argsort(rows, kind='stable')
        rows, cols, hi, lo = rows[order], cols[order], hi[order], lo[order]
        count = np.bincount(rows, minlength=n)
        start = np.concatenate([[0], np.cumsum(count)[:-1]])
        pos = np.arange(rows.size) - start[rows]
        width = int(count.max()) if rows.size else 0
        self.n, self.width = n, width
        self.idx = np.zeros((n, width), dtype=np.int64)
        self.hi = np.zeros((n, width))
        self.lo = np.zeros((n, width))
        self.idx[rows, pos], self.hi[rows, pos], self.lo[rows, pos] = cols, hi, lo
        self.has_lo = bool(np.any(lo != 0.0))

    def residual(self, B, xh, xl):
        """B - A (xh + xl) in double-double, returned rounded to float64 (it is tiny; the solve that follows is float64 anyway)"""
        rh, rl = B.copy(), np.zeros_like(B)
        for t in range(self.width):
            j = self.idx[:, t]
            a = self.hi[:, t, None]
            gh, gl = xh[j], xl[j]
            p, e = two_prod(a, gh)
            e = e + a * gl
            if self.has_lo:
                e = e + self.lo[:, t, None] * gh
            rh, rl = dd_add(rh, rl, -p, -e)
        return rh + rl


def _refine(rows, solve, B):
    x0 = solve(B)
    scale = np.maximum(np.abs(x0).max(axis=0), 1e-300)
    xh, xl = x0.copy(), np.zeros_like(x0)
    history = []
    for _ in range(MAX_ITER):
        d = solve(rows.residual(B, xh, xl))
        xh, xl = dd_add(xh, xl, d, np.zeros_like(d))
        history.append(float(np.max(np.abs(d).max(axis=0) / scale)))
        if history[-1] <= STOP:
            return xh, xl, x0, history
    raise ArithmeticError('double-double refinement did not reach %g of the column scale in %d rounds: corrections %s'
                          % (STOP, MAX_ITER, ' -> '.join('%.1e' % h for h in history)))


def _keep(n, anchor):
    keep = np.ones(n, dtype=bool)
    if anchor is not None:
        keep[9 * anchor:9 * anchor + 6] = False
    return keep


def _reduced(n, keep, rows, cols, *vals):
    """the triplets with the dropped rows / columns taken out and the rest renumbered"""
    new = np.cumsum(keep) - 1
    m = keep[rows] & keep[cols]
    return (int(keep.sum()), new[rows[m]], new[cols[m]]) + tuple(v[m] for v in vals)


class Refined(tuple):
    """(x_hi, x_lo, x0) with the corrections' sizes in ``history``"""
    history = ()


def _expand(keep, B, parts, history):
    out = []
    for p in parts:
        full = np.zeros_like(B)
        full[keep] = p
        out.append(full)
    out = Refined(out)
    out.history = tuple(history)
    return out


# ------------------------------------------------------------------------------------------------------------------ the two layouts
def band_triplets(Hd, Ho, extra=()):
    """(rows, cols, values) of the symmetric matrix with diagonal blocks Hd[k] (read from their upper triangles), blocks Ho[k] at
    (k, k + 1) and S at (i, j) for every (i, j, S) of ``extra`` (9 x 9, or 6 x 6 on the pose DoF), each with its transpose."""
    Hd, Ho = np.asarray(Hd, np.float64), np.asarray(Ho, np.float64)
    N = Hd.shape[0]
    k, r, c = np.meshgrid(np.arange(N), np.arange(9), np.arange(9), indexing='ij')
    up = r <= c
    Hs = np.where(up, Hd, Hd.transpose(0, 2, 1))
    R, C, V = [(9 * k + r).ravel()], [(9 * k + c).ravel()], [Hs.ravel()]
    if N > 1:
        k, r, c = k[:N - 1], r[:N - 1], c[:N - 1]
        o = Ho[:N - 1].ravel()
        R += [(9 * k + r).ravel(), (9 * k + 9 + c).ravel()]
        C += [(9 * k + 9 + c).ravel(), (9 * k + r).ravel()]
        V += [o, o]
    for (i, j, S) in extra:
        S = np.asarray(S, np.float64)
        assert i != j and S.shape[0] == S.shape[1]
        r, c = np.meshgrid(np.arange(S.shape[0]), np.arange(S.shape[0]), indexing='ij')
        R += [(9 * i + r).ravel(), (9 * j + c).ravel()]
        C += [(9 * j + c).ravel(), (9 * i + r).ravel()]
        V += [S.ravel(), S.ravel()]
    return np.concatenate(R), np.concatenate(C), np.concatenate(V)


def refine_band(Hd, Ho, B, extra=(), anchor=None, damping=0.0):
    """Solve A X = B for A = the block-tridiagonal (Hd, Ho) plus the off-band blocks ``extra``, the six pose DoF of node ``anchor``
    taken out, the diagonal multiplied by (1 + damping) -- exactly, as a double-double; LAPACK sees it rounded.
    Preconditioner: scipy.linalg.cholesky_banded (with ``extra``: the dense Cholesky factor).  Returns (x_hi, x_lo, x0)."""
    B = np.asarray(B, np.float64)
    B = B.reshape(B.shape[0], -1)
    n = B.shape[0]
    rows, cols, hi = band_triplets(Hd, Ho, extra)
    lo = np.zeros_like(hi)
    if damping:
        diag = rows == cols
        p, e = two_prod(hi[diag], np.float64(damping))                  # v + v * damping with the damping as given, not fl(1 + damping)
        hi[diag], lo[diag] = dd_add(hi[diag], np.zeros_like(p), p, e)
    keep = _keep(n, anchor)
    m, rows, cols, hi, lo = _reduced(n, keep, rows, cols, hi, lo)
    A = _Rows(m, rows, cols, hi, lo)
    if len(extra):
        D = np.zeros((m, m))
        np.add.at(D, (rows, cols), hi)
        fac = sla.cho_factor(D, lower=True)
        solve = lambda b: sla.cho_solve(fac, b)
    else:
        low = rows >= cols
        ab = np.zeros((int((rows - cols).max()) + 1, m))
        np.add.at(ab, (rows[low] - cols[low], cols[low]), hi[low])
        cb = sla.cholesky_banded(ab, lower=True)
        solve = lambda b: sla.cho_solve_banded((cb, True), b)
    xh, xl, x0, history = _refine(A, solve, B[keep])
    return _expand(keep, B, (xh, xl, x0), history)


def refine_dense(A, B, anchor=None):
    """Solve A X = B for the symmetric matrix that the upper triangle of A (diagonal included) stands for, the six pose DoF of node
    ``anchor`` taken out.  Preconditioner: scipy.linalg.cho_factor.  Returns (x_hi, x_lo, x0)."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    B = B.reshape(B.shape[0], -1)
    n = A.shape[0]
    r, c = np.nonzero(np.triu(A))
    v = A[r, c]
    off = r != c
    rows, cols, hi = np.concatenate([r, c[off]]), np.concatenate([c, r[off]]), np.concatenate([v, v[off]])
    keep = _keep(n, anchor)
    m, rows, cols, hi = _reduced(n, keep, rows, cols, hi)
    S = np.triu(A) + np.triu(A, 1).T
    fac = sla.cho_factor(S[np.ix_(keep, keep)], lower=True)
    xh, xl, x0, history = _refine(_Rows(m, rows, cols, hi), lambda b: sla.cho_solve(fac, b), B[keep])
    return _expand(keep, B, (xh, xl, x0), history)


def unit_columns(n, cols):
    E = np.zeros((n, len(cols)))
    E[np.asarray(cols, np.int64), np.arange(len(cols))] = 1.0
    return E


# ------------------------------------------------------------------------------------------------------------------ the tolerance rule
FACTOR = 10.0


def rule(err, floor, what, single=False):
    """The tolerance rule of the real-matrix accuracy tests.  err[j], floor[j]: the error of the code under test and of LAPACK's
    float64 solve (x0 above) in column j, each over the largest entry of the reference column.  Required:
        max err <= 10 max floor     and     median err <= 10 median floor        (single column: the first only)
    10 = one decimal order for a second backward-stable elimination of the same matrix in another order; the bound never comes from
    the code under test.  Prints the figures, returns (passed, text)."""
    err, floor = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(floor, np.float64))
    assert err.shape == floor.shape and err.size and np.all(np.isfinite(err)) and np.all(np.isfinite(floor))
    emax, fmax, emed, fmed = err.max(), floor.max(), np.median(err), np.median(floor)
    text = '%s: max err %.3e floor %.3e ratio %.2f' % (what, emax, fmax, emax / fmax)
    ok = emax <= FACTOR * fmax
    if not single:
        text += ' | median err %.3e floor %.3e ratio %.2f' % (emed, fmed, emed / fmed)
        ok = ok and emed <= FACTOR * fmed
    print(text)
    return bool(ok), text
