"""CPU tests of the in-place inverse of the dense Cholesky factor and the covariance blocks (islam_dense_chol_invert_factor,
islam_pvgo_dense_cov_blocks, csrc/dense_inverse.hip): a numpy model of the blocked in-place algorithm against
LAPACK's dtrtri, the exact-integer construction the GPU test relies on, host-side argument validation, workspace sizes, the kernels'
metadata and the call surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

SYMBOLS = ('islam_dense_chol_inverse_workspace_bytes', 'islam_dense_chol_invert_factor', 'islam_pvgo_dense_cov_blocks')
SIZES = (18, 63, 72, 135, 261, 585)
CONDS = (1e2, 1e8)
U = 2.0 ** -53
NB = 64


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def spd_matrix(n, cond, seed=0):
    """The generator of tests/test_dense_chol_gpu.py: A = Q diag(s) Q^T, s log-spaced from 1 down to 1 / cond; symmetrised."""
    rng = np.random.default_rng(1000 * seed + n)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    s = np.logspace(0, -np.log10(cond), n)
    A = (Q * s) @ Q.T
    return 0.5 * (A + A.T)


def diag_block_inverse(Ljj):
    """trinv_diag_kernel: columns descending, w_cc = 1 / l_cc, w_rc = -(sum_{k = c+1..r} w_rk l_kc) / l_cc; column c still holds L when it is
    read, the columns right of it already hold W."""
    x = np.tril(Ljj).copy()
    jb = x.shape[0]
    for c in range(jb - 1, -1, -1):
        d = x[c, c]
        s = x[:, c + 1:] @ x[c + 1:, c]                     # w_rk = 0 for k > r
        col = -s / d
        col[c] = 1.0 / d
        col[:c] = 0.0
        x[:, c] = col
    return x


def blocked_inverse_model(M, nb=NB):
    """islam_dense_chol_invert_factor on a copy of M: L in the lower triangle and diagonal -> W = L^-1 there.  Whatever the strict upper
    triangle holds (NaN in these tests) is neither written nor used: every read of a block that reaches above the diagonal goes through
    a mask.  Block columns descending; a: W_jj, b: T = -L[c1:, j] W_jj, c: W[c1:, j] = tril(W[c1:, c1:]) T."""
    A = M.copy()
    n = A.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    for j in range((n + nb - 1) // nb - 1, -1, -1):
        c0, c1 = j * nb, min(j * nb + nb, n)
        Wjj = diag_block_inverse(np.where(low[c0:c1, c0:c1], A[c0:c1, c0:c1], 0.0))
        if c1 < n:
            T = -(A[c1:, c0:c1] @ Wjj)
            W22 = np.where(low[c1:, c1:], A[c1:, c1:], 0.0)
            A[c1:, c0:c1] = W22 @ T
        A[c0:c1, c0:c1] = np.where(low[c0:c1, c0:c1], Wjj, A[c0:c1, c0:c1])
    return A


def exact_integer_factor(n=135, seed=7):
    """L = D (I - M): D powers of two in [1/4, 4], M block-nilpotent of index 3 (entries in {-2..2} in the blocks rows [37,90) x cols [0,37),
    rows [90,135) x cols [37,90), rows [90,135) x cols [0,37)), so that L^-1 = (I + M + M^2) D^-1 exactly.  Returns (L, W_exact)."""
    assert n == 135
    rng = np.random.default_rng(seed)
    D = 2.0 ** rng.integers(-2, 3, n)
    M = np.zeros((n, n))
    M[37:90, 0:37] = rng.integers(-2, 3, (53, 37))
    M[90:135, 37:90] = rng.integers(-2, 3, (45, 53))
    M[90:135, 0:37] = rng.integers(-2, 3, (45, 37))
    assert not (M @ M @ M).any()
    L = D[:, None] * (np.eye(n) - M)
    W = (np.eye(n) + M + M @ M) / D[None, :]
    return L, W


def with_nan_upper(L):
    return np.tril(L) + np.triu(np.full_like(L, np.nan), 1)


@pytest.mark.parametrize('cond', CONDS)
@pytest.mark.parametrize('n', SIZES)
def test_blocked_inverse_model_against_dtrtri(n, cond):
    """Forward error of a computed triangular inverse: |W - L^-1| <= c n u kappa(L) |L^-1| in norm (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., section 14.2) for the blocked method and for LAPACK's alike; kappa_2(L) = sqrt(cond).  Both sides
    carry that error, hence the factor 2; c = 4 covers the constants of both methods."""
    from scipy.linalg.lapack import dtrtri
    L = np.linalg.cholesky(spd_matrix(n, cond))
    ref, info = dtrtri(L, lower=1)
    assert info == 0
    out = blocked_inverse_model(with_nan_upper(L))
    iu = np.triu_indices(n, 1)
    assert np.isnan(out[iu]).all()                                      # never written
    W = np.tril(out)
    assert np.isfinite(W).all()                                         # never read as data
    err = np.linalg.norm(W - ref) / np.linalg.norm(ref)
    bound = 2 * 4 * n * U * np.sqrt(cond)
    print('n=%d cond=%g: |W - dtrtri| / |dtrtri| = %.3g (bound %.3g)' % (n, cond, err, bound))
    assert err <= bound


def test_exact_integer_construction():
    """The construction of tests/test_dense_marginals_gpu.py::test_exact_integer_inverse is exact in float64: L W = I as arrays, every
    entry and every partial sum far below 2^53, and the blocked model returns W to the bit."""
    L, W = exact_integer_factor()
    n = L.shape[0]
    assert np.array_equal(L, np.tril(L)) and np.array_equal(W, np.tril(W))
    assert np.array_equal(L @ W, np.eye(n)) and np.array_equal(W @ L, np.eye(n))
    assert np.array_equal(W * 4, np.round(W * 4)) and np.array_equal(L * 4, np.round(L * 4))      # multiples of 1/4 ...
    assert np.abs(W).max() < 2 ** 10 and (np.abs(L) @ np.abs(W)).max() * 16 < 2.0 ** 53          # ... whose sums of products stay exact
    out = blocked_inverse_model(with_nan_upper(L))
    assert np.array_equal(np.tril(out), W)
    assert np.isnan(out[np.triu_indices(n, 1)]).all()


def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib, ops, pvgo, pvgo_dense
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
        assert hasattr(lib._cdll, s), 'libislam_hip.so does not export %s' % s
    assert callable(ops.dense_chol_invert_factor) and callable(ops.dense_chol_inverse_workspace) and callable(ops.pvgo_dense_cov_blocks)
    assert callable(pvgo_dense.marginals_dense) and callable(pvgo.pvgo_marginals_general)
    assert {'node_cov', 'pairs', 'pair_cov', 'anchor'} <= set(vars(pvgo.PvgoGraphMarginals(1, 2, 3, 4)))


def test_workspace_bytes(lib):
    f = lib.islam_dense_chol_inverse_workspace_bytes
    assert f(0) == 0 and f(-5) == 0
    prev = 0
    for n in (1, 9, 18, 63, 64, 65, 585, 2313, 18441, 45009, 108000):
        b = f(n)
        assert b >= 64 * n * 8 and b >= prev                # the 64 x n panel
        assert b <= 64 * n * 8 + 256                        # and nothing like a second matrix
        prev = b


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    big = ctypes.c_size_t(1 << 20)

    def bad(name, args):
        assert getattr(lib, name)(*args) == -1         # ISLAM_EARG
        assert name.encode() in lib.islam_last_error()

    # L, n, workspace, workspace_bytes, stream
    good = [one, 18, one, big, None]
    for k in (0, 2):
        a = list(good)
        a[k] = None
        bad('islam_dense_chol_invert_factor', a)
    for n in (0, -1):
        a = list(good)
        a[1] = n
        bad('islam_dense_chol_invert_factor', a)
    a = list(good)
    a[3] = ctypes.c_size_t(lib.islam_dense_chol_inverse_workspace_bytes(18) - 1)
    bad('islam_dense_chol_invert_factor', a)
    # W, n, anchor, pairs (host), P, node_cov, pair_cov, stream
    pairs = np.array([[0, 1], [1, 0]], dtype=np.int64)
    pp = ctypes.c_void_p(pairs.ctypes.data)
    good = [one, 18, 0, pp, 2, one, one, None]
    for n in (0, -9, 17, 19):
        a = list(good)
        a[1] = n
        bad('islam_pvgo_dense_cov_blocks', a)
    a = list(good)
    a[0] = None
    bad('islam_pvgo_dense_cov_blocks', a)
    for anchor in (-2, 2, 100):
        a = list(good)
        a[2] = anchor
        bad('islam_pvgo_dense_cov_blocks', a)
    a = list(good)
    a[3] = None                                             # P > 0 without pairs
    bad('islam_pvgo_dense_cov_blocks', a)
    a = list(good)
    a[4] = -1
    bad('islam_pvgo_dense_cov_blocks', a)
    for wrong in ([[0, 2], [1, 0]], [[0, 1], [-1, 0]], [[2, 2], [0, 0]]):
        w = np.array(wrong, dtype=np.int64)
        a = list(good)
        a[3] = ctypes.c_void_p(w.ctypes.data)
        bad('islam_pvgo_dense_cov_blocks', a)


def test_kernels_use_no_scratch(lib):
    """The kernel metadata as tests/test_codeobj_cpu.py reads it: no private memory and no spilled register in any kernel of the family."""
    from tests.test_codeobj_cpu import READELF, _field, _kernels
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    ks = {k: v for k, v in _kernels().items() if re.search(r'trinv_(diag|panel|update)_kernel|cov_(node|pair)_kernel', k)}
    assert len(ks) == 6, sorted(ks)                       # (the update kernel in its two column splits)
    for name, blk in ks.items():
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, name


def test_surface_without_gpu(lib):
    """Argument checks of the Python layers that need no device, and the RuntimeError every entry point gives on CPU tensors."""
    from islam_amd import ops, pvgo
    A = torch.zeros((18, 18), dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.dense_chol_invert_factor(A)
    with pytest.raises(RuntimeError):
        ops.pvgo_dense_cov_blocks(A)
    z = torch.zeros
    links = torch.tensor([[0, 1], [0, 2], [2, 3]])
    with pytest.raises(RuntimeError):
        pvgo.pvgo_marginals_general(z(4, 7), z(4, 3), z(3, 7), links, z(3), z(3, 4), z(3, 3), z(3, 3))
    args = (z(4, 7), z(4, 3), z(3, 7), links, z(3), z(3, 4), z(3, 3), z(3, 3))
    for how in ('auto', 'dense', 'band_pcg'):               # decided before anything touches the device
        with pytest.raises(pvgo.UnsupportedGraphError, match='dense_hip'):
            pvgo.run_pvgo(*args, device='cuda', general_solver=how, marginals=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError) as e:
            pvgo.run_pvgo(*args, device='cuda', general_solver='dense_hip', marginals=True)
        assert not isinstance(e.value, NotImplementedError)
