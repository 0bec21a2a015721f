"""CPU tests of the marginal covariances of loop-closure graphs from the band form (islam_pvgo_band_inverse_columns,
islam_pvgo_band_cov_blocks, csrc/pvgo_band_cov.inl, pvgo_dense.band_columns / marginals_band): the column
bookkeeping against a plain restatement, the Woodbury formula in numpy against numpy's anchored inverse of the oracle's matrix, host-side
argument validation, the kernels' metadata and the call surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import pvgo as opvgo
from tests.closure_graphs import CASES, LW, case, sizes

SYMBOLS = ('islam_pvgo_band_inverse_workspace_bytes', 'islam_pvgo_band_inverse_columns', 'islam_pvgo_band_cov_blocks')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------ band_columns
def columns_restated(edges, anchor, pairs):
    """The definition, entry by entry: (closure part, extra part) as ascending lists."""
    ends = sorted({int(n) for i, j in edges if abs(int(i) - int(j)) > 1 for n in (i, j)})
    closure = [9 * n + c for n in ends for c in range(6) if n != anchor]
    seconds = sorted({int(b) for a, b in pairs if abs(int(a) - int(b)) > 1})
    extra = [9 * b + c for b in seconds for c in range(9) if not (b == anchor and c < 6) and 9 * b + c not in closure]
    return closure, extra


def check_columns(N, edges, anchor, pairs):
    from islam_amd.pvgo_dense import band_columns
    cols, Rc = band_columns(N, np.asarray(edges, dtype=np.int64).reshape(-1, 2), anchor, np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    closure, extra = columns_restated(edges, anchor, pairs)
    assert cols.dtype == np.int64 and cols.ndim == 1
    assert Rc == len(closure) and cols[:Rc].tolist() == closure and cols[Rc:].tolist() == extra
    assert len(set(cols.tolist())) == cols.size
    return cols, Rc


def test_band_columns_on_the_closure_graphs():
    links = {name: case(name)['links'] for name in CASES}
    # more17: the parallel pair (0, 9) gives one set of columns, (16, 2) counts reversed, the duplicate (3, 4) is not off-band
    cols, Rc = check_columns(17, links['more17'], 0, links['more17'])
    assert Rc == 6 * 5 and sorted(set(cols[:Rc] // 9)) == [2, 4, 9, 15, 16]              # ends {0, 2, 4, 9, 15, 16} less the anchor
    assert cols[Rc:].tolist() == [9 * n + c for n in (2, 9, 15) for c in (6, 7, 8)]     # the far pairs' second nodes: velocities only
    assert check_columns(17, links['more17'], None, links['more17'])[1] == 36          # anchor=None leaves nothing out
    assert check_columns(17, links['fewer17'], 0, links['fewer17'])[1] == 6            # the closure (0, 9) ends at the anchor
    assert check_columns(17, links['fewer17'], 8, links['fewer17'])[1] == 12
    assert check_columns(3, links['n3e1'], 0, links['n3e1'])[1] == 6
    assert check_columns(3, links['n3e4'], 1, links['n3e4'])[1] == 12
    cols, Rc = check_columns(2, links['n2e3'], 0, links['n2e3'])                        # K = 0
    assert Rc == 0 and cols.size == 0


def test_band_columns_far_pairs():
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (0, 4)]
    # a far pair whose second node is the anchor: its three velocity columns only
    cols, Rc = check_columns(7, edges, 0, [(6, 0)])
    assert Rc == 6 and cols.tolist() == [36, 37, 38, 39, 40, 41, 6, 7, 8]
    # a far pair whose second node is a closure end already: it gains the three velocity columns
    cols, Rc = check_columns(7, edges, 0, [(6, 4), (1, 4)])
    assert cols[Rc:].tolist() == [42, 43, 44]
    # a second node that is neither: all nine; adjacent and equal pairs ask for nothing; repeats count once
    cols, Rc = check_columns(7, edges, 3, [(0, 6), (2, 6), (5, 6), (6, 6), (6, 5)])
    assert Rc == 12 and cols[Rc:].tolist() == list(range(54, 63))
    from islam_amd.pvgo_dense import band_columns
    with pytest.raises(ValueError):
        band_columns(7, np.array(edges), 0, np.array([[0, 7]]))


# ------------------------------------------------------------------------------------------------------------------ the formula
def oracle_matrix(name):
    """J^T W J of the oracle's dense Jacobian at the initial state, in the solver's node-major ordering (the construction of
    tests/test_added_edges_gpu.py::_reference_normal)."""
    prob = case(name)
    N, E, M = sizes(name)
    res = opvgo.residuals(prob['init_nodes'], prob['init_vels'], prob['links'], prob['vo_motions'], prob['imu_drots'], prob['imu_dtrans'],
                          prob['imu_dvels'], prob['dts'])
    Ae, Bk = opvgo.jac_blocks(prob['init_nodes'], prob['links'], prob['vo_motions'], prob['imu_drots'], res[0], res[2])
    J10 = opvgo.jacobian_dense(N, prob['links'], Ae, Bk, prob['dts'])
    order = np.concatenate([np.concatenate([7 * k + np.arange(6), 7 * N + 3 * k + np.arange(3)]) for k in range(N)])
    J = J10[:, order]
    A = (J.T * opvgo.weight_vector(E, M, LW, np.float64)) @ J
    return 0.5 * (A + A.T)


def anchored_inverse(A, anchor):
    keep = np.ones(A.shape[0], dtype=bool)
    if anchor is not None:
        keep[9 * anchor:9 * anchor + 6] = False
    idx = np.nonzero(keep)[0]
    S = np.zeros_like(A)
    S[np.ix_(idx, idx)] = np.linalg.inv(A[np.ix_(idx, idx)])
    return S


def woodbury_model(A, N, cols, Rc, anchor):
    """Sigma = B_a^-1 - Y_c G Y_c^T from the band pieces of A and `cols` alone: B the block-tridiagonal part, R = A - B, M = R on the
    closure columns, G = (I + M Y_S)^-1 M symmetrised."""
    blk = np.arange(9 * N) // 9
    band = np.abs(blk[:, None] - blk[None, :]) <= 1
    B, R = np.where(band, A, 0.0), np.where(band, 0.0, A)
    Binv = anchored_inverse(B, anchor)
    cc = cols[:Rc]
    if Rc == 0:
        return Binv
    Yc = Binv[:, cc]
    M = R[np.ix_(cc, cc)]
    G = np.linalg.solve(np.eye(Rc) + M @ Yc[cc, :], M)
    return Binv - Yc @ (0.5 * (G + G.T)) @ Yc.T


@pytest.mark.parametrize('name', sorted(CASES))
def test_woodbury_model_reproduces_the_anchored_inverse(name):
    from islam_amd.pvgo_dense import band_columns
    N = sizes(name)[0]
    A = oracle_matrix(name)
    for anchor in (0, N // 2):
        cols, Rc = band_columns(N, case(name)['links'], anchor, case(name)['links'])
        S = anchored_inverse(A, anchor)
        got = woodbury_model(A, N, cols, Rc, anchor)
        err = np.max(np.abs(got - S) / np.maximum(np.abs(S).max(axis=0), 1e-300)[None, :])
        print('%s anchor=%d: Rc=%d, worst |formula - inverse| / column scale = %.3e' % (name, anchor, Rc, err))
        assert err <= 1e-11


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib, ops, pvgo, pvgo_dense
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
        assert hasattr(lib._cdll, s), 'libislam_hip.so does not export %s' % s
    assert callable(ops.pvgo_band_inverse_columns) and callable(ops.pvgo_band_cov_blocks) and callable(ops.pvgo_band_inverse_workspace)
    assert callable(pvgo_dense.marginals_band) and callable(pvgo_dense.band_columns)
    assert pvgo.PvgoGraphMarginals(1, 2, 3, 4).method == 'dense' and pvgo.PvgoGraphMarginals(1, 2, 3, 4, 'band').method == 'band'
    assert pvgo._BAND_MAX_COLUMN_BYTES == 4 << 30


def test_workspace_bytes(lib):
    f = lib.islam_pvgo_band_inverse_workspace_bytes
    assert f(1, 4) == 0 and f(0, 0) == 0 and f(5, -1) == 0
    solver = lib.islam_pvgo_workspace_bytes
    for N, R in ((2, 0), (3, 6), (17, 33), (3000, 84), (50001, 153)):
        b = f(N, R)
        pad = (R + 15) // 16 * 16
        assert b >= solver(N) - 256 + (2 * 81 + 9 + 9 * pad) * N * 8              # the solver's, the anchored band, a right-hand side, the columns
        assert b <= solver(N) + (2 * 81 + 9 + 9 * pad) * N * 8 + 2048           # O(N R): nothing like a (9N)^2 array


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    big = ctypes.c_size_t(1 << 30)
    host = lambda a: ctypes.c_void_p(a.ctypes.data)

    def bad(name, args):
        assert getattr(lib, name)(*args) == -1         # ISLAM_EARG
        assert name.encode() in lib.islam_last_error()

    def variants(name, good, changes):
        for k, v in changes:
            a = list(good)
            a[k] = v
            bad(name, a)

    cols = np.array([9, 10, 11, 12, 13, 14, 6, 7, 8], dtype=np.int64)       # node 1's pose DoF, then the anchor's velocity
    sl = (ctypes.c_int * 2)(0, 0)
    small = ctypes.c_size_t(lib.islam_pvgo_band_inverse_workspace_bytes(3, 9) - 1)
    # Hd, Ho, N, anchor, cols (host), R, seg_len, workspace, workspace_bytes, Y, ldy, status, stream
    good = [one, one, 3, 0, host(cols), 9, sl, one, big, one, 9, one, None]
    outside = np.array([9, 27], dtype=np.int64)
    anchored = np.array([3, 9], dtype=np.int64)
    variants('islam_pvgo_band_inverse_columns', good,
             [(2, 1), (2, 0), (5, -1), (10, 8), (0, None), (1, None), (4, None), (7, None), (9, None), (8, small), (3, 3), (3, -2),
              (4, host(outside)), (4, host(anchored))])
    pairs = np.array([[0, 1], [2, 0], [1, 1]], dtype=np.int64)
    # Sd, So, Y, ldy, N, anchor, cols, R, Rc, G, ldg, pairs, P, workspace, workspace_bytes, node_cov, pair_cov, status, stream
    good = [one, one, one, 9, 3, 0, host(cols), 9, 6, one, 16, host(pairs), 3, one, big, one, one, one, None]
    velocity_first = np.array([6, 7, 8, 9, 10, 11, 12, 13, 14], dtype=np.int64)
    far_without_columns = np.array([[0, 2], [1, 1], [0, 0]], dtype=np.int64)
    variants('islam_pvgo_band_cov_blocks', good,
             [(4, 1), (7, -1), (3, 8), (8, 10), (8, -1), (0, None), (1, None), (2, None), (6, None), (9, None), (13, None), (10, 15),
              (14, ctypes.c_size_t(3 * 9 * 16 * 8 - 1)), (5, 3), (11, None), (12, -1), (6, host(velocity_first)),
              (11, host(np.array([[0, 3], [1, 1], [0, 0]], dtype=np.int64))), (11, host(far_without_columns))])


def test_kernels_use_no_scratch(lib):
    """The kernel metadata as tests/test_codeobj_cpu.py reads it: no private memory and no spilled register in any kernel of the family."""
    from tests.test_codeobj_cpu import READELF, _field, _kernels
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    ks = {k: v for k, v in _kernels().items() if re.search(r'band_(anchor|rhs|transpose|status|project|node|pair)_kernel', k)}
    assert len(ks) == 7, sorted(ks)
    for name, blk in ks.items():
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, name
        assert _field(blk, 'group_segment_fixed_size') <= 64 << 10, name


def test_surface_without_gpu(lib):
    """Argument checks of the Python layers that need no device, and the RuntimeError every entry point gives on CPU tensors."""
    from islam_amd import ops, pvgo
    z = torch.zeros
    Hd, Ho = z((3, 9, 9), dtype=torch.float64), z((3, 9, 9), dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.pvgo_band_inverse_columns(Hd, Ho, [9, 10])
    with pytest.raises(RuntimeError):
        ops.pvgo_band_cov_blocks(Hd, Ho[:2], z((27, 2), dtype=torch.float64), [9, 10], 0, None)
    links = torch.tensor([[0, 1], [0, 2], [2, 3]])
    args = (z(4, 7), z(4, 3), z(3, 7), links, z(3), z(3, 4), z(3, 3), z(3, 3))
    with pytest.raises(RuntimeError):
        pvgo.pvgo_marginals_general(*args, method='band')
    for how in ('auto', 'dense', 'dense_hip', 'band_pcg'):  # decided before anything touches the device
        with pytest.raises(ValueError, match='marginals'):
            pvgo.run_pvgo(*args, device='cuda', general_solver=how, marginals='nope')
    from islam_amd.robust import Huber
    with pytest.raises(NotImplementedError):
        pvgo.run_pvgo(*args, device='cuda', marginals='band', kernel=Huber(0.1))
    if not torch.cuda.is_available():
        for how in ('auto', 'band_pcg', 'dense_hip'):      # marginals='band' is served with every solver: it gets as far as the device
            with pytest.raises(RuntimeError) as e:
                pvgo.run_pvgo(*args, device='cuda', general_solver=how, marginals='band')
            assert not isinstance(e.value, NotImplementedError)
