"""CPU tests of the dense Cholesky (islam_dense_chol_factor / _solve, csrc/dense_chol.hip): the symbols exist,
the workspace hides no second matrix, arguments are validated on the host before any device work, run_pvgo knows 'dense_hip', the
new kernels use no scratch, and a numpy model of the fragment index formulas the update kernel relies on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

SYMBOLS = ('islam_dense_chol_workspace_bytes', 'islam_dense_chol_factor', 'islam_dense_chol_solve')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    from islam_amd import _lib, ops
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES
        assert hasattr(lib._cdll, s), 'libislam_hip.so does not export %s' % s
    assert callable(ops.dense_chol_factor) and callable(ops.dense_chol_solve)


def test_workspace_bytes(lib):
    f = lib.islam_dense_chol_workspace_bytes
    assert f(0) == 0 and f(-5) == 0
    prev = 0
    for n in (1, 9, 18, 63, 64, 65, 585, 2313, 18441, 45009, 108000):
        b = f(n)
        assert b >= prev and b > 0
        prev = b
    assert f(45009) < 45009 ** 2 * 8
    assert f(45009) <= 64 * 45009                 # a few vectors, not a matrix


def test_bad_arguments_fail_on_the_host(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: validation comes before any device work
    big = ctypes.c_size_t(1 << 20)

    def bad(name, args):
        assert getattr(lib, name)(*args) == -1         # ISLAM_EARG
        assert name.encode() in lib.islam_last_error()

    # A, diag, n, workspace, workspace_bytes, info, stream
    good = [one, one, 18, one, big, one, None]
    for k in (0, 1, 3, 5):
        a = list(good)
        a[k] = None
        bad('islam_dense_chol_factor', a)
    for n in (0, -1):
        a = list(good)
        a[2] = n
        bad('islam_dense_chol_factor', a)
    a = list(good)
    a[4] = ctypes.c_size_t(lib.islam_dense_chol_workspace_bytes(18) - 1)
    bad('islam_dense_chol_factor', a)
    # L, n, b, x, workspace, workspace_bytes, stream
    good = [one, 18, one, one, one, big, None]
    for k in (0, 2, 3, 4):
        a = list(good)
        a[k] = None
        bad('islam_dense_chol_solve', a)
    for n in (0, -7):
        a = list(good)
        a[1] = n
        bad('islam_dense_chol_solve', a)
    a = list(good)
    a[5] = ctypes.c_size_t(lib.islam_dense_chol_workspace_bytes(18) - 1)
    bad('islam_dense_chol_solve', a)


def _loop_args():
    z = torch.zeros
    links = torch.tensor([[0, 1], [0, 2], [2, 3]])       # not the canonical chain
    return (z(4, 7), z(4, 3), z(3, 7), links, z(3), z(3, 4), z(3, 3), z(3, 3))


def test_run_pvgo_knows_dense_hip(lib):
    """The solver name is checked before anything touches the device: an unknown name is a ValueError whose text lists the new value,
    'dense_hip' is accepted and, without a GPU, ends in the RuntimeError every entry point of the package gives there."""
    from islam_amd import pvgo
    assert 'dense_hip' in pvgo._GENERAL_SOLVERS and {'auto', 'dense', 'band_pcg'} <= set(pvgo._GENERAL_SOLVERS)
    with pytest.raises(ValueError, match="'auto', 'dense', 'dense_hip' or 'band_pcg'"):
        pvgo.run_pvgo(*_loop_args(), device='cuda', general_solver='nope')
    if torch.cuda.is_available():
        pytest.skip('GPU present: tests/test_dense_chol_gpu.py runs the solver')
    for dev in ('cpu', 'cuda'):
        with pytest.raises(RuntimeError):
            pvgo.run_pvgo(*_loop_args(), device=dev, general_solver='dense_hip')


def test_kernels_use_no_scratch(lib):
    """The kernel metadata as tests/test_codeobj_cpu.py reads it: no private memory and no spilled register in any kernel of the family."""
    from tests.test_codeobj_cpu import READELF, _field, _kernels
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    ks = {k: v for k, v in _kernels().items() if re.search(r'chol_(update|diag|panel|fwd|bwd)_kernel', k)}
    assert len(ks) == 5, sorted(ks)
    for name, blk in ks.items():
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, name


def test_fragment_map_model():
    """numpy model of the index formulas of chol_update_kernel: operands A[m][k = q], B[k = q][n = m], results row = q + 4 i, col = m
    (q = lane >> 4, m = lane & 15); a lane holds columns k0 + 4 q .. + 3 of its row and MFMA kk of a chunk takes element kk.  With these
    formulas a 16-column chunk contributes exactly L_i L_j^T over its 16 columns."""
    rng = np.random.default_rng(0)
    Li, Lj = rng.integers(-3, 4, (16, 32)).astype(float), rng.integers(-3, 4, (16, 32)).astype(float)
    lane = np.arange(64)
    m, q = lane & 15, lane >> 4
    acc = np.zeros((64, 4))
    for k0 in range(0, 32, 16):
        fa = np.stack([Li[m, k0 + 4 * q + e] for e in range(4)], 1)     # (lane, element)
        fb = np.stack([Lj[m, k0 + 4 * q + e] for e in range(4)], 1)
        for kk in range(4):
            a_op, b_op = fa[:, kk], fb[:, kk]                             # one double per lane
            Amat, Bmat = np.zeros((16, 4)), np.zeros((4, 16))
            Amat[m, q] = a_op                                             # A[lane & 15][lane >> 4]
            Bmat[q, m] = b_op                                             # B[lane >> 4][lane & 15]
            D = Amat @ Bmat
            for i in range(4):
                acc[:, i] += D[q + 4 * i, m]                              # C/D: row = (lane >> 4) + 4 reg, col = lane & 15
    out = np.zeros((16, 16))
    for i in range(4):
        out[q + 4 * i, m] = acc[:, i]
    np.testing.assert_array_equal(out, Li @ Lj.T)
