"""Loop closures as additional edges (E != N - 1) on the CPU: the input condition of every graph that
tests/test_added_edges_gpu.py runs as an LM trajectory, the host-side validator of ``links``, the band bookkeeping (off-band edges, the
coupling block of adjacent pairs, the two CSR lists) on parallel and reversed edges against a plain numpy statement, and the code
objects of the two band kernels."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import pvgo as opvgo
from tests.closure_graphs import CASES, LW, UNIT, case, sizes
from tests.test_info_cpu import MARGIN, margin, pattern, random_omegas, run_info, scalar_omegas
from tests.test_robust_cpu import robust_loss, run_robust

# every (case, weights) tests/test_added_edges_gpu.py runs as a trajectory against oracle.pvgo.run_pvgo / run_info
PLAIN_RUNS = [('more17', UNIT), ('more17', LW), ('fewer17', UNIT), ('fewer17', LW), ('n2e3', UNIT), ('n3e1', UNIT)]
INFO_RUNS = ['more17', 'fewer17']
ROBUST_RUNS = [(name, kind) for name in ('more17', 'fewer17') for kind in ('huber', 'cauchy')]


def info_omegas(name):
    N, E, M = sizes(name)
    return random_omegas(E, M, UNIT, 100 + E)


def robust_kernel(kind):
    from islam_amd.robust import Cauchy, Huber
    return {'huber': Huber(0.1), 'cauchy': Cauchy(0.1)}[kind]


@functools.lru_cache(maxsize=None)
def info_reference(name, lw=None):
    """run_info on a case: lw given -> scalar information lw (the plain LM), lw None -> the random information of info_omegas."""
    N, E, M = sizes(name)
    return run_info(case(name), scalar_omegas(E, M, lw) if lw is not None else info_omegas(name), lw if lw is not None else UNIT, 'dense')


@functools.lru_cache(maxsize=None)
def robust_reference(name, kind):
    from islam_amd.robust import parse_kernel
    return run_robust(case(name), parse_kernel(robust_kernel(kind)), mode='dense')


def robust_margin(prob, spec, opt):
    """margin() for the robust restatement, whose trace does not carry the loss a trial is compared with: that loss is the initial
    one until a trial is accepted, then the accepted trial's."""
    c = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    res = opvgo.residuals(c(prob['init_nodes']), c(prob['init_vels']), np.asarray(prob['links'], dtype=np.int64), c(prob['vo_motions']),
                          c(prob['imu_drots']), c(prob['imu_dtrans']), c(prob['imu_dvels']), c(prob['dts']))
    last, worst = robust_loss(res, spec), np.inf
    for loss, _, accepted in opt.trace:
        worst = min(worst, abs(last - loss) / last)
        if accepted:
            last = loss
    return worst


# ------------------------------------------------------------------ the input condition
def test_case_table():
    assert {n: sizes(n) for n in CASES} == {'more17': (17, 21, 16), 'fewer17': (17, 14, 16), 'n2e3': (2, 3, 1), 'n3e1': (3, 1, 2),
                                            'n3e4': (3, 4, 2)}
    for name in CASES:
        N, E, M = sizes(name)
        p = case(name)
        assert p['links'].shape == (E, 2) and p['vo_motions'].shape == (E, 7) and p['init_nodes'].shape[0] == N and len(p['dts']) == M
    l = case('more17')['links']
    assert l[-1].tolist() == l[-5].tolist() == [0, 9] and l[-3].tolist() == [16, 2] and l[-2].tolist() == l[3].tolist() == [3, 4]
    assert 1 not in case('n3e1')['links']


@pytest.mark.parametrize('name,lw', PLAIN_RUNS)
def test_input_condition_plain(name, lw):
    """Every accept / reject verdict of the restatement is at least MARGIN (relative) from flipping, and scalar information takes the
    oracle LM's steps on these graphs too."""
    nodes, vels, opt = info_reference(name, lw)
    print(name, lw, len(opt.trace), 'trials', pattern(opt), 'margin %.2e' % margin(opt))
    assert margin(opt) >= MARGIN
    ref = opvgo.run_pvgo(**case(name), loss_weight=lw, mode='dense', return_optimizer=True)[5]
    assert [bool(t[2]) for t in ref.trace] == [t[2] for t in opt.trace]
    np.testing.assert_allclose([t[0] for t in ref.trace], [t[0] for t in opt.trace], rtol=1e-9)


@pytest.mark.parametrize('name', INFO_RUNS)
def test_input_condition_information(name):
    nodes, vels, opt = info_reference(name)
    print(name, len(opt.trace), 'trials', pattern(opt), 'margin %.2e' % margin(opt))
    assert margin(opt) >= MARGIN
    n0, _, _ = info_reference(name, UNIT)
    assert np.abs(nodes - n0).max() > 1e-4                     # the case cannot pass on scalar weights


@pytest.mark.parametrize('name,kind', ROBUST_RUNS)
def test_input_condition_robust(name, kind):
    from islam_amd.robust import parse_kernel
    nodes, vels, opt = robust_reference(name, kind)
    m = robust_margin(case(name), parse_kernel(robust_kernel(kind)), opt)
    print(name, kind, len(opt.trace), 'trials', ''.join('A' if t[2] else 'r' for t in opt.trace), 'margin %.2e' % m)
    assert m >= MARGIN


# ------------------------------------------------------------------ the validator
def test_validator_messages():
    from islam_amd.pvgo_dense import validate_graph
    ok = validate_graph(4, [[0, 1], [3, 1], [1, 0], [0, 1], [0, 3]], 5, dict(dts=3, imu_drots=3))
    assert ok.dtype == np.int64 and ok.shape == (5, 2)
    assert validate_graph(3, torch.tensor([[0, 2]]), 1).tolist() == [[0, 2]]                  # fewer edges than intervals
    with pytest.raises(ValueError, match=r'links: shape \(E, 2\) expected, got \(3,\)'):
        validate_graph(4, [0, 1, 2], 3)
    with pytest.raises(ValueError, match=r'got \(2, 3\)'):
        validate_graph(4, np.zeros((2, 3), dtype=np.int64), 2)
    with pytest.raises(ValueError, match=r'at least one VO edge is needed \(E = 0\)'):
        validate_graph(4, np.zeros((0, 2), dtype=np.int64), 0)
    with pytest.raises(ValueError, match='integer node indices'):
        validate_graph(4, np.array([[0.0, 1.0]]), 1)
    with pytest.raises(ValueError, match=r'links\[2\] = \(2, 2\) is a self-loop'):
        validate_graph(4, [[0, 1], [1, 2], [2, 2], [3, 3]], 4)
    with pytest.raises(ValueError, match=r'links\[1\] = \(1, 4\): node index outside \[0, 4\)'):
        validate_graph(4, [[0, 1], [1, 4], [2, 2]], 3)
    with pytest.raises(ValueError, match=r'links\[0\] = \(-1, 2\): node index outside'):
        validate_graph(4, [[-1, 2], [1, 1]], 2)
    with pytest.raises(ValueError, match=r'links\[0\] = \(7, 7\): node index outside'):        # out of range wins over self-loop
        validate_graph(4, [[7, 7]], 1)
    with pytest.raises(ValueError, match='one VO motion per edge: 3 motions for 2 edges'):
        validate_graph(4, [[0, 1], [0, 2]], 3)
    with pytest.raises(ValueError, match=r'dts: 4 rows, one per IMU interval expected \(N - 1 = 3\)'):
        validate_graph(4, [[0, 1]], 1, dict(imu_drots=3, dts=4))
    with pytest.raises(ValueError, match='at least 2 nodes'):
        validate_graph(1, [[0, 1]], 1)


def test_lm_entry_points_validate_before_device_work():
    """_lm_graph is where run_lm_dense and run_lm_band_pcg check their inputs: host tensors are enough to reach every refusal, and the
    refusal of E != N - 1 is gone."""
    from islam_amd import pvgo_dense
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    N = 5
    good = dict(nodes=z(N, 7), poses=z(6, 7), drots=z(N - 1, 4), dtrans=z(N - 1, 3), dvels=z(N - 1, 3), dts=z(N - 1))
    links = torch.tensor([[0, 1], [1, 2], [2, 3], [3, 4], [0, 4], [4, 0]])

    def graph(edges=links, **kw):
        a = dict(good, **kw)
        return pvgo_dense._lm_graph(a['nodes'], edges, a['poses'], a['drots'], a['dtrans'], a['dvels'], a['dts'], UNIT, None, None)

    g = graph()
    assert g.N == N and g.edges.shape[0] == 6
    assert graph(links[:2], poses=z(2, 7)).edges.shape[0] == 2
    with pytest.raises(ValueError, match='self-loop'):
        graph(torch.tensor([[0, 1], [2, 2]]), poses=z(2, 7))
    with pytest.raises(ValueError, match=r'links\[5\] = \(4, 5\)'):
        graph(torch.tensor(links.tolist()[:5] + [[4, 5]]))
    with pytest.raises(ValueError, match='one VO motion per edge: 4 motions for 6 edges'):
        graph(poses=z(4, 7))
    with pytest.raises(ValueError, match='E = 0'):
        graph(links[:0], poses=z(0, 7))
    with pytest.raises(ValueError, match='imu_dvels: 5 rows'):
        graph(dvels=z(N, 3))
    with pytest.raises(ValueError, match='dts: 3 rows'):
        graph(dts=z(3))


# ------------------------------------------------------------------ band bookkeeping
def _walk(edges, N, S):
    """What band_assemble_kernel does with one symmetric block S[e] per edge, in numpy: node t walks its CSR row; every entry adds S to
    the node's diagonal block, and -S to the coupling block of (t, t + 1) when the entry's other end is t + 1.  The off-band list and
    its own CSR come from _BandTopology's construction.  Returns the dense matrix the band arrays and the list stand for."""
    from islam_amd.pvgo_dense import _node_adjacency, off_band_edges
    nptr, nadj = _node_adjacency(edges, N)
    A = np.zeros((N, N) + S.shape[1:])
    for t in range(N):
        for code in nadj[nptr[t]:nptr[t + 1]]:
            e, end = code >> 1, code & 1
            assert edges[e, end] == t
            A[t, t] += S[e]
            if edges[e, 1 - end] == t + 1:
                A[t, t + 1] -= S[e]
                A[t + 1, t] -= S[e].T
    off = off_band_edges(edges)
    optr, oadj = _node_adjacency(edges[off], N)
    for t in range(N):
        for code in oadj[optr[t]:optr[t + 1]]:
            k, end = code >> 1, code & 1
            i, j = edges[off[k]]
            assert (i, j)[end] == t
            A[t, (j, i)[end]] -= S[off[k]]
    return A


@pytest.mark.parametrize('name', sorted(CASES) + ['reversed_chain'])
def test_band_bookkeeping_against_numpy(name):
    from islam_amd.pvgo_dense import _BandTopology, _node_adjacency, off_band_edges
    if name == 'reversed_chain':
        N, edges = 6, np.array([[1, 0], [2, 1], [1, 2], [3, 2], [5, 3], [3, 5], [4, 5], [5, 4], [0, 5]], dtype=np.int64)
    else:
        N, edges = sizes(name)[0], case(name)['links']
    E = edges.shape[0]
    d = np.abs(edges[:, 0] - edges[:, 1])
    assert off_band_edges(edges).tolist() == [e for e in range(E) if d[e] > 1]
    topo = _BandTopology(edges, N, 'cpu')
    off = off_band_edges(edges)
    assert topo.K == len(off) and topo.off_idx.tolist() == off.tolist() and topo.optr.tolist()[-1] == 2 * topo.K
    assert sorted(topo.oadj.tolist()) == list(range(2 * topo.K)) and topo.nptr.shape == topo.optr.shape == (N + 1,)
    nptr, nadj = _node_adjacency(edges, N)
    assert nptr[0] == 0 and nptr[-1] == 2 * E and sorted(nadj.tolist()) == list(range(2 * E))
    for t in range(N):
        row = nadj[nptr[t]:nptr[t + 1]].tolist()
        assert row == sorted(c for c in range(2 * E) if edges[c >> 1, c & 1] == t)           # ascending: the summation order
    rng = np.random.default_rng(E)
    S = rng.normal(size=(E, 2, 2))
    S = S + S.transpose(0, 2, 1)
    want = np.zeros((N, N, 2, 2))
    for e, (i, j) in enumerate(edges):
        want[i, i] += S[e]
        want[j, j] += S[e]
        want[i, j] -= S[e]
        want[j, i] -= S[e]
    np.testing.assert_allclose(_walk(edges, N, S), want, atol=1e-14)


# ------------------------------------------------------------------ the code objects
def test_band_kernels_use_no_scratch():
    """No private memory and no spilled register in band_assemble_kernel (three instances), band_matvec_kernel and the dense assembly
    over the same weighting function, dense_nodes_kernel and dense_edges_kernel (three instances each)."""
    import __graft_entry__ as g
    g.build()
    from tests.test_codeobj_cpu import READELF, _field, _kernels
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    ks = {k: v for k, v in _kernels().items() if re.search(r'band_(assemble|matvec)_kernel|dense_(nodes|edges)_kernel', k)}
    assert len(ks) == 10, sorted(ks)
    for name, blk in ks.items():
        print(name, 'vgpr', _field(blk, 'vgpr_count'), 'sgpr', _field(blk, 'sgpr_count'), 'lds', _field(blk, 'group_segment_fixed_size'))
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, name
