"""Loop closures as additional edges (E != N - 1) on the MI355X: run_pvgo on every general-topology solver
against the oracle's dense LM and the restatements of tests/test_info_cpu.py / tests/test_robust_cpu.py, the dense and the band
assembly against J^T W J of the oracle's dense Jacobian, islam_pvgo_band_matvec against the dense product, marginal covariances,
the returned values and the refused inputs.  The graphs are those of tests/closure_graphs.py; tests/test_added_edges_cpu.py asserts
the input condition of every one that runs as an LM trajectory here."""
import functools

import numpy as np
import pytest
import torch

from oracle import lie, pvgo as opvgo
from tests.closure_graphs import CASES, LW, UNIT, case, closure_graph, sizes
from tests.helpers import se3_log_err
from tests.test_added_edges_cpu import INFO_RUNS, PLAIN_RUNS, ROBUST_RUNS, info_omegas, info_reference, robust_kernel, robust_reference
from tests.test_info_cpu import pvgo_info
from tests.test_robust_gpu import _check_against

pytestmark = pytest.mark.gpu
SOLVERS = ('dense', 'dense_hip', 'band_pcg')
W2 = lambda lw: [float(x) ** 2 for x in lw]


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _d(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


def _run(prob, lw, **kw):
    from islam_amd import lietensor as pp
    from islam_amd.pvgo import run_pvgo
    return run_pvgo(pp.SE3(_t(prob['init_nodes'])), _t(prob['init_vels']), pp.SE3(_t(prob['vo_motions']).to('cuda')),
                    torch.tensor(prob['links']), _t(prob['dts']), pp.SO3(_t(prob['imu_drots'])), _t(prob['imu_dtrans']),
                    _t(prob['imu_dvels']), device='cuda', loss_weight=lw, **kw)


def _solvers_agree(out):
    """tests/test_surface_gpu.py::test_general_topology_band_pcg_equals_dense: equal steps and trials, trace rtol 1e-9, iterates 1e-9."""
    d = out['dense']
    for how in out:
        o = out[how]
        assert o[5]['steps'] == d[5]['steps'] and o[5]['trials'] == d[5]['trials'], how
        np.testing.assert_allclose([x[0] for x in o[5]['trace']], [x[0] for x in d[5]['trace']], rtol=1e-9)
        np.testing.assert_allclose(o[2].tensor().numpy(), d[2].tensor().numpy(), atol=1e-9)
        np.testing.assert_allclose(o[3].numpy(), d[3].numpy(), atol=1e-9)


# ------------------------------------------------------------------ 1. oracle, plain
@functools.lru_cache(maxsize=None)
def _oracle(name, lw):
    return opvgo.run_pvgo(**case(name), loss_weight=lw, mode='dense')


@pytest.mark.parametrize('name,lw', PLAIN_RUNS)
def test_run_pvgo_matches_oracle_on_every_solver(cuda, name, lw):
    prob = case(name)
    N, E, M = sizes(name)
    otl, orl, on, ov, _ = _oracle(name, lw)
    ref = np.maximum(np.linalg.norm(lie.se3_log(on), axis=-1), 1e-6)
    out = {how: _run(prob, lw, general_solver=how, return_info=True) for how in SOLVERS + ('auto',)}
    for how, o in out.items():
        err = se3_log_err(o[2].tensor().numpy(), on)
        print('%s %s %s: %d trials, worst relative se3_log error %.2e' % (name, lw, how, o[5]['trials'], (err / ref).max()))
        assert (err / ref).max() < 1e-6, how
        np.testing.assert_allclose(o[3].numpy(), ov, atol=1e-7)
        assert o[0].shape == (E,)
        np.testing.assert_allclose(o[0].cpu().numpy(), otl, rtol=1e-6, atol=1e-10)
    assert 'pcg_iterations' in out['band_pcg'][5] and 'pcg_iterations' not in out['auto'][5]          # N <= 512: 'auto' is dense
    assert out['band_pcg'][5]['off_band_edges'] == int((np.abs(prob['links'][:, 0] - prob['links'][:, 1]) > 1).sum())
    _solvers_agree(out)


# ------------------------------------------------------------------ 2. assembly
def _reference_normal(prob, w_rows):
    """(A, b, J (rows x 9N, node-major), R) of the oracle's dense Jacobian at the initial state; w_rows: one weight per residual row."""
    links = prob['links']
    N = prob['init_nodes'].shape[0]
    res = opvgo.residuals(prob['init_nodes'], prob['init_vels'], links, prob['vo_motions'], prob['imu_drots'], prob['imu_dtrans'],
                          prob['imu_dvels'], prob['dts'])
    Ae, Bk = opvgo.jac_blocks(prob['init_nodes'], links, prob['vo_motions'], prob['imu_drots'], res[0], res[2])
    J10 = opvgo.jacobian_dense(N, links, Ae, Bk, prob['dts'])
    cols = np.concatenate([np.concatenate([7 * k + np.arange(6), 7 * N + 3 * k + np.arange(3)]) for k in range(N)])
    J = J10[:, cols]
    R = np.concatenate([r.reshape(-1) for r in res])
    return (J.T * w_rows) @ J, -(J.T * w_rows) @ R, J, R


def _device_pieces(prob):
    """(vo, lin) at the initial state, graph(lw, info) -> the pvgo_dense._Graph under those weights, and the band topology."""
    from islam_amd import pvgo_dense
    N = prob['init_nodes'].shape[0]
    nodes, vels, poses = _d(prob['init_nodes']), _d(prob['init_vels']), _d(prob['vo_motions'])
    drots, dtrans, dvels, dts = _d(prob['imu_drots']), _d(prob['imu_dtrans']), _d(prob['imu_dvels']), _d(prob['dts'])
    edges = torch.tensor(prob['links'], device='cuda')
    graph = lambda lw, info=None: pvgo_dense._Graph(nodes, edges, poses, drots, dtrans, dvels, dts, lw, info)
    vo, lin = graph(LW).linearize(nodes, vels)
    return vo, lin, graph, pvgo_dense._BandTopology(prob['links'], N, torch.device('cuda'))


def _dense_assembly(vo, lin, graph, topo, N, lw, c_vo=None, c_imu=None, info=None):
    from islam_amd import ops
    g = graph(lw, info)
    Hd, Ho, rhs = g.imu_part(lin, c_imu)
    A = torch.full((9 * N, 9 * N), float('nan'), dtype=torch.float64, device='cuda')
    b = torch.full((9 * N,), float('nan'), dtype=torch.float64, device='cuda')
    ops.pvgo_assemble_dense(Hd, Ho, rhs, vo, g.edges, topo.nptr, topo.nadj, g.w[0], c_vo, g.info_vo, out=(A, b))
    return A.cpu().numpy(), b.cpu().numpy()


def _band_assembly(vo, lin, graph, topo, N, lw, c_vo=None, c_imu=None, info=None):
    """The band arrays and the off-band list of islam_pvgo_band_assemble, as they are and expanded to the dense matrix they stand for."""
    from islam_amd import ops
    g = graph(lw, info)
    Hd, Ho, rhs = g.imu_part(lin, c_imu)
    io, jo, So = ops.pvgo_band_assemble(Hd, Ho, rhs, vo, g.edges, topo.nptr, topo.nadj, g.w[0], topo.off_idx, c_vo, g.info_vo)
    raw = [x.cpu().numpy() for x in (Hd, Ho, rhs, io, jo, So)]
    hd, ho, b, i_, j_, so = raw
    A = np.zeros((9 * N, 9 * N))
    for k in range(N):
        A[9 * k:9 * k + 9, 9 * k:9 * k + 9] = hd[k]
        if k < N - 1:
            A[9 * k:9 * k + 9, 9 * k + 9:9 * k + 18] = ho[k]
            A[9 * k + 9:9 * k + 18, 9 * k:9 * k + 9] = ho[k].T
    for t in range(len(i_)):
        A[9 * i_[t]:9 * i_[t] + 6, 9 * j_[t]:9 * j_[t] + 6] -= so[t]
        A[9 * j_[t]:9 * j_[t] + 6, 9 * i_[t]:9 * i_[t] + 6] -= so[t].T
    return A, b.reshape(-1), raw, (Hd, Ho, io, jo, So)


def _weights(name, mode):
    """mode 'plain' | 'scaled' | 'info' -> (row weights of the reference, kwargs of the two assemblies)"""
    N, E, M = sizes(name)
    if mode == 'plain':
        return opvgo.weight_vector(E, M, LW, np.float64), {}
    if mode == 'scaled':
        rng = np.random.default_rng(7 + E)
        c_vo, c_imu = rng.uniform(0.2, 1.0, E), rng.uniform(0.2, 1.0, (3, M))
        rows = np.concatenate([np.repeat(c_vo, 6), np.repeat(c_imu[0], 3), np.repeat(c_imu[1], 3), np.repeat(c_imu[2], 3)])
        return opvgo.weight_vector(E, M, LW, np.float64) * rows, dict(c_vo=_d(c_vo), c_imu=_d(c_imu))
    om = info_omegas(name)
    return om, dict(info=pvgo_info(om).packed(E, M, UNIT, 'cuda'))


def _reference_for(name, mode):
    prob = case(name)
    w, kw = _weights(name, mode)
    if mode != 'info':
        A, b, _, _ = _reference_normal(prob, w)
        return A, b, kw
    _, _, J, R = _reference_normal(prob, 1.0)
    N, E, M = sizes(name)
    W = np.zeros((J.shape[0], J.shape[0]))
    r0 = 0
    for rows, Om in zip((6, 3, 3, 3), w):
        for f in range(Om.shape[0]):
            W[r0:r0 + rows, r0:r0 + rows] = Om[f]
            r0 += rows
    return J.T @ W @ J, -J.T @ W @ R, kw


@pytest.mark.parametrize('mode', ['plain', 'scaled', 'info'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_assemblies_match_the_dense_jacobian_product(cuda, name, mode):
    """islam_pvgo_assemble_dense / _scaled / _info and islam_pvgo_band_assemble against J^T W J and -J^T W r of the oracle's dense
    Jacobian at the tolerance of tests/test_surface_gpu.py::test_dense_assembly_matches_dense_jacobian_product; the band arrays and
    the off-band list expanded to dense equal the dense assembly to the same tolerance; a second call gives the same bits."""
    N, E, M = sizes(name)
    A_ref, b_ref, kw = _reference_for(name, mode)
    lw = UNIT if mode == 'info' else LW
    pieces = _device_pieces(case(name))
    A_d, b_d = _dense_assembly(*pieces, N, lw, **kw)
    A_b, b_b, raw, _ = _band_assembly(*pieces, N, lw, **kw)
    scale, bscale = np.abs(A_ref).max(), np.abs(b_ref).max()
    for what, A, b in (('dense', A_d, b_d), ('band', A_b, b_b)):
        print('%s %s %s: A error %.2e, b error %.2e (of the largest entry)' % (name, mode, what, np.abs(A - A_ref).max() / scale,
                                                                                np.abs(b - b_ref).max() / bscale))
        np.testing.assert_allclose(A, A_ref, atol=1e-12 * scale)
        np.testing.assert_allclose(b, b_ref, atol=1e-11 * bscale)
    np.testing.assert_allclose(A_b, A_d, atol=1e-12 * scale)
    np.testing.assert_allclose(b_b, b_d, atol=1e-11 * bscale)
    assert raw[3].tolist() == [int(i) for i, j in case(name)['links'] if abs(i - j) > 1]
    assert raw[4].tolist() == [int(j) for i, j in case(name)['links'] if abs(i - j) > 1]
    again = _band_assembly(*pieces, N, lw, **kw)[2]
    for x, y in zip(raw, again):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    A2, b2 = _dense_assembly(*pieces, N, lw, **kw)
    if name != 'more17' and name != 'n2e3' and name != 'n3e4':          # (parallel edges: the dense off-diagonal atomics may reorder)
        assert np.array_equal(A2.view(np.int64), A_d.view(np.int64))
    assert np.array_equal(b2.view(np.int64), b_d.view(np.int64))


def test_dense_modes_share_one_weighting(cuda):
    """The three modes of ops.pvgo_assemble_dense run the same kernels over one weighting function, on the
    smallest graphs that hold each hazard: n2e3 (all edges parallel, one reversed), n3e1 (an empty CSR row), fewer17 (frames without a
    VO edge), more17 (a parallel pair, an adjacent duplicate, a reversed edge).  Scaled mode with c_vo = 1 gives the bits of plain mode
    -- w0 * 1.0 is exact and the two instances run the same statements -- for b everywhere and for all of A where no two edges share
    a node pair (n3e1, fewer17: the atomics cannot reorder).  Info mode with Omega0_e = w0 c_e I6 agrees with scaled mode at the
    tolerances of test_assemblies_match_the_dense_jacobian_product.  Then the refused arguments of the wrapper and of the C symbols."""
    from islam_amd import ops
    from islam_amd._lib import c_double, lib
    w = W2(LW)
    for name in ('n2e3', 'n3e1', 'fewer17', 'more17'):
        N, E, M = sizes(name)
        pieces = _device_pieces(case(name))
        A_p, b_p = _dense_assembly(*pieces, N, LW)
        A_1, b_1 = _dense_assembly(*pieces, N, LW, c_vo=torch.ones(E, dtype=torch.float64, device='cuda'))
        assert np.array_equal(b_1.view(np.int64), b_p.view(np.int64)), name
        if name in ('n3e1', 'fewer17'):
            assert np.array_equal(A_1.view(np.int64), A_p.view(np.int64)), name
        c = np.random.default_rng(11 + E).uniform(0.2, 1.0, E)
        info_vo, info_imu = np.zeros((21, E)), np.zeros((18, M))
        info_vo[[0, 6, 11, 15, 18, 20]] = w[0] * c                         # the diagonal of the packed upper triangle of a 6x6
        for grp in range(3):                                                # [velocity | rotation | translation-velocity], [00 01 02 11 12 22]
            info_imu[[6 * grp, 6 * grp + 3, 6 * grp + 5]] = w[1 + grp]
        A_s, b_s = _dense_assembly(*pieces, N, LW, c_vo=_d(c))
        A_i, b_i = _dense_assembly(*pieces, N, LW, info=(_d(info_vo), _d(info_imu)))
        scale, bscale = np.abs(A_s).max(), np.abs(b_s).max()
        print('%s: info vs scaled, A %.2e, b %.2e (of the largest entry)' % (name, np.abs(A_i - A_s).max() / scale, np.abs(b_i - b_s).max() / bscale))
        np.testing.assert_allclose(A_i, A_s, atol=1e-12 * scale)
        np.testing.assert_allclose(b_i, b_s, atol=1e-11 * bscale)

    vo, lin, graph, topo = pieces                                           # more17
    g = graph(LW)
    Hd, Ho, rhs = g.imu_part(lin)
    args = lambda **kw: [kw.get(k, v) for k, v in (('Hd', Hd), ('Ho', Ho), ('rhs', rhs), ('vo', vo), ('edges', g.edges), ('nptr', topo.nptr),
                                                   ('nadj', topo.nadj), ('w0', w[0]))]
    ones = lambda *shape, dtype=torch.float64: torch.ones(shape, dtype=dtype, device='cuda')
    for bad in (dict(c_vo=ones(E), info_vo=ones(21, E)), dict(c_vo=ones(E + 1)), dict(c_vo=ones(E, 1)), dict(info_vo=ones(20, E)),
                dict(c_vo=ones(2 * E)[::2]), dict(c_vo=ones(E, dtype=torch.float32)), dict(info_vo=ones(E, 21).t()),
                dict(info_vo=ones(21, E, dtype=torch.float32))):
        with pytest.raises(ValueError, match='pvgo_assemble_dense'):
            ops.pvgo_assemble_dense(*args(), **bad)
    for bad in (dict(vo=vo.t().contiguous().t()), dict(Hd=Hd.float()), dict(edges=g.edges.int())):
        with pytest.raises(ValueError, match='pvgo_assemble_dense'):
            ops.pvgo_assemble_dense(*args(**bad))
    L = lib()
    assert L.islam_pvgo_assemble_dense(*[None] * 7, c_double(1.0), 1, 0, None, None, None) == -1
    assert b'islam_pvgo_assemble_dense:' in L.islam_last_error()
    assert L.islam_pvgo_assemble_dense_scaled(*[None] * 8, c_double(1.0), 1, 0, None, None, None) == -1
    assert b'islam_pvgo_assemble_dense_scaled:' in L.islam_last_error()
    assert L.islam_pvgo_assemble_dense_info(*[None] * 8, 1, 0, None, None, None) == -1
    assert b'islam_pvgo_assemble_dense_info:' in L.islam_last_error()


# ------------------------------------------------------------------ 3. matvec
def _fewer17_without_closure():
    F, extra, drop = CASES['fewer17']
    return closure_graph(F, (), drop)


@pytest.mark.parametrize('name', ['more17', 'n2e3', 'n3e1', 'no_off_band'])
def test_band_matvec_matches_the_dense_product(cuda, name):
    """Per row |y - A p| <= 1e-13 (|A| |p|): an fp64 sum of under a hundred terms is within n 2^-53 of that; 1e-13 leaves a factor ten."""
    from islam_amd import ops
    prob = _fewer17_without_closure() if name == 'no_off_band' else case(name)
    N = prob['init_nodes'].shape[0]
    pieces = _device_pieces(prob)
    topo = pieces[3]
    A, _, _, (Hd, Ho, io, jo, So) = _band_assembly(*pieces, N, LW)
    assert (topo.K == 0) == (name in ('no_off_band', 'n2e3')) and io.numel() == topo.K
    p = np.random.default_rng(3).normal(size=(N, 9))
    pd = _d(p)
    y = ops.pvgo_band_matvec(Hd, Ho, pd, topo.optr, topo.oadj, io, jo, So)
    want, bound = A @ p.reshape(-1), np.abs(A) @ np.abs(p.reshape(-1))
    err = np.abs(y.cpu().numpy().reshape(-1) - want)
    print('%s: worst |error| / (|A||p|) = %.2e' % (name, (err / bound).max()))
    assert np.all(err <= 1e-13 * bound)
    assert torch.equal(pd, _d(p))                                                   # the input is left alone
    assert torch.equal(ops.pvgo_band_matvec(Hd, Ho, pd, topo.optr, topo.oadj, io, jo, So), y)


# ------------------------------------------------------------------ 4. information
@pytest.mark.parametrize('name', INFO_RUNS)
def test_information_matches_restatement_on_every_solver(cuda, name):
    nodes_ref, vels_ref, opt = info_reference(name)
    info = pvgo_info(info_omegas(name))
    out = {}
    for how in SOLVERS:
        out[how] = _run(case(name), UNIT, info=info, general_solver=how, return_info=True)
        res = out[how][5]
        _check_against(out[how], res['steps'], res['trials'], res['trace'], nodes_ref, vels_ref, opt)
    _solvers_agree(out)
    N, E, M = sizes(name)
    covs = out['dense'][4]
    assert len(covs['vo_rot']) == len(covs['vo_trans']) == E and len(covs['imu_rot']) == M


# ------------------------------------------------------------------ 5. robust kernels
@pytest.mark.parametrize('name,kind', ROBUST_RUNS)
def test_robust_kernels_match_restatement_on_every_solver(cuda, name, kind):
    nodes_ref, vels_ref, opt = robust_reference(name, kind)
    out = {}
    for how in SOLVERS:
        out[how] = _run(case(name), LW, kernel=robust_kernel(kind), general_solver=how, return_info=True)
        res = out[how][5]
        _check_against(out[how], res['steps'], res['trials'], res['trace'], nodes_ref, vels_ref, opt)
    _solvers_agree(out)


# ------------------------------------------------------------------ 6. marginals
def test_marginals_on_added_edges(cuda):
    """pvgo_marginals_general and run_pvgo(marginals=True, general_solver='dense_hip') on more17 against numpy's inverse of the anchored
    oracle matrix at the tolerance of tests/test_dense_marginals_gpu.py; pairs default to all 21 links."""
    from islam_amd import pvgo
    from tests.test_dense_marginals_gpu import _anchored_inverse, _worst_block_error
    prob = case('more17')
    N, E, M = sizes('more17')
    dev = dict(nodes=_d(prob['init_nodes']), vels=_d(prob['init_vels']), vo_motions=_d(prob['vo_motions']),
               links=torch.tensor(prob['links'], device='cuda'), dts=_d(prob['dts']), imu_drots=_d(prob['imu_drots']),
               imu_dtrans=_d(prob['imu_dtrans']), imu_dvels=_d(prob['imu_dvels']))

    def check(mg, state):
        A = _reference_normal(dict(prob, init_nodes=state[0], init_vels=state[1]), opvgo.weight_vector(E, M, LW, np.float64))[0]
        S = _anchored_inverse(0.5 * (A + A.T), N, 0)
        assert mg.pairs.cpu().tolist() == prob['links'].tolist() and mg.pair_cov.shape == (E, 9, 9) and mg.node_cov.shape == (N, 9, 9)
        node, pair = mg.node_cov.cpu().numpy(), mg.pair_cov.cpu().numpy()
        worst = _worst_block_error(node, prob['links'], pair, S)
        print('more17 marginals: worst error / column scale = %.3e' % worst)
        assert worst <= 1e-9
        assert np.array_equal(pair[E - 1], pair[E - 5]) and np.abs(pair[E - 1]).max() > 0          # the parallel pair (0, 9), twice
        assert not node[0][:6, :].any() and not node[0][:, :6].any()

    check(pvgo.pvgo_marginals_general(**dev, loss_weight=LW), (prob['init_nodes'], prob['init_vels']))
    out = _run(prob, LW, general_solver='dense_hip', marginals=True)
    assert isinstance(out[-1], pvgo.PvgoGraphMarginals)
    check(out[-1], (out[2].tensor().numpy(), out[3].numpy()))


# ------------------------------------------------------------------ 7. returned values
@pytest.mark.parametrize('name', ['more17', 'fewer17'])
def test_returned_values_and_vo_gradient(cuda, name):
    from islam_amd import lietensor as pp
    from islam_amd.pvgo import run_pvgo
    prob = case(name)
    N, E, M = sizes(name)
    vo = _t(prob['vo_motions']).to('cuda').requires_grad_(True)
    args = (pp.SE3(_t(prob['init_nodes'])), _t(prob['init_vels']), pp.SE3(vo), torch.tensor(prob['links']), _t(prob['dts']),
            pp.SO3(_t(prob['imu_drots'])), _t(prob['imu_dtrans']), _t(prob['imu_dvels']))
    tl, rl, nodes, vels, covs, res = run_pvgo(*args, device='cuda', loss_weight=LW, target='vo', return_info=True)
    assert tl.shape == (E,) and rl.shape == (E,) and nodes.shape == (N, 7) and vels.shape == (N, 3)
    assert tl.host.shape == (E,) and res['trials'] >= res['steps'] >= 1
    assert covs['vo_rot'].shape == (E,) and covs['vo_trans'].shape == (E,) and np.all(covs['vo_rot'] == LW[0] ** 2)
    assert covs['imu_rot'].shape == covs['imu_vel'].shape == covs['transvel'].shape == (M,)
    loss_bp = torch.cat((1.0 * rl, 0.1 * tl))
    loss_bp.backward(torch.ones_like(loss_bp))
    g = vo.grad.cpu().numpy()
    opt = opvgo.run_pvgo(**prob, loss_weight=LW, mode='dense', return_optimizer=True)[5]
    og = opvgo.vo_loss_grad(opt.nodes, prob['links'], prob['vo_motions'], np.full(E, 0.1), np.full(E, 1.0))
    assert g.shape == (E, 7) and np.all(g[:, 6] == 0)
    np.testing.assert_allclose(g, og, rtol=5e-3, atol=1e-5)
    itl, irl = run_pvgo(*args, device='cuda', loss_weight=LW, target='imu')[:2]
    assert itl.shape == (M,) and irl.shape == (M,)


# ------------------------------------------------------------------ 8. refused inputs
def test_refused_inputs_leave_the_nodes_alone(cuda):
    from islam_amd import pvgo, pvgo_dense
    prob = case('more17')
    N, E, M = sizes('more17')
    links = prob['links']
    self_loop, too_large = links.copy(), links.copy()
    self_loop[18] = (7, 7)
    too_large[20] = (0, N)
    bad = [(self_loop, prob['vo_motions'], r'links\[18\] = \(7, 7\) is a self-loop'),
           (too_large, prob['vo_motions'], r'links\[20\] = \(0, 17\): node index outside \[0, 17\)'),
           (links, prob['vo_motions'][:-1], 'one VO motion per edge: 20 motions for 21 edges'),
           (links[:0], prob['vo_motions'][:0], r'E = 0')]
    nodes, vels = _d(prob['init_nodes']), _d(prob['init_vels'])
    rest = [_d(prob[k]) for k in ('imu_drots', 'imu_dtrans', 'imu_dvels', 'dts')]
    n0, v0 = nodes.clone(), vels.clone()
    for l, vo, msg in bad:
        with pytest.raises(ValueError, match=msg):
            _run(dict(prob, links=l, vo_motions=vo), LW)
        for how in SOLVERS:
            with pytest.raises(ValueError, match=msg):
                _run(dict(prob, links=l, vo_motions=vo), LW, general_solver=how)
        edges = torch.tensor(l, dtype=torch.int64, device='cuda').reshape(-1, 2)
        for fn in (pvgo_dense.run_lm_dense, pvgo_dense.run_lm_band_pcg):
            with pytest.raises(ValueError, match=msg):
                fn(nodes, vels, edges, _d(vo).reshape(-1, 7), *rest, LW)
        with pytest.raises(ValueError, match=msg):
            pvgo.pvgo_marginals_general(nodes, vels, _d(vo).reshape(-1, 7), edges, rest[3], rest[0], rest[1], rest[2], loss_weight=LW)
    assert torch.equal(nodes, n0) and torch.equal(vels, v0)
    from islam_amd._lib import lib
    assert lib().islam_pvgo_band_assemble(None, None, None, None, None, None, None, None, None, 1.0, 5, 4, None, 0, None, None, None, None) == -1
    assert b'islam_pvgo_band_assemble' in lib().islam_last_error()
    assert lib().islam_pvgo_band_matvec(None, None, None, None, None, None, None, None, 5, 0, None, None) == -1
