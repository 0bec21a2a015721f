"""The full 9x9 pre-integration information per IMU link on the MI355X (run_pvgo(info=PvgoInfo(vo=..., imu=...)); DESIGN.md section
3.22): info9_build_kernel against the contract's table in numpy, the chain loop (islam_pvgo_run_chain_info9) and the three
general-topology solvers against the float64 restatement of tests/test_info_full_cpu.py, the three kinds of marginals, IMU
pre-integration covariances end to end with their cross blocks, the paths of today left alone and the argument errors."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pvgo as opvgo
from tests.helpers import chain_problem, tumbling_problem
from tests.test_info_cpu import LW, MARGIN, UNIT, _inputs, margin, pattern, pvgo_info, random_omegas, run_info, scalar_omegas
from tests.test_info_full_cpu import (CHAIN_CASES9, _DenseLinInfo9, block_diag9, chain_case9, closure_case9, diag_blocks, omega9, pvgo_info9,
                                      run_info9, table9)
from tests.test_info_gpu import (IMU_ACC_COV, IMU_GYRO_COV, IMU_SEED, _assert_blocks, _build_info, _chain_trace, _d, _device_lin, _graph_dev)
from tests.test_robust_cpu import pose_error
from tests.test_robust_gpu import _check_against, _run

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ assembly
def _contract9(lin, dts, O0, O9, vmin, vmax):
    """The contract in numpy from a `lin` record (42,M): table9 for the IMU part, A_k^T Omega0 A_k for the VO
    group (O0 None: left out), the clamp last.  Returns Hd (N,9,9), Ho (N,9,9; the last block zero), rhs (N,9)."""
    M = lin.shape[1]
    N = M + 1
    m3 = lambda r: lin[r:r + 9].T.reshape(M, 3, 3)
    T = lambda a: np.swapaxes(a, 1, 2)
    e, G, C, er, B, rv, rt = lin[0:6].T, m3(6), m3(15), lin[24:27].T, m3(27), lin[36:39].T, lin[39:42].T
    Hd, Ho_m, g = table9(B, dts, rv, er, rt, O9)
    Ho = np.zeros((N, 9, 9))
    Ho[:-1] = Ho_m
    if O0 is not None:
        A = np.zeros((M, 6, 6))
        A[:, :3, :3], A[:, :3, 3:], A[:, 3:, 3:] = G, C, G
        S = T(A) @ O0 @ A
        gp = ((T(A) @ O0) @ e[:, :, None])[:, :, 0]
        Hd[:-1, :6, :6] += S
        Hd[1:, :6, :6] += S
        Ho[:-1, :6, :6] += -S
        g[1:, :6] += gp
        g[:-1, :6] -= gp
    i = np.arange(9)
    Hd[:, i, i] = np.clip(Hd[:, i, i], vmin, vmax)
    return Hd, Ho, -g


def _build9(lin, dts, N, O0, O9, vmin=1e-4, vmax=1e32):
    from islam_amd import ops
    from islam_amd.information import PvgoInfo
    iv, i9 = PvgoInfo(vo=O0, imu=O9).packed(N - 1, N - 1, UNIT, 'cuda')
    assert tuple(i9.shape) == (45, N - 1)
    return ops.pvgo_build_normal_info(lin, dts, N, iv if O0 is not None else None, i9, vmin, vmax)


@pytest.mark.parametrize('N', [2, 3, 64, 65, 130])
def test_build_normal_info9(cuda, N):
    """One link, a node with both ends, a full wave, a wave plus one lane, three workgroups."""
    from islam_amd import ops
    prob, _ = chain_problem(N)
    lin = _device_lin(prob)
    lin_h, dts_h, dts = lin.cpu().numpy(), np.asarray(prob['dts'], dtype=np.float64), _d(prob['dts'])
    M = N - 1
    O0 = random_omegas(M, M, LW, 100 + N)[0]
    O9 = omega9(M, LW, 900 + N)
    got = _build9(lin, dts, N, O0, O9)
    for g, w, what in zip(got, _contract9(lin_h, dts_h, O0, O9, 1e-4, 1e32), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s against the contract, N=%d' % (what, N))
    assert torch.equal(got[0], got[0].transpose(1, 2))                       # exactly symmetric node blocks
    assert float(got[0][:, 3:6, 6:9].abs().max()) > 0 and float(got[1][:-1, :, 6:9].abs().min()) > 0      # the blocks that were zero
    assert not got[1][-1].any()
    # a second call: the same bits
    again = _build9(lin, dts, N, O0, O9)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # a block-diagonal imu is islam_pvgo_build_normal_info
    om = random_omegas(M, M, LW, 100 + N)
    for g, w, what in zip(_build9(lin, dts, N, om[0], block_diag9(*om[1:])), _build_info(lin, dts, N, om), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s with a block-diagonal imu against build_normal_info, N=%d' % (what, N))
    # without the VO group
    novo = _build9(lin, dts, N, None, O9)
    for g, w, what in zip(novo, _contract9(lin_h, dts_h, None, O9, 1e-4, 1e32), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s without VO against the contract, N=%d' % (what, N))
    # Omega = 0 on one link: that link's scalar-zero result (robust multipliers 0 on its three IMU factors, w0 = 0), and the contract
    k = M // 2
    w4 = [x ** 2 for x in LW]
    om_s = scalar_omegas(M, M, LW)
    O9_z = block_diag9(*om_s[1:])
    O9_z[k] = 0.0
    c_imu = torch.ones((3, M), dtype=torch.float64, device='cuda')
    c_imu[:, k] = 0.0
    for g, w, what in zip(_build9(lin, dts, N, None, O9_z), ops.pvgo_build_normal(lin, dts, N, [0.0] + w4[1:], c_imu=c_imu), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s with link %d switched off, N=%d' % (what, k, N))
    O9_k = O9.copy()
    O9_k[k] = 0.0
    for g, w, what in zip(_build9(lin, dts, N, O0, O9_k), _contract9(lin_h, dts_h, O0, O9_k, 1e-4, 1e32), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s with Omega = 0 on link %d against the contract, N=%d' % (what, k, N))
    if N == 2:                                                              # every factor off: only the clamp is left
        Hd, Ho, rhs = _build9(lin, dts, N, np.zeros_like(O0), np.zeros_like(O9))
        assert torch.equal(Hd, 1e-4 * torch.eye(9, dtype=torch.float64, device='cuda').expand(2, 9, 9)) and not rhs.any() and not Ho.any()
    # the clamp
    Hd, Ho, rhs = _build9(lin, dts, N, O0, O9, vmin=5.0, vmax=6.0)
    dg = Hd.diagonal(dim1=1, dim2=2)
    assert float(dg.min()) >= 5.0 and float(dg.max()) <= 6.0
    _assert_blocks(Hd, _contract9(lin_h, dts_h, O0, O9, 5.0, 6.0)[0], 'Hd clamped to [5, 6], N=%d' % N)
    assert torch.equal(Ho, got[1]) and torch.equal(rhs, got[2])


def info_matrix9(nodes, vels, prob, O0, O9):
    """A = sum J^T Omega J (9N x 9N, per node [rho phi v]) and b = -sum J^T Omega r of the restatement at (nodes, vels)."""
    _, _, inp = _inputs(prob)
    N = nodes.shape[0]
    res = opvgo.residuals(nodes, vels, *inp)
    A_e, B_k = opvgo.jac_blocks(nodes, inp[0], inp[1], inp[2], res[0], res[2])
    lin = _DenseLinInfo9(nodes, inp, res, A_e, B_k, (O0, O9))
    cols = np.concatenate([np.concatenate([7 * k + np.arange(6), 7 * N + 3 * k + np.arange(3)]) for k in range(N)])
    return lin.A[np.ix_(cols, cols)], lin.b[cols]


def test_dense_assembly_on_the_closure_graph(cuda):
    from islam_amd.pvgo_dense import _DenseSystem, _Graph
    prob, O0, O9, lw, _ = closure_case9()
    d = _graph_dev(prob)
    packed = pvgo_info9(O0, O9).packed(32, 32, lw, 'cuda')
    g = _Graph(d['nodes'], d['edges'], d['poses'], d['drots'], d['dtrans'], d['dvels'], d['dts'], lw, packed)
    sysm = _DenseSystem(g)
    vo, lin = g.linearize(d['nodes'], d['vels'])
    sysm.fill(vo, lin)
    A, b = info_matrix9(np.asarray(prob['init_nodes'], np.float64), np.asarray(prob['init_vels'], np.float64), prob, O0, O9)
    np.testing.assert_allclose(sysm.A.cpu().numpy(), A, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(sysm.b.cpu().numpy(), b, rtol=1e-8, atol=1e-8)
    first = sysm.A.clone()
    sysm.fill(vo, lin)                                   # (no two edges of this graph share a node pair: one atomic per entry, same bits)
    assert torch.equal(first, sysm.A)


# ------------------------------------------------------------------ the chain LM
@pytest.mark.parametrize('name', sorted(CHAIN_CASES9))
def test_chain_matches_restatement(cuda, name):
    """N = 2 ... 257: both sides of the small-window (16) and fused-loop (96) switches that the information route overrides, up to a
    multi-level plan.  The tolerances are those of tests/test_info_gpu.py (test_robust_gpu._check_against)."""
    prob, O0, O9, lw, (nodes_ref, vels_ref, opt) = chain_case9(name)
    N = CHAIN_CASES9[name][0]
    info = pvgo_info9(O0, O9)
    out = _run(prob, lw, info=info, return_info=True)
    res = out[5]
    res2, trace = _chain_trace(prob, info.packed(N - 1, N - 1, lw, 'cuda'), lw)
    print(name, res.steps, res.trials, ''.join('A' if t[2] else 'r' for t in trace), pattern(opt))
    assert (res2.steps, res2.trials) == (res.steps, res.trials) and res.status == 0
    _check_against(out, res.steps, res.trials, trace, nodes_ref, vels_ref, opt)


def test_todays_paths_are_left_alone(cuda):
    """n9: info=None and a block-diagonal PvgoInfo give what they give without this feature -- None the default loop bit for bit, the
    block-diagonal PvgoInfo the (18,M) route and its restatement; the same matrices as one block-diagonal 9x9 agree with it."""
    prob, _ = chain_problem(9)
    a = _run(prob, UNIT, return_info=True)
    b = _run(prob, UNIT, return_info=True, info=None)
    for x, y in zip(a[:4], b[:4]):
        x = x.tensor() if hasattr(x, 'tensor') else x
        y = y.tensor() if hasattr(y, 'tensor') else y
        assert torch.equal(x.cpu(), y.cpu())
    assert (a[5].steps, a[5].trials, a[5].loss, a[5].damping) == (b[5].steps, b[5].trials, b[5].loss, b[5].damping)
    om = random_omegas(8, 8, UNIT, 109)
    info = pvgo_info(om)
    assert tuple(info.packed(8, 8, UNIT, 'cuda')[1].shape) == (18, 8)
    nodes_ref, vels_ref, opt = run_info(prob, om, UNIT, 'dense')
    out = _run(prob, UNIT, info=info, return_info=True)
    _, trace = _chain_trace(prob, info.packed(8, 8, UNIT, 'cuda'), UNIT)
    _check_against(out, out[5].steps, out[5].trials, trace, nodes_ref, vels_ref, opt)
    out9 = _run(prob, UNIT, info=pvgo_info9(om[0], block_diag9(*om[1:])), return_info=True)
    assert (out9[5].steps, out9[5].trials) == (out[5].steps, out[5].trials)
    assert pose_error(out9[2].tensor().numpy(), out[2].tensor().numpy()).max() < 1e-9
    np.testing.assert_allclose(out9[3].numpy(), out[3].numpy(), atol=1e-9)


def test_covs_under_imu_information(cuda):
    prob, O0, O9, lw, _ = chain_case9('n9')
    covs = _run(prob, lw, info=pvgo_info9(O0, O9))[4]
    tr = lambda m, lo, hi: np.diagonal(m, axis1=1, axis2=2)[:, lo:hi].mean(axis=1)
    want = {'vo_trans': tr(O0, 0, 3), 'vo_rot': tr(O0, 3, 6), 'imu_vel': tr(O9, 0, 3), 'imu_rot': tr(O9, 3, 6), 'transvel': tr(O9, 6, 9)}
    assert sorted(covs) == sorted(want)
    for k in want:
        np.testing.assert_allclose(covs[k], want[k], rtol=1e-15)


# ------------------------------------------------------------------ loop closures
def test_loop_closure_solvers_match_restatement_and_each_other(cuda):
    prob, O0, O9, lw, (nodes_ref, vels_ref, opt) = closure_case9()
    info = pvgo_info9(O0, O9)
    out = {}
    for how in ('dense', 'dense_hip', 'band_pcg'):
        out[how] = _run(prob, lw, info=info, general_solver=how, return_info=True)
        res = out[how][5]
        _check_against(out[how], res['steps'], res['trials'], res['trace'], nodes_ref, vels_ref, opt)
    assert out['band_pcg'][5]['off_band_edges'] == 4
    for how in ('dense_hip', 'band_pcg'):
        np.testing.assert_allclose(out[how][2].tensor().numpy(), out['dense'][2].tensor().numpy(), atol=1e-9)
        np.testing.assert_allclose(out[how][3].numpy(), out['dense'][3].numpy(), atol=1e-9)


# ------------------------------------------------------------------ marginals
def test_chain_marginals_under_imu_information(cuda):
    """n17.  Against numpy's inverse of the restatement's anchored, undamped, unclamped matrix: 1e-8 of the column's largest entry, the
    figure of tests/test_info_gpu.py::test_chain_marginals_under_information."""
    from islam_amd import pvgo
    from tests.test_marginals_gpu import _anchored_inverse, _check_against_dense
    prob, O0, O9, lw, _ = chain_case9('n17')
    info = pvgo_info9(O0, O9)
    out = _run(prob, lw, info=info, marginals=True)
    nodes, vels = out[2].tensor().numpy(), out[3].numpy()
    S = _anchored_inverse(info_matrix9(nodes, vels, prob, O0, O9)[0], 17, 0)
    mg = out[5]
    _check_against_dense(mg.node_cov.cpu().numpy(), mg.cross.cpu().numpy(), S, 1e-8)
    mg2 = pvgo.pvgo_marginals_info(_d(nodes), _d(vels), _d(prob['vo_motions']), _d(prob['dts']), _d(prob['imu_drots']), _d(prob['imu_dtrans']),
                                   _d(prob['imu_dvels']), info, loss_weight=lw)
    _check_against_dense(mg2.node_cov.cpu().numpy(), mg2.cross.cpu().numpy(), S, 1e-8)
    blockdiag = pvgo.pvgo_marginals_info(_d(nodes), _d(vels), _d(prob['vo_motions']), _d(prob['dts']), _d(prob['imu_drots']),
                                         _d(prob['imu_dtrans']), _d(prob['imu_dvels']), pvgo_info([O0] + diag_blocks(O9)), loss_weight=lw)
    assert not torch.allclose(blockdiag.node_cov, mg2.node_cov, rtol=1e-3, atol=0)       # the cross blocks change the answer


@pytest.mark.parametrize('method', ['dense', 'band'])
def test_graph_marginals_under_imu_information(cuda, method):
    """The 33-node closure graph.  Against the restatement's matrix: 1e-8 of the column's largest entry, the figure of
    tests/test_info_gpu.py::test_graph_marginals_under_information."""
    from islam_amd import pvgo
    from tests.test_dense_marginals_gpu import _anchored_inverse, _worst_block_error
    prob, O0, O9, lw, (nodes, vels, _) = closure_case9()
    info = pvgo_info9(O0, O9)
    pairs = np.asarray(prob['links'])
    S = _anchored_inverse(info_matrix9(nodes, vels, prob, O0, O9)[0], 33, 0)
    d = _graph_dev(prob)
    mg = pvgo.pvgo_marginals_general(_d(nodes), _d(vels), d['poses'], d['edges'], d['dts'], d['drots'], d['dtrans'], d['dvels'], loss_weight=lw,
                                     info=info, method=method)
    worst = _worst_block_error(mg.node_cov.cpu().numpy(), pairs, mg.pair_cov.cpu().numpy(), S)
    print('graph marginals (%s) under imu information: worst error / column scale = %.3e' % (method, worst))
    assert worst <= 1e-8


# ------------------------------------------------------------------ IMU covariances end to end
def test_imu_covariances_end_to_end_correlated(cuda):
    """The 9-node tumbling window of tests/test_info_gpu.py::test_imu_covariances_end_to_end (IMU_SEED = 5 meets the margin under
    correlated information too: 5.7e-5; every covariance is positive definite, no floor): ops.imu_preint_cov (motion mode) ->
    PvgoInfo.from_imu_cov(correlated=True) -> run_pvgo, against the restatement fed the same Omega."""
    from islam_amd import ops
    from islam_amd.information import PvgoInfo
    prob, tr = tumbling_problem(9, seed=IMU_SEED)
    seg = np.ascontiguousarray(tr['rgb2imu_sync'], dtype=np.int64)
    cov = ops.imu_preint_cov(_d(tr['imu_dts']), _d(tr['gyros']), _d(tr['accels']), torch.tensor(seg, device='cuda'), seg, IMU_GYRO_COV,
                             IMU_ACC_COV, True)
    assert tuple(cov.shape) == (8, 9, 9)
    rot = np.asarray(prob['init_nodes'], np.float64)[:-1, 3:]
    info = PvgoInfo.from_imu_cov(cov, rot=rot, correlated=True)
    assert info.imu.shape == (8, 9, 9)
    O0 = info.matrices(8, 8, UNIT)[0]
    print('information scale %.2e, largest cross entry %.2e' % (np.abs(info.imu).max(), max(np.abs(info.imu[:, a:a + 3, b:b + 3]).max()
                                                                                         for a, b in ((0, 3), (0, 6), (3, 6)))))
    nodes_ref, vels_ref, opt = run_info9(prob, O0, info.imu, UNIT, 'dense')
    print('imu case', len(opt.trace), 'trials', pattern(opt), 'margin %.2e' % margin(opt))
    assert margin(opt) >= MARGIN
    out = _run(prob, UNIT, info=info, return_info=True)
    res = out[5]
    assert res.status == 0
    _, trace = _chain_trace(prob, info.packed(8, 8, UNIT, 'cuda'), UNIT)
    _check_against(out, res.steps, res.trials, trace, nodes_ref, vels_ref, opt)
    sep = _run(prob, UNIT, info=PvgoInfo.from_imu_cov(cov, rot=rot))
    assert pose_error(out[2].tensor().numpy(), sep[2].tensor().numpy()).max() > 1e-6          # the cross blocks change the answer


# ------------------------------------------------------------------ argument errors
def test_errors(cuda):
    from islam_amd import ops
    from islam_amd._lib import IslamHipError, lib
    from islam_amd.information import PvgoInfo
    from islam_amd.ops import ptr
    from islam_amd.robust import Huber
    prob, O0, O9, lw, _ = chain_case9('n9')
    info = pvgo_info9(O0, O9)
    with pytest.raises(NotImplementedError, match='kernel'):
        _run(prob, info=info, kernel=Huber(0.1))
    with pytest.raises(NotImplementedError, match='reproj'):
        _run(prob, lw=tuple(LW) + (1.0,), info=info, reproj=object())
    with pytest.raises(ValueError, match='imu: 7 factors given, the graph has 8'):
        _run(prob, info=PvgoInfo(imu=O9[:7]))
    with pytest.raises(ValueError, match='imu: 7 factors given'):
        _run(prob, info=PvgoInfo(imu=O9[:7]), general_solver='dense')
    iv, i9 = info.packed(8, 8, lw, 'cuda')
    args = lambda: (_d(prob['vo_motions']), _d(prob['imu_drots']), _d(prob['imu_dtrans']), _d(prob['imu_dvels']), _d(prob['dts']),
                    ops.pvgo_default_params(lw))
    # a 30-row packed array is neither layout
    nodes, vels = _d(prob['init_nodes']), _d(prob['init_vels'])
    before = nodes.clone()
    with pytest.raises(ValueError, match='info_imu'):
        ops.pvgo_run_chain(nodes, vels, *args(), info=(iv, i9[:30].contiguous()))
    with pytest.raises(ValueError, match='info_imu'):
        ops.pvgo_build_normal_info(_device_lin(prob), _d(prob['dts']), 9, None, i9[:30].contiguous())
    with pytest.raises(NotImplementedError):
        ops.pvgo_run_chain(nodes, vels, *args(), info=(iv, i9), robust=object())
    assert torch.equal(nodes, before)
    # the C entry points: exactly one NULL information pointer is an argument error, before any device work
    ws, nbytes = ops.pvgo_workspace(9, nodes.device)
    for pair in ((None, i9), (iv, None)):
        res = ops._lib.PvgoResult()
        a = args()
        rc = lib().islam_pvgo_run_chain_info9(ptr(nodes), ptr(vels), *[ptr(t) for t in a[:5]], 9, ctypes.byref(a[5]), ptr(pair[0]), ptr(pair[1]),
                                              ptr(ws), ctypes.c_size_t(nbytes), ctypes.byref(res), ctypes.c_void_p(0), 0, ctypes.c_void_p(0))
        assert rc == -1 and torch.equal(nodes, before)
    with pytest.raises(IslamHipError) as ei:                                   # through ops: info_vo missing, the (45,M) array given
        ops.pvgo_run_chain(nodes, vels, *args(), info=(None, i9))
    assert ei.value.code == -1 and torch.equal(nodes, before)
    # islam_pvgo_build_normal_info9: a missing info_imu9 or output, N < 2
    lin, dts = _device_lin(prob), _d(prob['dts'])
    Hd, Ho, rhs = (torch.zeros((9, 9, 9), dtype=torch.float64, device='cuda') for _ in range(3))
    build = lib().islam_pvgo_build_normal_info9
    tail = (ctypes.c_double(1e-4), ctypes.c_double(1e32))
    assert build(ptr(lin), ptr(dts), 9, ptr(iv), ptr(None), *tail, ptr(Hd), ptr(Ho), ptr(rhs), ctypes.c_void_p(0)) == -1
    assert build(ptr(lin), ptr(dts), 9, ptr(iv), ptr(i9), *tail, ptr(Hd), ptr(None), ptr(rhs), ctypes.c_void_p(0)) == -1
    assert build(ptr(lin), ptr(dts), 1, ptr(iv), ptr(i9), *tail, ptr(Hd), ptr(Ho), ptr(rhs), ctypes.c_void_p(0)) == -1
    assert not Hd.any() and not Ho.any() and not rhs.any()
    from islam_amd.dist_pvgo import run_chain_sharded
    with pytest.raises(NotImplementedError, match='sharded'):
        run_chain_sharded(None, _d(prob['init_nodes']), _d(prob['init_vels']), None, None, None, None, None, lw, info=info)
