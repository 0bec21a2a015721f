"""Per-factor information matrices on the MI355X (run_pvgo(info=...)): info_build_kernel and the dense information
kernels against numpy evaluations of the contract, the chain loop (islam_pvgo_run_chain_info) and the three general-topology solvers
against the float64 restatement of tests/test_info_cpu.py, the marginals under information, IMU pre-integration covariances end to end,
the default path left alone and the argument errors."""
import numpy as np
import pytest
import torch

from oracle import pvgo as opvgo
from tests.helpers import chain_problem, tumbling_problem
from tests.test_info_cpu import (CHAIN_CASES, LONG_EDGES, LW, MARGIN, UNIT, _inputs, chain_case, closure_case, margin, pattern,
                                 pvgo_info, random_omegas, run_info, scalar_omegas)
from tests.test_robust_gpu import _check_against, _run
from tests.test_robust_cpu import pose_error

pytestmark = pytest.mark.gpu


def _d(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')


# ------------------------------------------------------------------ assembly
def _device_lin(prob):
    from islam_amd import ops
    lin, _ = ops.pvgo_linearize(_d(prob['init_nodes']), _d(prob['init_vels']), _d(prob['vo_motions']), _d(prob['imu_drots']),
                                _d(prob['imu_dtrans']), _d(prob['imu_dvels']), _d(prob['dts']))
    return lin


def _contract(lin, dts, om, vmin, vmax):
    """The contract's per-link table in numpy from a `lin` record (42,M); om[0] None: no VO group."""
    M = lin.shape[1]
    N = M + 1
    m3 = lambda r: lin[r:r + 9].T.reshape(M, 3, 3)
    T = lambda a: np.swapaxes(a, 1, 2)
    mv = lambda a, v: (a @ v[:, :, None])[:, :, 0]
    e, G, C, er, B, rv, rt = lin[0:6].T, m3(6), m3(15), lin[24:27].T, m3(27), lin[36:39].T, lin[39:42].T
    O0, O1, O2, O3 = om
    S = np.zeros((M, 6, 6))
    gp = np.zeros((M, 6))
    if O0 is not None:
        A = np.zeros((M, 6, 6))
        A[:, :3, :3], A[:, :3, 3:], A[:, 3:, 3:] = G, C, G
        S += T(A) @ O0 @ A
        gp += mv(T(A) @ O0, e)
    S[:, :3, :3] += O3
    S[:, 3:, 3:] += T(B) @ O2 @ B
    gp[:, :3] += mv(O3, rt)
    gp[:, 3:] += mv(T(B) @ O2, er)
    Hd, Ho, g = np.zeros((N, 9, 9)), np.zeros((N, 9, 9)), np.zeros((N, 9))
    Hd[:-1, :6, :6] += S
    Hd[1:, :6, :6] += S
    Ho[:-1, :6, :6] = -S
    Hd[:-1, 6:, 6:] += O1 + (dts * dts)[:, None, None] * O3
    Hd[1:, 6:, 6:] += O1
    Ho[:-1, 6:, 6:] = -O1
    c = dts[:, None, None] * O3
    Hd[:-1, 0:3, 6:9] += c
    Hd[:-1, 6:9, 0:3] += c
    Ho[:-1, 6:9, 0:3] = -c
    g[1:, :6] += gp
    g[:-1, :6] -= gp
    g[:-1, 6:] += mv(O1, rv) - dts[:, None] * mv(O3, rt)
    g[1:, 6:] -= mv(O1, rv)
    i = np.arange(9)
    Hd[:, i, i] = np.clip(Hd[:, i, i], vmin, vmax)
    return Hd, Ho, -g


def _assert_blocks(got, want, what):
    """Entrywise error <= 1e-12 x the largest absolute entry of the same block (row of rhs).  Each entry sums fewer than 200 fp64
    products: gamma_200 = 4.4e-14 on sum |terms|, and with cond(Omega) <= 16 sum |terms| stays within a small multiple of the block's
    largest entry."""
    got, want = [np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for x in (got, want)]
    scale = np.abs(want).reshape(want.shape[0], -1).max(axis=1).reshape((-1,) + (1,) * (want.ndim - 1))
    err = np.abs(got - want)
    print('%s: worst error / block scale = %.2e' % (what, (err / np.maximum(scale, 1e-300)).max()))
    assert np.all(err <= 1e-12 * scale), what


def _build_info(lin, dts, N, om, vmin=1e-4, vmax=1e32):
    from islam_amd import ops
    from islam_amd.information import PvgoInfo
    info = PvgoInfo(vo=om[0], vel=om[1], rot=om[2], transvel=om[3])
    iv, ii = info.packed(N - 1, N - 1, UNIT, 'cuda')
    return ops.pvgo_build_normal_info(lin, dts, N, iv if om[0] is not None else None, ii, vmin, vmax)


@pytest.mark.parametrize('N', [2, 3, 64, 65, 130])
def test_build_normal_info(cuda, N):
    """One link, both ends, a full wave, a wave plus one lane, three workgroups."""
    from islam_amd import ops
    prob, _ = chain_problem(N)
    lin = _device_lin(prob)
    lin_h, dts_h, dts = lin.cpu().numpy(), np.asarray(prob['dts'], dtype=np.float64), _d(prob['dts'])
    om = random_omegas(N - 1, N - 1, LW, 100 + N)
    got = _build_info(lin, dts, N, om)
    for g, w, what in zip(got, _contract(lin_h, dts_h, om, 1e-4, 1e32), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s against the contract, N=%d' % (what, N))
    assert torch.equal(got[0], got[0].transpose(1, 2))                       # exactly symmetric node blocks
    # Omega = w I is islam_pvgo_build_normal
    w4 = [x ** 2 for x in LW]
    for g, w, what in zip(_build_info(lin, dts, N, scalar_omegas(N - 1, N - 1, LW)), ops.pvgo_build_normal(lin, dts, N, w4), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s with w I against build_normal, N=%d' % (what, N))
    # no VO group = the w0 = 0 call
    om_s = scalar_omegas(N - 1, N - 1, LW)
    novo = _build_info(lin, dts, N, [None] + om_s[1:])
    for g, w, what in zip(novo, ops.pvgo_build_normal(lin, dts, N, [0.0] + w4[1:]), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s without VO against w0 = 0, N=%d' % (what, N))
    # Omega = 0 on one link: that link's scalar-zero result (robust multipliers 0 on its three IMU factors, w0 = 0)
    k = (N - 1) // 2
    om_z = [None] + [o.copy() for o in om_s[1:]]
    for o in om_z[1:]:
        o[k] = 0.0
    c_imu = torch.ones((3, N - 1), dtype=torch.float64, device='cuda')
    c_imu[:, k] = 0.0
    for g, w, what in zip(_build_info(lin, dts, N, om_z), ops.pvgo_build_normal(lin, dts, N, [0.0] + w4[1:], c_imu=c_imu), ('Hd', 'Ho', 'rhs')):
        _assert_blocks(g, w, '%s with link %d switched off, N=%d' % (what, k, N))
    if N == 2:                                                              # every factor off: only the clamp is left
        Hd, Ho, rhs = _build_info(lin, dts, N, [np.zeros_like(o) for o in om])
        assert torch.equal(Hd, 1e-4 * torch.eye(9, dtype=torch.float64, device='cuda').expand(2, 9, 9)) and not rhs.any() and not Ho.any()
    # the clamp
    Hd, Ho, rhs = _build_info(lin, dts, N, om, vmin=5.0, vmax=6.0)
    dg = Hd.diagonal(dim1=1, dim2=2)
    assert float(dg.min()) >= 5.0 and float(dg.max()) <= 6.0
    want = _contract(lin_h, dts_h, om, 5.0, 6.0)
    _assert_blocks(Hd, want[0], 'Hd clamped to [5, 6], N=%d' % N)
    assert torch.equal(Ho, got[1]) and torch.equal(rhs, got[2])


def info_matrix(nodes, vels, prob, om):
    """A = sum J^T Omega J (9N x 9N, per node [rho phi v]) and b = -sum J^T Omega r of the restatement at (nodes, vels)."""
    from tests.test_info_cpu import _DenseLinInfo
    _, _, inp = _inputs(prob)
    N = nodes.shape[0]
    res = opvgo.residuals(nodes, vels, *inp)
    A_e, B_k = opvgo.jac_blocks(nodes, inp[0], inp[1], inp[2], res[0], res[2])
    lin = _DenseLinInfo(nodes, inp, res, A_e, B_k, om)
    cols = np.concatenate([np.concatenate([7 * k + np.arange(6), 7 * N + 3 * k + np.arange(3)]) for k in range(N)])
    return lin.A[np.ix_(cols, cols)], lin.b[cols]


def _graph_dev(prob):
    return dict(nodes=_d(prob['init_nodes']), vels=_d(prob['init_vels']), edges=torch.tensor(np.asarray(prob['links']), dtype=torch.int64, device='cuda'),
                poses=_d(prob['vo_motions']), drots=_d(prob['imu_drots']), dtrans=_d(prob['imu_dtrans']), dvels=_d(prob['imu_dvels']), dts=_d(prob['dts']))


def test_dense_assembly_on_the_closure_graph(cuda):
    from islam_amd.pvgo_dense import _DenseSystem, _Graph
    prob, om, lw, _ = closure_case()
    d = _graph_dev(prob)
    packed = pvgo_info(om).packed(32, 32, lw, 'cuda')
    g = _Graph(d['nodes'], d['edges'], d['poses'], d['drots'], d['dtrans'], d['dvels'], d['dts'], lw, packed)
    sysm = _DenseSystem(g)
    vo, lin = g.linearize(d['nodes'], d['vels'])
    sysm.fill(vo, lin)
    A, b = info_matrix(np.asarray(prob['init_nodes'], np.float64), np.asarray(prob['init_vels'], np.float64), prob, om)
    np.testing.assert_allclose(sysm.A.cpu().numpy(), A, rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(sysm.b.cpu().numpy(), b, rtol=1e-8, atol=1e-8)
    first = sysm.A.clone()
    sysm.fill(vo, lin)                                   # (no two edges of this graph share a node pair: one atomic per entry, same bits)
    assert torch.equal(first, sysm.A)


# ------------------------------------------------------------------ the chain LM
def _chain_trace(prob, packed, lw):
    from islam_amd import ops
    nodes, vels = _d(prob['init_nodes']), _d(prob['init_vels'])
    return ops.pvgo_run_chain(nodes, vels, _d(prob['vo_motions']), _d(prob['imu_drots']), _d(prob['imu_dtrans']), _d(prob['imu_dvels']),
                              _d(prob['dts']), ops.pvgo_default_params(lw), trace_cap=256, info=packed)


@pytest.mark.parametrize('name', sorted(CHAIN_CASES))
def test_chain_matches_restatement(cuda, name):
    """N = 2, 9, 17, 130, 257: both sides of the small-window (16) and fused-loop (96) switches of the driver, up to a multi-level plan."""
    prob, om, lw, (nodes_ref, vels_ref, opt) = chain_case(name)
    N = CHAIN_CASES[name][0]
    info = pvgo_info(om)
    out = _run(prob, lw, info=info, return_info=True)
    res = out[5]
    res2, trace = _chain_trace(prob, info.packed(N - 1, N - 1, lw, 'cuda'), lw)
    print(name, res.steps, res.trials, ''.join('A' if t[2] else 'r' for t in trace), pattern(opt))
    assert (res2.steps, res2.trials) == (res.steps, res.trials) and res.status == 0
    _check_against(out, res.steps, res.trials, trace, nodes_ref, vels_ref, opt)


@pytest.mark.parametrize('N', [9, 130])
def test_scalar_information_is_the_default_lm(cuda, N):
    from islam_amd.information import PvgoInfo
    prob, _ = chain_problem(N)
    a = _run(prob, LW, return_info=True)
    om = scalar_omegas(N - 1, N - 1, LW)
    for info in (PvgoInfo(), pvgo_info(om)):                                  # None groups are filled with loss_weight^2 I
        b = _run(prob, LW, return_info=True, info=info)
        assert (b[5].steps, b[5].trials) == (a[5].steps, a[5].trials)
        assert pose_error(b[2].tensor().numpy(), a[2].tensor().numpy()).max() < 1e-9
        np.testing.assert_allclose(b[3].numpy(), a[3].numpy(), atol=1e-9)
        for key in a[4]:
            np.testing.assert_allclose(b[4][key], a[4][key], rtol=1e-14)
    ta = _chain_trace(prob, None, LW)[1]
    tb = _chain_trace(prob, pvgo_info(om).packed(N - 1, N - 1, LW, 'cuda'), LW)[1]
    assert [t[2] for t in ta] == [t[2] for t in tb]


def test_info_none_is_the_code_path_of_today(cuda):
    prob, _ = chain_problem(130)
    a = _run(prob, return_info=True)
    b = _run(prob, return_info=True, info=None)
    for x, y in zip(a[:4], b[:4]):
        x = x.tensor() if hasattr(x, 'tensor') else x
        y = y.tensor() if hasattr(y, 'tensor') else y
        assert torch.equal(x.cpu(), y.cpu())
    assert (a[5].steps, a[5].trials, a[5].loss, a[5].damping) == (b[5].steps, b[5].trials, b[5].loss, b[5].damping)
    assert all(np.array_equal(a[4][k], b[4][k]) for k in a[4])


def test_covs_under_information(cuda):
    prob, om, lw, _ = chain_case('n9')
    covs = _run(prob, lw, info=pvgo_info(om))[4]
    tr = lambda m, lo, hi: np.diagonal(m, axis1=1, axis2=2)[:, lo:hi].mean(axis=1)
    want = {'vo_trans': tr(om[0], 0, 3), 'vo_rot': tr(om[0], 3, 6), 'imu_vel': tr(om[1], 0, 3), 'imu_rot': tr(om[2], 0, 3),
            'transvel': tr(om[3], 0, 3)}
    assert sorted(covs) == sorted(want)
    for k in want:
        np.testing.assert_allclose(covs[k], want[k], rtol=1e-15)


# ------------------------------------------------------------------ loop closures
@pytest.mark.parametrize('zero_long', [False, True])
def test_loop_closure_solvers_match_restatement_and_each_other(cuda, zero_long):
    """zero_long: Omega = 0 on the four long edges; the restatement has their rows taken out of the normal equations."""
    prob, om, lw, (nodes_ref, vels_ref, opt) = closure_case(zero_long)
    info = pvgo_info(om)
    out = {}
    for how in ('dense', 'dense_hip', 'band_pcg'):
        out[how] = _run(prob, lw, info=info, general_solver=how, return_info=True)
        res = out[how][5]
        _check_against(out[how], res['steps'], res['trials'], res['trace'], nodes_ref, vels_ref, opt)
    assert out['band_pcg'][5]['off_band_edges'] == len(LONG_EDGES)
    for how in ('dense_hip', 'band_pcg'):
        np.testing.assert_allclose(out[how][2].tensor().numpy(), out['dense'][2].tensor().numpy(), atol=1e-9)
        np.testing.assert_allclose(out[how][3].numpy(), out['dense'][3].numpy(), atol=1e-9)


# ------------------------------------------------------------------ marginals
def test_chain_marginals_under_information(cuda):
    """Against numpy's inverse of the restatement's anchored, undamped, unclamped matrix: 1e-8 of the column's largest entry, the
    figure of tests/test_marginals_gpu.py::test_pvgo_matrix_against_oracle."""
    from islam_amd import pvgo
    from tests.test_marginals_gpu import _anchored_inverse, _check_against_dense
    prob, om, lw, _ = chain_case('n9')
    info = pvgo_info(om)
    out = _run(prob, lw, info=info, marginals=True)
    nodes, vels = out[2].tensor().numpy(), out[3].numpy()
    S = _anchored_inverse(info_matrix(nodes, vels, prob, om)[0], 9, 0)
    mg = out[5]
    _check_against_dense(mg.node_cov.cpu().numpy(), mg.cross.cpu().numpy(), S, 1e-8)
    mg2 = pvgo.pvgo_marginals_info(_d(nodes), _d(vels), _d(prob['vo_motions']), _d(prob['dts']), _d(prob['imu_drots']), _d(prob['imu_dtrans']),
                                   _d(prob['imu_dvels']), info, loss_weight=lw)
    _check_against_dense(mg2.node_cov.cpu().numpy(), mg2.cross.cpu().numpy(), S, 1e-8)
    plain = _run(prob, lw, marginals=True)[5]
    assert not torch.allclose(plain.node_cov, mg.node_cov, rtol=1e-3, atol=0)        # the information changes the answer


def test_graph_marginals_under_information(cuda):
    """dense_hip on the 33-node graph.  Against the restatement's matrix: 1e-8 of the column's largest entry, as for the chain; against
    the device's own assembled matrix: 1e-9, the figure of tests/test_dense_marginals_gpu.py::test_loop_closures_against_numpy."""
    from islam_amd import pvgo
    from islam_amd.pvgo_dense import gauss_newton_matrix
    from tests.test_dense_marginals_gpu import _anchored_inverse, _worst_block_error
    prob, om, lw, _ = closure_case()
    info = pvgo_info(om)
    out = _run(prob, lw, info=info, general_solver='dense_hip', marginals=True)
    nodes, vels = out[2].tensor().numpy(), out[3].numpy()
    mg = out[5]
    assert isinstance(mg, pvgo.PvgoGraphMarginals)
    pairs = np.asarray(prob['links'])
    S = _anchored_inverse(info_matrix(nodes, vels, prob, om)[0], 33, 0)
    worst = _worst_block_error(mg.node_cov.cpu().numpy(), pairs, mg.pair_cov.cpu().numpy(), S)
    d = _graph_dev(prob)
    A = gauss_newton_matrix(_d(nodes), _d(vels), d['edges'], d['poses'], d['drots'], d['dtrans'], d['dvels'], d['dts'], lw,
                            info=info.packed(32, 32, lw, 'cuda')).cpu().numpy()
    S_dev = _anchored_inverse(np.triu(A) + np.triu(A, 1).T, 33, 0)
    worst_dev = _worst_block_error(mg.node_cov.cpu().numpy(), pairs, mg.pair_cov.cpu().numpy(), S_dev)
    print('graph marginals under information: worst error / column scale = %.3e (restatement), %.3e (device matrix)' % (worst, worst_dev))
    assert worst <= 1e-8 and worst_dev <= 1e-9
    mg2 = pvgo.pvgo_marginals_general(_d(nodes), _d(vels), d['poses'], d['edges'], d['dts'], d['drots'], d['dtrans'], d['dvels'], loss_weight=lw,
                                      info=info)
    assert _worst_block_error(mg2.node_cov.cpu().numpy(), pairs, mg2.pair_cov.cpu().numpy(), S) <= 1e-8


# ------------------------------------------------------------------ IMU covariances end to end
IMU_SEED = 5
IMU_GYRO_COV, IMU_ACC_COV = 1e-2, 1.0      # per-sample variances of a consumer-grade IMU at 100 Hz, (rad/s)^2 and (m/s^2)^2


def test_imu_covariances_end_to_end(cuda):
    """A 9-node tumbling window: ops.imu_preint_cov (motion mode) -> PvgoInfo.from_imu_cov -> run_pvgo, against the restatement fed the
    same Omega.  The CPU half asserts the input condition of this case."""
    from islam_amd import ops
    from islam_amd.information import PvgoInfo
    prob, tr = tumbling_problem(9, seed=IMU_SEED)
    seg = np.ascontiguousarray(tr['rgb2imu_sync'], dtype=np.int64)
    cov = ops.imu_preint_cov(_d(tr['imu_dts']), _d(tr['gyros']), _d(tr['accels']), torch.tensor(seg, device='cuda'), seg, IMU_GYRO_COV,
                             IMU_ACC_COV, True)
    assert tuple(cov.shape) == (8, 9, 9)
    info = PvgoInfo.from_imu_cov(cov, rot=np.asarray(prob['init_nodes'], np.float64)[:-1, 3:])
    om = info.matrices(8, 8, UNIT)
    print('information scales: rot %.2e, vel %.2e, transvel %.2e' % tuple(np.abs(m).max() for m in om[1:]))
    nodes_ref, vels_ref, opt = run_info(prob, om, UNIT, 'dense')
    print('imu case', len(opt.trace), 'trials', pattern(opt), 'margin %.2e' % margin(opt))
    assert margin(opt) >= MARGIN
    out = _run(prob, UNIT, info=info, return_info=True)
    res = out[5]
    assert res.status == 0
    _, trace = _chain_trace(prob, info.packed(8, 8, UNIT, 'cuda'), UNIT)
    _check_against(out, res.steps, res.trials, trace, nodes_ref, vels_ref, opt)
    plain = _run(prob, UNIT)
    assert pose_error(out[2].tensor().numpy(), plain[2].tensor().numpy()).max() > 1e-6        # the covariances change the answer


# ------------------------------------------------------------------ argument errors
def test_errors(cuda):
    from islam_amd import ops
    from islam_amd._lib import IslamHipError
    from islam_amd.information import PvgoInfo
    from islam_amd.robust import Huber
    prob, om, lw, _ = chain_case('n9')
    info = pvgo_info(om)
    with pytest.raises(NotImplementedError, match='kernel'):
        _run(prob, info=info, kernel=Huber(0.1))
    with pytest.raises(NotImplementedError, match='reproj'):
        _run(prob, lw=tuple(LW) + (1.0,), info=info, reproj=object())
    with pytest.raises(TypeError):
        _run(prob, info=om)
    with pytest.raises(TypeError):
        _run(prob, info=(1.0, 1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match='vo: 7 factors given, the graph has 8'):
        _run(prob, info=PvgoInfo(vo=om[0][:7]))
    with pytest.raises(ValueError, match='rot: 7 factors given'):
        _run(prob, info=PvgoInfo(rot=om[2][:7]), general_solver='dense')
    # the C entry point: exactly one NULL information pointer is an argument error, before any device work
    iv, ii = info.packed(8, 8, lw, 'cuda')
    for pair in ((None, ii), (iv, None)):
        nodes, vels = _d(prob['init_nodes']), _d(prob['init_vels'])
        before = nodes.clone()
        with pytest.raises(IslamHipError) as ei:
            ops.pvgo_run_chain(nodes, vels, _d(prob['vo_motions']), _d(prob['imu_drots']), _d(prob['imu_dtrans']), _d(prob['imu_dvels']),
                               _d(prob['dts']), ops.pvgo_default_params(lw), info=pair)
        assert ei.value.code == -1 and torch.equal(nodes, before)
    with pytest.raises(ValueError):
        ops.pvgo_run_chain(_d(prob['init_nodes']), _d(prob['init_vels']), _d(prob['vo_motions']), _d(prob['imu_drots']), _d(prob['imu_dtrans']),
                           _d(prob['imu_dvels']), _d(prob['dts']), ops.pvgo_default_params(lw), info=(iv[:, :7].contiguous(), ii))
    with pytest.raises(NotImplementedError):
        ops.pvgo_run_chain(_d(prob['init_nodes']), _d(prob['init_vels']), _d(prob['vo_motions']), _d(prob['imu_drots']), _d(prob['imu_dtrans']),
                           _d(prob['imu_dvels']), _d(prob['dts']), ops.pvgo_default_params(lw), info=(iv, ii), robust=object())
    from islam_amd.dist_pvgo import run_chain_sharded
    with pytest.raises(NotImplementedError, match='sharded'):
        run_chain_sharded(None, _d(prob['init_nodes']), _d(prob['init_vels']), None, None, None, None, None, lw, info=info)
