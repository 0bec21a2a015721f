"""Marginal covariances of PVGO poses and velocities on chains (islam_pvgo_marginals: partitioned selected inversion) against
dense / banded CPU inverses of the same matrices."""
import numpy as np
import pytest
import torch

from tests.helpers import chain_problem, reproj_inputs

pytestmark = pytest.mark.gpu

LW = (1, 0.1, 10, 0.1)


def _random_spd(N):
    """The generator of tests/test_pvgo_gpu.py::test_block_tridiagonal_solver (SPD by construction)."""
    rng = np.random.default_rng(N)
    Hd = np.zeros((N, 9, 9))
    Ho = np.zeros((N, 9, 9))
    for k in range(N):
        Hd[k] += np.diag(rng.uniform(0.1, 2.0, 9))
    Jk = rng.normal(size=(max(N - 1, 0), 12, 18))
    for k in range(N - 1):
        JJ = Jk[k].T @ Jk[k]
        Hd[k] += JJ[:9, :9]
        Hd[k + 1] += JJ[9:, 9:]
        Ho[k] = JJ[:9, 9:]
    return Hd, Ho


def _dense(Hd, Ho):
    N = Hd.shape[0]
    A = np.zeros((9 * N, 9 * N))
    for k in range(N):
        A[9 * k:9 * k + 9, 9 * k:9 * k + 9] = Hd[k]
        if k + 1 < N:
            A[9 * k:9 * k + 9, 9 * k + 9:9 * k + 18] = Ho[k]
            A[9 * k + 9:9 * k + 18, 9 * k:9 * k + 9] = Ho[k].T
    return A


def _blocks(S, N):
    Sd = np.stack([S[9 * k:9 * k + 9, 9 * k:9 * k + 9] for k in range(N)])
    So = np.stack([S[9 * k:9 * k + 9, 9 * k + 9:9 * k + 18] for k in range(N - 1)]) if N > 1 else np.zeros((0, 9, 9))
    return Sd, So


def _check_against_dense(Sd, So, S, rtol):
    """|error| <= rtol * (largest entry of the block column of Sigma), for every computed block."""
    N = Sd.shape[0]
    col = np.abs(S).max(axis=0).reshape(N, 9)              # per column of Sigma
    col = np.maximum(col, 1e-300)
    Rd, Ro = _blocks(S, N)
    assert np.all(np.abs(Sd - Rd) <= rtol * col[:, None, :]), np.max(np.abs(Sd - Rd) / col[:, None, :])
    if N > 1:
        assert np.all(np.abs(So - Ro) <= rtol * col[1:, None, :]), np.max(np.abs(So - Ro) / col[1:, None, :])


def _anchored_inverse(A, N, anchor):
    keep = np.ones(9 * N, dtype=bool)
    if anchor is not None:
        keep[9 * anchor:9 * anchor + 6] = False
    S = np.zeros_like(A)
    idx = np.nonzero(keep)[0]
    S[np.ix_(idx, idx)] = np.linalg.inv(A[np.ix_(idx, idx)])
    return S


GRID = [(1, (0, 0)), (2, (0, 0)), (9, (0, 0)), (40, (0, 0)), (41, (0, 0)), (64, (4, 4)), (65, (7, 4)), (100, (9, 0)),
        (257, (0, 0)), (13, (0, 0)), (23, (0, 0)), (47, (0, 0)), (57, (5, 5)), (64, (7, 7)), (500, (6, 5)),
        (1000, (0, 0)), (1000, (4, 4)), (5001, (0, 0)), (5001, (19, 15)), (5003, (24, 6)), (5001, (7, 5)), (30011, (0, 0)),
        (300007, (0, 0))]


@pytest.mark.parametrize('N,seg', GRID)
def test_random_spd_selected_inverse(cuda, N, seg):
    from islam_amd import ops
    import scipy.linalg as sla
    Hd, Ho = _random_spd(N)
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=cuda)
    Hd_d, Ho_d = t(Hd), t(Ho)
    Sd, So = ops.pvgo_marginals(Hd_d, Ho_d, anchor=None, seg_len=seg)
    Sd, So = Sd.cpu().numpy(), So.cpu().numpy()
    assert np.array_equal(Hd_d.cpu().numpy(), Hd) and np.array_equal(Ho_d.cpu().numpy(), Ho)      # inputs untouched
    if 9 * N <= 5000:
        _check_against_dense(Sd, So, np.linalg.inv(_dense(Hd, Ho)), 1e-9)
        return
    # unit columns at the start, the middle, the end and at the segment boundaries of the plan's levels 0 and 1
    plan = ops.pvgo_marginals_plan(N, seg)
    m0 = plan[0][1]
    nodes = {0, 1, N // 2, N - 2, N - 1, m0 - 1, m0, m0 + 1, 2 * m0 + 1}
    if len(plan) > 2:
        m1 = plan[1][1]
        s1 = (m1 + 1) * (m0 + 1) - 1                              # level-0 node of the first level-1 separator
        nodes |= {s1 - 1, s1, s1 + 1}
    nodes = sorted(k for k in nodes if 0 <= k < N)
    cols = sorted({9 * k + i for k in nodes for i in (0, 4, 8)})
    assert len(cols) >= 16
    ab = np.zeros((18, 9 * N))
    for r in range(9):
        for c in range(9):
            if r >= c:
                ab[r - c, c::9] = Hd[:, r, c]
            ab[9 + c - r, r:9 * (N - 1):9] = Ho[:N - 1, r, c]
    E = np.zeros((9 * N, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    X = sla.solveh_banded(ab, E, lower=True)
    for q, j in enumerate(cols):
        k, i = divmod(j, 9)
        x = X[:, q]
        tol = 1e-9 * np.abs(x).max()
        assert np.abs(Sd[k][:, i] - x[9 * k:9 * k + 9]).max() <= tol
        if k > 0:
            assert np.abs(So[k - 1][:, i] - x[9 * k - 9:9 * k]).max() <= tol
        if k + 1 < N:
            assert np.abs(So[k][i, :] - x[9 * k + 9:9 * k + 18]).max() <= tol


def _oracle_A(nodes, vels, prob, lw):
    """A = J^T W J from the oracle's dense PyPose-layout Jacobian, pose column 7 dropped, per node [rho phi v]."""
    from oracle import pvgo as opvgo
    N = nodes.shape[0]
    links = prob['links']
    E, M = N - 1, N - 1
    res = opvgo.residuals(nodes, vels, links, prob['vo_motions'], prob['imu_drots'], prob['imu_dtrans'], prob['imu_dvels'],
                          prob['dts'])
    Ae, Bk = opvgo.jac_blocks(nodes, links, prob['vo_motions'], prob['imu_drots'], res[0], res[2])
    J10 = opvgo.jacobian_dense(N, links, Ae, Bk, prob['dts'])
    cols = np.concatenate([np.concatenate([7 * k + np.arange(6), 7 * N + 3 * k + np.arange(3)]) for k in range(N)])
    J = J10[:, cols]
    w = opvgo.weight_vector(E, M, lw, np.float64)
    return (J.T * w) @ J


def _device_inputs(prob, cuda):
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    return dict(vo_motions=t(prob['vo_motions']), dts=t(prob['dts']), imu_drots=t(prob['imu_drots']),
                imu_dtrans=t(prob['imu_dtrans']), imu_dvels=t(prob['imu_dvels']))


def _solution(prob, cuda, lw):
    from islam_amd import ops
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    nodes, vels = t(prob['init_nodes']), t(prob['init_vels'])
    ops.pvgo_run_chain(nodes, vels, t(prob['vo_motions']), t(prob['imu_drots']), t(prob['imu_dtrans']), t(prob['imu_dvels']),
                       t(prob['dts']), ops.pvgo_default_params(lw))
    return nodes.cpu().numpy(), vels.cpu().numpy()


def _check_against_dd_ref(Sd, So, A, anchor, rtol):
    """|error| <= rtol * (largest entry of the column of Sigma) for every computed block entry in the checked columns (DoF 0, 4, 8 of
    the start, the quarter, the middle, the end, the anchor's neighbours and the level-0 segment boundaries), Sigma's columns from the
    double-double refinement of tests/dd_ref.py: np.linalg.inv of these matrices is itself in error by up to 4e-10 at F = 65 and 1e-8
    at F = 200, the tolerance asserted here."""
    from islam_amd import ops
    from tests import dd_ref
    from tests.test_dd_ref_cpu import checked_columns, checked_nodes
    from tests.test_real_matrix_accuracy_gpu import _errors, _tridiagonal_pieces
    N = Sd.shape[0]
    m0 = ops.pvgo_marginals_plan(N)[0][1]
    cols = checked_columns(checked_nodes(N, anchor, boundaries=(m0 - 1, m0, m0 + 1)), anchor)
    xh, xl, x0 = dd_ref.refine_dense(A, dd_ref.unit_columns(9 * N, cols), anchor=anchor)
    err, floor = _errors(_tridiagonal_pieces(Sd, So, cols), xh, xl, x0)
    print('N=%d anchor=%d: %d columns, worst error / column scale %.3e (LAPACK Cholesky solve: %.3e)' % (N, anchor, cols.size, err.max(), floor.max()))
    assert err.max() <= rtol


@pytest.mark.parametrize('F', [2, 9, 65, 300])
@pytest.mark.parametrize('state', ['initial', 'solution'])
def test_pvgo_matrix_against_oracle(cuda, F, state):
    from islam_amd import pvgo
    prob, _ = chain_problem(F)
    if state == 'initial':
        nodes, vels = np.asarray(prob['init_nodes'], np.float64), np.asarray(prob['init_vels'], np.float64)
    else:
        nodes, vels = _solution(prob, cuda, LW)
    A = _oracle_A(nodes, vels, prob, LW)
    N = F
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    for anchor in sorted({0, N // 2, N - 1}):
        mg = pvgo.pvgo_marginals(t(nodes), t(vels), loss_weight=LW, anchor=anchor, **_device_inputs(prob, cuda))
        Sd, So = mg.node_cov.cpu().numpy(), mg.cross.cpu().numpy()
        if F <= 9:
            _check_against_dense(Sd, So, _anchored_inverse(A, N, anchor), 1e-8)
        else:
            _check_against_dd_ref(Sd, So, A, anchor, 1e-8)
        assert np.all(Sd[anchor][:6, :] == 0) and np.all(Sd[anchor][:, :6] == 0)
        if anchor > 0:
            assert np.all(So[anchor - 1][:, :6] == 0)
        if anchor < N - 1:
            assert np.all(So[anchor][:6, :] == 0)
        assert mg.pose_cov.shape == (N, 6, 6) and mg.vel_cov.shape == (N, 3, 3)
        assert torch.equal(mg.pose_cov, mg.node_cov[:, :6, :6]) and torch.equal(mg.vel_cov, mg.node_cov[:, 6:, 6:])


def test_pvgo_matrix_with_reprojection_factor(cuda):
    from islam_amd import dense_ba, lietensor as pp, pvgo
    from islam_amd.pvgo_dense import _ReprojTerms
    lw5 = (1, 0.1, 10, 0.1, 2.0)
    T_IL = np.array([0.1, -0.05, 0.02, 0.5, -0.5, 0.5, -0.5])
    F = 33
    prob, tr = chain_problem(F)
    inp = reproj_inputs(tr, 40, T_IL)
    th = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    hip = dense_ba.SparseReprojectionLoss(th(inp['points2d']), th(inp['depth']), th(inp['flow']), inp['fx'], inp['fy'], inp['cx'],
                                          inp['cy'], pp.SE3(th(T_IL)), device=cuda)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    nodes, vels = t(prob['init_nodes']), t(prob['init_vels'])
    A = _oracle_A(prob['init_nodes'], prob['init_vels'], prob, lw5)
    terms = _ReprojTerms(nodes, pvgo._reproj_struct(hip, lw5, cuda))
    wS = (terms.w * terms.S).cpu().numpy()
    for k in range(F - 1):
        i, j = 9 * k, 9 * (k + 1)
        A[i:i + 6, i:i + 6] += wS[k]
        A[j:j + 6, j:j + 6] += wS[k]
        A[i:i + 6, j:j + 6] -= wS[k]
        A[j:j + 6, i:i + 6] -= wS[k]
    mg = pvgo.pvgo_marginals(nodes, vels, loss_weight=lw5, reproj=hip, anchor=0, **_device_inputs(prob, cuda))
    S = _anchored_inverse(A, F, 0)
    _check_against_dense(mg.node_cov.cpu().numpy(), mg.cross.cpu().numpy(), S, 1e-8)
    # the factor changes the answer (the test would not notice a dropped term otherwise)
    without = pvgo.pvgo_marginals(nodes, vels, loss_weight=lw5, anchor=0, **_device_inputs(prob, cuda))
    assert not torch.allclose(without.node_cov, mg.node_cov, rtol=1e-3, atol=0)


def test_properties(cuda):
    from islam_amd import pvgo
    F = 300
    prob, _ = chain_problem(F)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    nodes, vels = t(prob['init_nodes']), t(prob['init_vels'])
    mg = pvgo.pvgo_marginals(nodes, vels, loss_weight=LW, **_device_inputs(prob, cuda))
    Sd = mg.node_cov.cpu().numpy()
    assert np.array_equal(Sd, Sd.transpose(0, 2, 1))
    for k in range(F):
        ev = np.linalg.eigvalsh(Sd[k])
        assert ev.min() >= -1e-12 * np.abs(Sd[k]).max()
    # loss weights scaled by c: Sigma scaled by 1 / c^2
    c = 3.0
    mg3 = pvgo.pvgo_marginals(nodes, vels, loss_weight=tuple(c * w for w in LW), **_device_inputs(prob, cuda))
    np.testing.assert_allclose(mg3.node_cov.cpu().numpy() * c * c, Sd, rtol=1e-9, atol=1e-9 * np.abs(Sd).max())
    np.testing.assert_allclose(mg3.cross.cpu().numpy() * c * c, mg.cross.cpu().numpy(), rtol=1e-9,
                               atol=1e-9 * np.abs(Sd).max())
    # drift: anchored at node 0, the position uncertainty grows along the chain
    P = mg.pose_cov.cpu().numpy()
    assert np.trace(P[F - 1][:3, :3]) > np.trace(P[1][:3, :3]) > 0
    # deterministic
    again = pvgo.pvgo_marginals(nodes, vels, loss_weight=LW, **_device_inputs(prob, cuda))
    assert torch.equal(again.node_cov, mg.node_cov) and torch.equal(again.cross, mg.cross)


def test_not_positive_definite(cuda):
    from islam_amd import ops
    from islam_amd._lib import IslamHipError
    z = torch.zeros((1, 9, 9), dtype=torch.float64, device=cuda)
    with pytest.raises(IslamHipError) as e:                   # N = 1: 3 free velocity DoF
        ops.pvgo_marginals(z, z, anchor=0)
    assert e.value.code == -3
    N = 30
    Hd = torch.eye(9, dtype=torch.float64, device=cuda).repeat(N, 1, 1)
    Hd[7, 3, 3] = -1.0
    Ho = torch.zeros((N, 9, 9), dtype=torch.float64, device=cuda)
    before = Hd.clone()
    with pytest.raises(IslamHipError) as e:
        ops.pvgo_marginals(Hd, Ho, anchor=None, seg_len=(4, 4))
    assert e.value.code == -3
    assert torch.equal(Hd, before)
    # stream-ordered form: the status lands on the device, the outputs are zero
    st = torch.zeros((1,), dtype=torch.int32, device=cuda)
    Sd, So = ops.pvgo_marginals(Hd, Ho, anchor=None, seg_len=(4, 4), status=st)
    assert int(st.item()) == -3 and not Sd.any() and not So.any()
    Hd[7, 3, 3] = 1.0
    Sd, So = ops.pvgo_marginals(Hd, Ho, anchor=None, seg_len=(4, 4), status=st)
    assert int(st.item()) == 0
    torch.testing.assert_close(Sd, Hd, rtol=0, atol=1e-15)


def test_run_pvgo_loop_closure_graph_rejects_marginals(cuda):
    from islam_amd import pvgo
    prob, _ = chain_problem(12)
    links = np.asarray(prob['links']).copy()
    links[5] = (0, 7)
    args = {k: v for k, v in prob.items() if k != 'links'}
    with pytest.raises(pvgo.UnsupportedGraphError):
        pvgo.run_pvgo(links=links, device=cuda, loss_weight=LW, marginals=True, **args)


@pytest.mark.parametrize('F', [9, 65])
def test_run_pvgo_marginals_surface(cuda, F):
    from islam_amd import pvgo
    prob, _ = chain_problem(F)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)
    args = dict(init_nodes=t(prob['init_nodes']), init_vels=t(prob['init_vels']), vo_motions=t(prob['vo_motions']),
                links=prob['links'], dts=t(prob['dts']), imu_drots=t(prob['imu_drots']), imu_dtrans=t(prob['imu_dtrans']),
                imu_dvels=t(prob['imu_dvels']))
    base = pvgo.run_pvgo(device=cuda, loss_weight=LW, return_info=True, **args)
    out = pvgo.run_pvgo(device=cuda, loss_weight=LW, return_info=True, marginals=True, **args)
    assert len(out) == len(base) + 1
    for a, b in zip(base[:4], out[:4]):
        assert torch.equal(pp_plain(a).cpu(), pp_plain(b).cpu())
    mg = out[-1]
    assert isinstance(mg, pvgo.PvgoMarginals)
    d = lambda a: a.to(cuda, torch.float64).contiguous()
    ref = pvgo.pvgo_marginals(d(pp_plain(out[2])), d(out[3]), args['vo_motions'], args['dts'], args['imu_drots'],
                              args['imu_dtrans'], args['imu_dvels'], loss_weight=LW)
    assert torch.equal(ref.node_cov, mg.node_cov) and torch.equal(ref.cross, mg.cross)
    assert not mg.pose_cov[0].any()


def pp_plain(x):
    from islam_amd import lietensor as pp
    return pp._plain(x).detach()


def test_bench_configuration(cuda):
    """N = 5001 (bench.py's graph size): the call succeeds at the optimised state and node 0's pose covariance is zero."""
    from islam_amd import pvgo
    F = 5001
    prob, _ = chain_problem(F)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)
    out = pvgo.run_pvgo(t(prob['init_nodes']), t(prob['init_vels']), t(prob['vo_motions']), prob['links'], t(prob['dts']),
                        t(prob['imu_drots']), t(prob['imu_dtrans']), t(prob['imu_dvels']), device=cuda, loss_weight=LW,
                        marginals=True)
    mg = out[-1]
    assert mg.node_cov.shape == (F, 9, 9) and mg.cross.shape == (F - 1, 9, 9)
    assert not mg.pose_cov[0].any()
    assert torch.isfinite(mg.node_cov).all() and torch.isfinite(mg.cross).all()
    v = torch.diagonal(mg.node_cov[1:], dim1=1, dim2=2)
    assert (v > 0).all()
