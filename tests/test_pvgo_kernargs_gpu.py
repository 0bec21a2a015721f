"""bt_eliminate_tw_kernel takes what its first column loads need as flat leading arguments (kernel-argument preload): the previous
level's products as ONE base pointer + 32-bit offsets, the shape of the level, the window of segments.  These tests run the
smallest graphs at which that plumbing can go wrong -- the fused loop just engaged, a short last segment, different segment counts
per level (so different product offsets), four levels, roots of 2, 3, 4 and 6 nodes behind them, and ranks of the sharded loop (a
window of segments that does not start at 0, products of the exchange level in the exchange buffer's packed layout instead of the
workspace's carving)."""
import numpy as np
import pytest
import torch

from tests.helpers import chain_problem
from tests.np_shard_backend import plan_levels

pytestmark = pytest.mark.gpu
LW = (1, 0.1, 10, 0.1)
# (nodes, pinned segment lengths of levels 0 / 1)
CASES = [(97, (0, 0)), (131, (0, 0)), (191, (3, 0)), (191, (7, 0)), (1001, (0, 0))]


def _args(F, cuda):
    prob, _ = chain_problem(F)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    return [t(prob[k]) for k in ('init_nodes', 'init_vels', 'vo_motions', 'imu_drots', 'imu_dtrans', 'imu_dvels', 'dts')]


@pytest.fixture(scope='module')
def fused():
    """(F, seg) -> (nodes, vels, result, trace) of the single-GPU fused loop on the case: computed once per case with
    ISLAM_PVGO_NO_FUSE cleared, whatever the calling test has set, shared by the tests of this module (which do not modify it) and
    released with the module"""
    from islam_amd import ops
    done = {}

    def run(F, seg):
        if (F, seg) not in done:
            with pytest.MonkeyPatch.context() as mp:
                mp.delenv('ISLAM_PVGO_NO_FUSE', raising=False)
                args = _args(F, torch.device('cuda:0'))
                nodes, vels = args[0].clone(), args[1].clone()
                res, trace = ops.pvgo_run_chain(nodes, vels, *args[2:], ops.pvgo_default_params(LW, radius=1e4, seg_len=seg), trace_cap=256)
            done[(F, seg)] = (nodes, vels, res, np.asarray(trace)[:res.trials])
        return done[(F, seg)]
    yield run
    done.clear()


def test_the_cases_cover_the_plans_they_are_meant_to():
    plans = {c: plan_levels(c[0], c[1], twisted=True) for c in CASES}
    # (nodes, segment length, segments) per level: roots of 2, 3, 6, 3 and 4 nodes -- the three-node root that never leaves its
    # workgroup and the ones that do; last segments of 1, 5 (no right separator), 1 and 7 nodes; 39 against 24 level-0 segments on the
    # same graph, so different product offsets; four levels
    assert plans[(97, (0, 0))] == [(97, 5, 17), (16, 5, 3), (2, 2, 1)]
    assert plans[(131, (0, 0))] == [(131, 5, 22), (21, 5, 4), (3, 3, 1)]
    assert plans[(191, (3, 0))] == [(191, 4, 39), (38, 5, 7), (6, 6, 1)]
    assert plans[(191, (7, 0))] == [(191, 7, 24), (23, 5, 4), (3, 3, 1)]
    assert plans[(1001, (0, 0))] == [(1001, 5, 167), (166, 5, 28), (27, 5, 5), (4, 4, 1)]
    assert all(F > 96 and lv[0][1] <= 7 for (F, _), lv in plans.items())      # the fused loop engages: more than 96 nodes, segments its LDS holds


@pytest.mark.parametrize('F,seg', CASES)
def test_fused_loop_equals_the_launch_per_stage_loop(cuda, fused, F, seg, monkeypatch):
    from islam_amd import ops
    n1, v1, r1, t1 = fused(F, seg)
    monkeypatch.setenv('ISLAM_PVGO_NO_FUSE', '1')
    args = _args(F, cuda)
    n0, v0 = args[0].clone(), args[1].clone()
    r0, t0 = ops.pvgo_run_chain(n0, v0, *args[2:], ops.pvgo_default_params(LW, radius=1e4, seg_len=seg), trace_cap=256)
    t0 = np.asarray(t0)[:r0.trials]
    assert (r1.trials, r1.steps, r1.status) == (r0.trials, r0.steps, r0.status)
    np.testing.assert_array_equal(t1[:, 2], t0[:, 2])                       # accept / reject pattern
    np.testing.assert_allclose(t1[:, 1], t0[:, 1], rtol=1e-12)              # dampings
    np.testing.assert_allclose(t1[:, 0], t0[:, 0], rtol=1e-9)               # trial losses
    np.testing.assert_allclose(n1.cpu().numpy(), n0.cpu().numpy(), rtol=0, atol=1e-8)
    np.testing.assert_allclose(v1.cpu().numpy(), v0.cpu().numpy(), rtol=0, atol=1e-8)


@pytest.mark.parametrize('N,seg', CASES)
def test_solve_chain_against_the_banded_solve(cuda, N, seg):
    """islam_pvgo_solve_chain (level 0 from the caller's arrays, the upper levels and the down-sweep's root from carved products) vs
    the banded Cholesky solve the oracle's LM uses, on a random SPD block-tridiagonal system."""
    from islam_amd import ops
    import scipy.linalg as sla
    rng = np.random.default_rng(N)
    Hd = np.zeros((N, 9, 9))
    Ho = np.zeros((N, 9, 9))
    for k in range(N):
        Hd[k] += np.diag(rng.uniform(0.1, 2.0, 9))
    Jk = rng.normal(size=(N - 1, 12, 18))
    for k in range(N - 1):
        JJ = Jk[k].T @ Jk[k]
        Hd[k] += JJ[:9, :9]
        Hd[k + 1] += JJ[9:, 9:]
        Ho[k] = JJ[:9, 9:]
    rhs = rng.normal(size=(N, 9))
    damping = 0.37
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=cuda)
    dx = ops.pvgo_solve_chain(t(Hd), t(Ho), t(rhs), damping, seg_len=seg).cpu().numpy()
    ab = np.zeros((18, 9 * N))
    for r in range(9):
        for c in range(9):
            if r >= c:
                ab[r - c, c::9] = Hd[:, r, c] * ((1 + damping) if r == c else 1.0)
            ab[9 + c - r, r:9 * (N - 1):9] = Ho[:N - 1, r, c]
    ref = sla.solveh_banded(ab, rhs.reshape(-1), lower=True).reshape(N, 9)
    assert np.abs(dx - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('F,seg', CASES)
def test_ranks_as_threads_equal_the_single_gpu_loop(cuda, fused, F, seg, world):
    """every rank's window of segments starts behind the chain's first one and its arrays are local"""
    from islam_amd import ops
    from tests.test_dist_c_gpu import _run_ranks_as_threads
    nodes, vels, res, _ = fused(F, seg)
    outs = _run_ranks_as_threads(_args(F, cuda), world, params=ops.pvgo_default_params(LW, radius=1e4, seg_len=seg))
    for r, (n, v, rr, xb) in enumerate(outs):
        assert (rr.trials, rr.steps, rr.status) == (res.trials, res.steps, 0), r
        torch.testing.assert_close(n, nodes, rtol=0, atol=1e-9)
        torch.testing.assert_close(v, vels, rtol=0, atol=1e-9)
