"""The LM loops that inline the pose-graph link and the retraction of lie_dev.h, against the launch-per-stage loop on the 3-D
large-angle geometry of tests/golden/lie_cases.npz (residual angles across every series / closed-form switch up to pi - 1e-6, residual
translations up to 5 m, composed quaternions with w < 0): the fused loop (trial_elim_kernel states the link through vo_link, the
function linbuild_kernel and trial_lin_kernel call) at N = 97, the smallest graph it takes, and N = 201, the whole file; the one-launch
small-graph loop (small_lm_kernel) at N = 9.  Same accept / reject pattern, iterate within atol = 1e-8 -- the bound
test_pvgo_gpu.py::test_fused_loop_equals_the_launch_per_stage_loop_on_reject_heavy_graphs uses for the same comparison.  The values
themselves are held to the 50-digit reference by tests/test_lie_gpu.py.  Every test is two small runs."""
import numpy as np
import pytest
import torch

from tests.golden import make_lie_golden as gen

pytestmark = pytest.mark.gpu
LW = (1, 0.1, 10, 0.1)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(gen.PATH))


def _run_both(z, N, cuda, monkeypatch, switch):
    """run_pvgo on the first N nodes of the file, with the environment switch (read per call) on and off"""
    from islam_amd import ops
    prm = ops.pvgo_default_params(LW, radius=1e4)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=cuda)
    outs = []
    for off in ('1', '0'):
        monkeypatch.setenv(switch, off)
        nodes, vels = t(z['nodes'][:N]), t(z['vels'][:N])
        args = [t(z[k][:N - 1]) for k in ('poses', 'drots', 'dtrans', 'dvels', 'dts')]
        res, trace = ops.pvgo_run_chain(nodes, vels, *args, prm, trace_cap=256)
        outs.append((res, np.asarray(trace)[:res.trials], nodes.cpu().numpy(), vels.cpu().numpy()))
    return outs


def _same(outs):
    (r0, t0, n0, v0), (r1, t1, n1, v1) = outs
    print('trials %d / %d  steps %d / %d  status %d / %d  accept pattern %s' % (r0.trials, r1.trials, r0.steps, r1.steps, r0.status, r1.status,
                                                                            ''.join(str(int(a)) for a in t0[:, 2])))
    print('max |nodes - nodes| = %.3e  max |vels - vels| = %.3e' % (np.abs(n1 - n0).max(), np.abs(v1 - v0).max()))
    assert (r1.trials, r1.steps, r1.status) == (r0.trials, r0.steps, r0.status)
    np.testing.assert_array_equal(t1[:, 2], t0[:, 2])                       # accept / reject pattern
    assert np.isfinite(n0).all() and np.isfinite(v0).all()
    np.testing.assert_allclose(n1, n0, rtol=0, atol=1e-8)
    np.testing.assert_allclose(v1, v0, rtol=0, atol=1e-8)


@pytest.mark.parametrize('N', [97, 201])
def test_fused_loop_equals_the_launch_per_stage_loop_on_large_angles(cuda, gold, monkeypatch, N):
    _same(_run_both(gold, N, cuda, monkeypatch, 'ISLAM_PVGO_NO_FUSE'))


def test_small_graph_loop_equals_the_launch_per_stage_loop_on_large_angles(cuda, gold, monkeypatch):
    _same(_run_both(gold, 9, cuda, monkeypatch, 'ISLAM_PVGO_NO_SMALL'))
