"""The PVGO kernels that take their geometry from islam_amd/csrc/lie_dev.h, on 3-D large-angle cases, against the 60-digit reference
in tests/golden/lie_cases.npz (tests/golden/make_lie_golden.py): general rotation axes, residual angles from 0 across every series /
closed-form switch up to pi - 1e-6, composed quaternions with w < 0, residual translations up to 5 m.  Error of a case =
max|x - ref| / max(1, max|ref|); the tolerance per quantity is stored in the file: 16 x the rounding floor of the same formulas in
NumPy float64, measured and mutation-checked by tests/test_lie_golden_cpu.py (between 4e-15 and 4e-13 -- and exactly 0 for the
retracted velocities, one correctly rounded addition).  Every test is one small launch."""
import numpy as np
import pytest
import torch

from tests.golden import make_lie_golden as gen

pytestmark = pytest.mark.gpu
LW = (1, 0.1, 10, 0.1)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(gen.PATH))


def _t(a, cuda, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=cuda)


def _chain(z, cuda):
    return tuple(_t(z[k], cuda) for k in ('nodes', 'vels', 'poses', 'drots', 'dtrans', 'dvels', 'dts'))


def _check(z, out, names):
    errs = gen.case_errors(z, out)
    tol = dict(zip(z['quantities'], z['tolerances']))
    bad = {}
    for q in names:
        worst = int(np.argmax(errs[q]))
        print('%-14s error %.3e (case %d)  tolerance %.3e' % (q, errs[q][worst], worst, tol[q]))
        if not errs[q][worst] <= tol[q]:
            bad[q] = (float(errs[q][worst]), worst, float(tol[q]))
    assert not bad, bad


def test_linearize(cuda, gold):
    """Residuals, G, C, B, rv, rt of every link and the sum of squares per 64-link block."""
    from islam_amd import ops
    lin, part = ops.pvgo_linearize(*_chain(gold, cuda))
    _check(gold, dict(lin=lin.cpu().numpy(), loss_part=part.cpu().numpy()), ('res', 'G', 'C', 'B', 'loss_part'))


def test_linearize_edges(cuda, gold):
    """VO factors on arbitrary edges: i > j, j = i + 1, long range."""
    from islam_amd._lib import check, lib, ptr, stream_ptr
    E = len(gold['edges'])
    nodes, edges, poses = _t(gold['nodes'], cuda), _t(gold['edges'], cuda, torch.int64), _t(gold['edge_poses'], cuda)
    out = torch.empty((24, E), dtype=torch.float64, device=cuda)
    check(lib().islam_pvgo_linearize_edges(ptr(nodes), ptr(edges), ptr(poses), E, ptr(out), stream_ptr(cuda)))
    _check(gold, dict(edge_lin=out.cpu().numpy()), ('edge_e', 'edge_G', 'edge_C'))


def test_retract_both_signs(cuda, gold):
    from islam_amd import ops
    nodes, vels, dx = _t(gold['nodes'], cuda), _t(gold['vels'], cuda), _t(gold['dx'], cuda)
    n = gen.N_PARTIAL
    pos = ops.pvgo_retract(nodes, vels, dx, 1.0)
    neg = ops.pvgo_retract(nodes[:n].contiguous(), vels[:n].contiguous(), dx[:n].contiguous(), -1.0)
    _check(gold, dict(retract_pos=[a.cpu().numpy() for a in pos], retract_neg=[a.cpu().numpy() for a in neg]),
           ('retract_nodes', 'retract_vels'))


def test_align_to_a_general_target(cuda, gold):
    from islam_amd import ops
    n = gen.N_PARTIAL
    an, av = ops.pvgo_align(_t(gold['nodes'][:n], cuda), _t(gold['vels'][:n], cuda), _t(gold['align_target'], cuda))
    _check(gold, dict(align=(an.cpu().numpy(), av.cpu().numpy())), ('align_nodes', 'align_vels'))


def test_vo_loss_and_gradient(cuda, gold):
    """Forward values, and the gradient with respect to P <- Exp(delta) P under non-uniform upstream weights."""
    from islam_amd import ops
    nodes, edges = _t(gold['nodes'], cuda), _t(gold['edges'], cuda, torch.int64)
    poses = _t(gold['edge_poses'], cuda).requires_grad_(True)
    tl, rl = ops.pvgo_vo_loss(nodes, edges, poses)
    (tl * _t(gold['g_trans'], cuda) + rl * _t(gold['g_rot'], cuda)).sum().backward()
    g = poses.grad.cpu().numpy()
    assert g.shape == (len(gold['edges']), 7) and np.all(g[:, 6] == 0.0)
    _check(gold, dict(vo_loss=(tl.detach().cpu().numpy(), rl.detach().cpu().numpy()), vo_grad=g), ('vo_loss', 'vo_grad'))


def test_trial(cuda, gold):
    """islam_pvgo_trial as dist_pvgo.py calls it, on the reference linearisation: the retracted state, and per 64-link block the sum
    of squared residuals there and sum JD.(2R + JD) of the step."""
    from islam_amd._lib import check, lib, ptr, stream_ptr
    nodes, vels, poses, drots, dtrans, dvels, dts = _chain(gold, cuda)
    dx, lin = _t(gold['dx'], cuda), _t(gold['lin_ref'], cuda)
    M = len(gold['poses'])
    nblk = (M + 63) // 64
    nt, vt = torch.zeros_like(nodes), torch.zeros_like(vels)
    part = torch.zeros(2 * nblk + 2, dtype=torch.float64, device=cuda)
    check(lib().islam_pvgo_trial(ptr(nodes), ptr(vels), ptr(dx), ptr(poses), ptr(drots), ptr(dtrans), ptr(dvels), ptr(dts), ptr(lin), M,
                                 ptr(nt), ptr(vt), ptr(part), stream_ptr(cuda)))
    _check(gold, dict(trial=(nt.cpu().numpy(), vt.cpu().numpy(), part[:2 * nblk].view(nblk, 2).cpu().numpy())),
           ('trial_nodes', 'trial_vels', 'trial_sq', 'trial_qd'))


@pytest.mark.parametrize('F', [13, 129])
def test_lm_on_a_tumbling_trajectory_matches_oracle(cuda, F):
    """The whole LM loop on 3-D geometry (body rates up to 2 rad/s about all axes): 13 nodes run in the one-launch small-graph loop,
    129 in the fused loop -- linbuild, trial_lin, trial_elim and small_lm share link_residuals and link_jacobians with the kernels
    checked above.  Same assertions and tolerances as test_pvgo_gpu.test_lm_matches_oracle."""
    from islam_amd import ops
    from oracle import lie, pvgo as opvgo
    from tests.helpers import se3_log_err, tumbling_problem
    prob, _ = tumbling_problem(F)
    opt = opvgo.run_pvgo(**prob, loss_weight=LW, mode='dense' if F <= 33 else 'banded', return_optimizer=True)[5]
    nodes, vels, poses, drots, dtrans, dvels, dts = (_t(prob[k], cuda) for k in ('init_nodes', 'init_vels', 'vo_motions', 'imu_drots',
                                                                                'imu_dtrans', 'imu_dvels', 'dts'))
    res, trace = ops.pvgo_run_chain(nodes, vels, poses, drots, dtrans, dvels, dts, ops.pvgo_default_params(LW, radius=1e4), trace_cap=256)
    ot = np.array([(l, d, float(a)) for l, d, a in opt.trace])
    assert res.trials == len(ot)
    np.testing.assert_array_equal(trace[:, 2], ot[:, 2])
    np.testing.assert_allclose(trace[:, 0], ot[:, 0], rtol=1e-8)
    np.testing.assert_allclose(trace[:, 1], ot[:, 1], rtol=1e-12)
    err = se3_log_err(nodes.cpu().numpy(), opt.nodes)
    ref = np.maximum(np.linalg.norm(lie.se3_log(opt.nodes), axis=-1), 1e-6)
    assert (err / ref).max() < 1e-6
    np.testing.assert_allclose(vels.cpu().numpy(), opt.vels, rtol=1e-6, atol=1e-8)
