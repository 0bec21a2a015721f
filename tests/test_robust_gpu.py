"""run_pvgo(kernel=...) on the MI355X: the chain loop (islam_pvgo_run_chain_robust) and the two
general-topology solvers against the float64 restatement of the robust LM in tests/test_robust_cpu.py, outlier rejection, the
default path left alone, the argument errors and BilevelLoop's hand-over of the kernel."""
import numpy as np
import pytest
import torch

from oracle import lie
from tests.helpers import chain_problem
from tests.test_robust_cpu import LW, OUTLIER_CASE, OUTLIER_RATIO, corrupt, outlier_kernels, pose_error, run_robust

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _run(prob, lw=LW, **kw):
    from islam_amd import lietensor as pp
    from islam_amd.pvgo import run_pvgo
    return run_pvgo(pp.SE3(_t(prob['init_nodes'])), _t(prob['init_vels']), pp.SE3(_t(prob['vo_motions'])), torch.tensor(prob['links']),
                    _t(prob['dts']), pp.SO3(_t(prob['imu_drots'])), _t(prob['imu_dtrans']), _t(prob['imu_dvels']), device='cuda',
                    loss_weight=lw, **kw)


def _chain_trace(prob, spec, lw=LW):
    """The per-trial (loss, damping, accepted) of islam_pvgo_run_chain_robust."""
    from islam_amd import ops
    d = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    nodes, vels = d(prob['init_nodes']), d(prob['init_vels'])
    res, trace = ops.pvgo_run_chain(nodes, vels, d(prob['vo_motions']), d(prob['imu_drots']), d(prob['imu_dtrans']),
                                    d(prob['imu_dvels']), d(prob['dts']), ops.pvgo_default_params(lw), trace_cap=256, robust=spec)
    return res, trace


def _check_against(out, info_steps, info_trials, trace, nodes_ref, vels_ref, opt):
    assert info_trials == len(opt.trace) and info_steps == len(opt.step_losses)
    assert [bool(t[2]) for t in trace] == [t[2] for t in opt.trace]
    np.testing.assert_allclose([t[0] for t in trace], [t[0] for t in opt.trace], rtol=1e-10)
    np.testing.assert_allclose([t[1] for t in trace], [t[1] for t in opt.trace], rtol=1e-10)
    assert pose_error(out[2].tensor().numpy(), nodes_ref).max() < 1e-8
    np.testing.assert_allclose(out[3].numpy(), vels_ref, atol=1e-8)


@pytest.mark.parametrize('N', [9, 64, 257, 5001])
@pytest.mark.parametrize('kind', ['huber', 'cauchy'])
def test_chain_matches_restatement(cuda, N, kind):
    from islam_amd.robust import Cauchy, Huber, parse_kernel
    kernel = {'huber': Huber(0.1), 'cauchy': Cauchy(0.1)}[kind]
    prob, _ = chain_problem(N)
    bad = corrupt(prob)
    spec = parse_kernel(kernel)
    nodes_ref, vels_ref, opt = run_robust(bad, spec, mode='dense' if N <= 64 else 'banded')
    out = _run(bad, kernel=kernel, return_info=True)
    res = out[5]
    res2, trace = _chain_trace(bad, spec)
    assert (res2.steps, res2.trials) == (res.steps, res.trials)
    assert res.loss == pytest.approx(opt.loss, rel=1e-10)
    _check_against(out, res.steps, res.trials, trace, nodes_ref, vels_ref, opt)


def _closure_problem(F, closures, seed=5):
    """chain_problem(F) with chain edges replaced by long-range ones measured with a little noise (tests/test_surface_gpu.py)."""
    prob, tr = chain_problem(F)
    links = prob['links'].copy()
    vo = prob['vo_motions'].copy()
    gt = np.concatenate([tr['gt_pos'], tr['gt_quat']], 1)
    rng = np.random.default_rng(seed)
    for e, (i, j) in closures.items():
        links[e] = (i, j)
        rel = lie.se3_mul(lie.se3_inv(gt[i]), gt[j])
        vo[e] = lie.se3_mul(rel, lie.se3_exp(rng.normal(0, 0.01, 6)))
    return dict(prob, links=links, vo_motions=vo)


@pytest.mark.parametrize('kind', ['huber', 'cauchy'])
def test_loop_closure_solvers_match_restatement_and_each_other(cuda, kind):
    from islam_amd.robust import Cauchy, Huber, parse_kernel
    kernel = {'huber': Huber(0.1), 'cauchy': [Cauchy(0.1), Cauchy(0.05), None, Huber(0.2)]}[kind]
    p2 = _closure_problem(33, {3: (0, 9), 11: (4, 17), 19: (30, 2), 25: (25, 26), 28: (31, 8)})
    bad = corrupt(p2, edges=(11, 16, 28))                  # one false loop closure, two bad frame-to-frame motions
    nodes_ref, vels_ref, opt = run_robust(bad, parse_kernel(kernel), mode='dense')
    out = {}
    for how in ('dense', 'band_pcg'):
        out[how] = _run(bad, kernel=kernel, general_solver=how, return_info=True)
        info = out[how][5]
        _check_against(out[how], info['steps'], info['trials'], info['trace'], nodes_ref, vels_ref, opt)
    d, p = out['dense'], out['band_pcg']
    assert p[5]['off_band_edges'] == 4 and p[5]['trials'] == d[5]['trials']
    np.testing.assert_allclose([x[0] for x in p[5]['trace']], [x[0] for x in d[5]['trace']], rtol=1e-9)
    np.testing.assert_allclose(p[2].tensor().numpy(), d[2].tensor().numpy(), atol=1e-9)
    np.testing.assert_allclose(p[3].numpy(), d[3].numpy(), atol=1e-9)


def test_kernel_rejects_corrupted_vo_motions(cuda):
    """Calibrated on the restatement (tests/test_robust_cpu.py): the robust solution's largest pose error is at most a quarter of the
    least-squares one, measured against the clean problem's solution."""
    from islam_amd.robust import parse_kernel
    lw = OUTLIER_CASE['lw']
    prob, _ = chain_problem(OUTLIER_CASE['N'])
    target = _run(prob, lw)[2].tensor().numpy()
    bad = corrupt(prob)
    worst_ls = pose_error(_run(bad, lw)[2].tensor().numpy(), target).max()
    assert worst_ls > 1.0
    for k in outlier_kernels():
        got = _run(bad, lw, kernel=k)[2].tensor().numpy()
        assert pose_error(got, target).max() <= OUTLIER_RATIO * worst_ls
        ref, _, _ = run_robust(bad, parse_kernel(k), loss_weight=lw, mode='banded')
        assert pose_error(got, ref).max() < 1e-8


def test_default_path_unchanged(cuda):
    """kernel=None is the code path of today, bit for bit; an inactive Huber (c = 1 everywhere) lands on the same solution."""
    from islam_amd.robust import Huber
    prob, _ = chain_problem(257)
    bad = corrupt(prob)
    a = _run(bad, return_info=True)
    b = _run(bad, return_info=True, kernel=None)
    for x, y in zip(a[:4], b[:4]):
        x = x.tensor() if hasattr(x, 'tensor') else x
        y = y.tensor() if hasattr(y, 'tensor') else y
        assert torch.equal(x.cpu(), y.cpu())
    assert (a[5].steps, a[5].trials, a[5].loss, a[5].damping) == (b[5].steps, b[5].trials, b[5].loss, b[5].damping)
    c = _run(bad, return_info=True, kernel=Huber(1e6))
    assert (c[5].steps, c[5].trials) == (a[5].steps, a[5].trials)
    assert c[5].loss == pytest.approx(a[5].loss, rel=1e-12)
    assert pose_error(c[2].tensor().numpy(), a[2].tensor().numpy()).max() < 1e-12
    np.testing.assert_allclose(c[3].numpy(), a[3].numpy(), atol=1e-12)
    np.testing.assert_allclose(c[0].cpu().numpy(), a[0].cpu().numpy(), rtol=1e-12, atol=1e-15)


def test_errors(cuda):
    from islam_amd.robust import Cauchy, Huber
    prob, tr = chain_problem(9)
    with pytest.raises(NotImplementedError):
        _run(prob, kernel=Huber(), marginals=True)
    with pytest.raises(ValueError):
        _run(prob, kernel=[Huber(), None, Cauchy()])
    with pytest.raises(ValueError):
        _run(prob, kernel=Huber(0.0))
    with pytest.raises(ValueError):
        Cauchy(-1.0)
    with pytest.raises(ValueError):
        _run(prob, kernel='huber')
    # with a reprojection factor: refused before anything is built from it
    with pytest.raises(NotImplementedError):
        _run(prob, lw=tuple(LW) + (1.0,), kernel=Huber(), reproj=object())
    # the C entry point validates the spec itself
    from islam_amd import ops
    from islam_amd._lib import IslamHipError
    from islam_amd.robust import parse_kernel
    spec = parse_kernel(Huber(0.1))
    spec.kernels[0].delta = -1.0
    d = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    with pytest.raises(IslamHipError):
        ops.pvgo_run_chain(d(prob['init_nodes']), d(prob['init_vels']), d(prob['vo_motions']), d(prob['imu_drots']),
                           d(prob['imu_dtrans']), d(prob['imu_dvels']), d(prob['dts']), ops.pvgo_default_params(LW), robust=spec)


def test_bilevel_loop_hands_the_kernel_to_run_pvgo(cuda, monkeypatch):
    """One BilevelLoop step of the smallest configuration tests/test_configs_gpu.py drives: run_pvgo receives ``kernel``."""
    from islam_amd import bilevel, synthetic
    from islam_amd import lietensor as pp
    from islam_amd.imu_integrator import IMUModule
    from islam_amd.robust import Cauchy
    from tests.test_configs_gpu import B, CONFIGS, _StubVO
    cfg = CONFIGS['kitti04']
    tr = synthetic.car_trajectory(B + 1, seed=21, **cfg['traj'])
    T_IL = np.asarray(cfg['T_IL'], dtype=np.float64)
    cam = lie.se3_mul(lie.se3_inv(T_IL)[None], lie.se3_mul(tr['vo_motions'], T_IL[None]))
    imu = IMUModule(tr['accels'], tr['gyros'], tr['imu_dts'], np.zeros(3), np.zeros(3), tr['init'], tr['gravity'],
                    tr['rgb2imu_sync'], device='cuda', denoise_model_name=None, denoise_accel=True, denoise_gyro=False,
                    dtype=torch.float64)
    seen = []
    real = bilevel.run_pvgo

    def spy(*a, **kw):
        seen.append(kw.get('kernel', 'absent'))
        return real(*a, **kw)

    monkeypatch.setattr(bilevel, 'run_pvgo', spy)
    sample = {'link': torch.stack([torch.arange(B), torch.arange(1, B + 1)], 1), 'dt': torch.tensor(tr['dts'][:B])}
    k = Cauchy(0.5)
    loop = bilevel.BilevelLoop(_StubVO(cam, cuda), imu, pp.SE3(torch.tensor(T_IL)), tr['init'], loss_weight=cfg['lw'], batch_size=B,
                               device='cuda', pvgo_kernel=k)
    loss = loop.step(sample)
    assert seen == [k] and np.isfinite(loss)
    plain = bilevel.BilevelLoop(_StubVO(cam, cuda), imu, pp.SE3(torch.tensor(T_IL)), tr['init'], loss_weight=cfg['lw'], batch_size=B,
                                device='cuda')
    plain.step(sample)
    assert seen == [k, 'absent']
    with pytest.raises(ValueError):
        bilevel.BilevelLoop(_StubVO(cam, cuda), imu, pp.SE3(torch.tensor(T_IL)), tr['init'], pvgo_kernel='cauchy')
