"""Dense reprojection normal equations and pose refinement on the MI355X (csrc/dense_reproj.hip) against the
float64 restatement of tests/dense_reproj_f64.py.

Shapes are chosen against the kernel's constants (256 threads, ISLAM_DENSE_REPROJ_NBLK = 64 workgroups per link): 7 x 9 is below one
wavefront, 24 x 40 = 960 leaves most workgroups idle and is no multiple of 256, 136 x 168 = 22848 is above 64 * 256 = 16384 with a
ragged tail, so some threads loop twice.

Tolerances.  All per-pixel arithmetic is float64 on both sides, so a sum differs from the restatement's only through rounding: each
of its n terms carries at most 64 roundings and any summation order adds at most n more, |dev - ref| <= 2^-52 (64 + n) sum|term|.
At n = 15000 that is 3.3e-12 of sum|term|; one missing pixel changes a sum by about 1e-4 of it."""
import functools

import numpy as np
import pytest
import torch

from islam_amd import ops, robust
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseReprojectionLoss
from islam_amd.information import PvgoInfo
from tests.dense_reproj_f64 import (FEW, KERNELS, MOUNT, OK, S_COST, S_COUNT, S_L1, SEEDS, SHAPES, XI0, U, _dev, _dev_args, make_scene,
                                    refine_reference_link, reproj_reference, right_perturb, scene_args)
from tests.dense_reproj_f64 import pose_dist as _dist

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """The scene of a shape, evaluated 0.02 away from the planted motion, and its restatement under each kernel (computed once)."""
    sc = make_scene(B, H, W, seed=SEEDS[H], noise=0.3)
    sc['start'] = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    refs = {k: reproj_reference(*scene_args(sc, sc['start']), kernel=kern) for k, kern in KERNELS.items()}
    return sc, refs


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_scene_conditions(B, H, W):
    """On the restatement alone: every clause drops a pixel, at least half the pixels stay, and no pixel lies within 1e-9 of a
    clause's threshold (so the count must match exactly)."""
    sc, refs = _case(B, H, W)
    for r in refs['none']:
        print('%dx%d: kept %d of %d, dropped by clause %s, closest margin %.2e' % (H, W, r['count'], H * W, r['rejects'], np.nanmin(r['margin'])))
        assert (r['rejects'] > 0).all()
        assert 2 * r['count'] >= H * W
        assert np.nanmin(r['margin']) > 1e-9


@pytest.mark.parametrize('kind', list(KERNELS))
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_sums_match_restatement(cuda, B, H, W, kind):
    sc, refs = _case(B, H, W)
    out = ops.dense_reproj_normal(*_dev_args(sc, sc['start']), rgb2imu=_dev(MOUNT), kernel=KERNELS[kind])
    got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
    for b, r in enumerate(refs[kind]):
        n = r['count']
        bound = U * (64 + n)
        assert got['count'][b] == n == got['sums'][b, S_COUNT]
        err = np.abs(got['sums'][b] - r['sums'])
        print('link %d n %d: worst error / bound: camera-frame sums %.3f, H %.3f, g %.3f' % (
            b, n, (err / np.maximum(bound * r['abs'], 1e-300)).max(), (np.abs(got['H'][b] - r['H']) / (bound * r['Habs'])).max(),
            (np.abs(got['g'][b] - r['g']) / (bound * r['gabs'])).max()))
        assert (err <= bound * r['abs']).all()
        assert (np.abs(got['H'][b] - r['H']) <= bound * r['Habs']).all()
        assert (np.abs(got['g'][b] - r['g']) <= bound * r['gabs']).all()
        assert abs(got['cost'][b] - r['cost']) <= bound * r['abs'][S_COST] and got['cost'][b] == got['sums'][b, S_COST]
        assert abs(got['l1'][b] - r['l1']) <= bound * r['abs'][S_L1] and got['l1'][b] == got['sums'][b, S_L1]
        assert np.array_equal(got['H'][b], got['H'][b].T)
        if kind == 'none':        # the reference's value: DenseReprojectionLoss.__call__ in float64 on the same tensors
            fx, fy, cx, cy = sc['intr'][b]
            loss = DenseReprojectionLoss(_dev(sc['depth'][b:b + 1], torch.float64), _dev(sc['flow'][b:b + 1], torch.float64), fx, fy, cx, cy,
                                         _dev(sc['mask'][b:b + 1]), pp.SE3(_dev(MOUNT)), device='cuda')
            want = float(loss(pp.SE3(_dev(sc['start'][b:b + 1])))[0])
            assert abs(got['l1'][b] / n - want) <= bound * r['abs'][S_L1] / n
    # one missing pixel would show: the smallest single term of the count column is 1, far above the bound
    assert U * (64 + refs[kind][0]['count']) * refs[kind][0]['abs'][S_COUNT] < 1e-6


def test_identity_mount_and_missing_mask(cuda):
    """rgb2imu=None is the identity mount and mask=None is all ones."""
    sc, _ = _case(1, 24, 40)
    ref = reproj_reference(sc['depth'], sc['flow'], None, sc['start'], None, sc['intr'])[0]
    d = _dev_args(sc, sc['start'])
    out = ops.dense_reproj_normal(d[0], d[1], None, d[3], d[4])
    n = ref['count']
    assert out.count.item() == n > 480
    assert (np.abs(out.H[0].cpu().numpy() - ref['H']) <= U * (64 + n) * ref['Habs']).all()
    assert (np.abs(out.g[0].cpu().numpy() - ref['g']) <= U * (64 + n) * ref['gabs']).all()
    ident = ops.dense_reproj_normal(d[0], d[1], None, d[3], d[4], rgb2imu=_dev(np.array([0, 0, 0, 0, 0, 0, 1.0])))
    assert torch.equal(ident.sums, out.sums)


def test_two_calls_give_the_same_bits(cuda):
    sc, _ = _case(3, 136, 168)
    a = ops.dense_reproj_normal(*_dev_args(sc, sc['start']), rgb2imu=_dev(MOUNT), kernel=robust.Huber(1.0))
    b = ops.dense_reproj_normal(*_dev_args(sc, sc['start']), rgb2imu=_dev(MOUNT), kernel=robust.Huber(1.0))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ra = ops.dense_reproj_refine(*_dev_args(sc, sc['start']), rgb2imu=_dev(MOUNT), iters=4, trace_cap=4)
    rb = ops.dense_reproj_refine(*_dev_args(sc, sc['start']), rgb2imu=_dev(MOUNT), iters=4, trace_cap=4)
    for x, y in zip(ra, rb):
        assert torch.equal(x, y)


def test_empty_mask_gives_zeros_and_nan_mean(cuda):
    sc, _ = _case(1, 24, 40)
    d = _dev_args(sc)
    out = ops.dense_reproj_normal(d[0], d[1], torch.zeros_like(d[2]), d[3], d[4], rgb2imu=_dev(MOUNT))
    assert not out.H.any() and not out.g.any() and out.count.item() == 0 and out.cost.item() == 0
    assert torch.isnan(out.l1 / out.count).all()


def test_cost_is_the_quadratic_form_of_the_device_H(cuda):
    """Zero-residual flow (rounded to float32, as the kernel reads it): the kernel's cost at motion Exp(xi), |xi| = 2e-3, against
    xi^T H xi with the kernel's H at motion.  Held to 10 x the restatement's own defect for the same xi, which is third order in xi
    (plus the 2.6e-13 that the rounding of the flow leaves at motion): 3.6e-4 .. 6.8e-3 of the quadratic form for these five xi.  A
    wrong frame, sign or row order gives O(1); the restatement's defect is asserted below 5 %."""
    sc = make_scene(1, 24, 40, seed=5)
    base = ops.dense_reproj_normal(*_dev_args(sc), rgb2imu=_dev(MOUNT))
    ref0 = reproj_reference(*scene_args(sc))[0]
    Hd = base.H[0].cpu().numpy()
    rng = np.random.default_rng(0)
    for _ in range(5):
        xi = rng.standard_normal(6)
        xi *= 2e-3 / np.linalg.norm(xi)
        moved = right_perturb(sc['motion'], xi)
        ref = reproj_reference(*scene_args(sc, moved))[0]
        quad_ref = xi @ ref0['H'] @ xi
        defect = abs(ref['cost'] - quad_ref)
        got = ops.dense_reproj_normal(*_dev_args(sc, moved), rgb2imu=_dev(MOUNT)).cost.item()
        quad = xi @ Hd @ xi
        print('quadratic form %.6e, device cost %.6e (off by %.2e), restatement defect %.2e = %.2e of it' % (
            quad, got, abs(got - quad), defect, defect / quad_ref))
        assert 0 < defect <= 0.05 * quad_ref
        assert abs(got - quad) <= 10 * defect


@functools.lru_cache(maxsize=None)
def _planted(H, W, outliers):
    sc = make_scene(1, H, W, seed=23, noise=0.3, outliers=0.1 if outliers else 0.0)
    sc['start'] = right_perturb(sc['motion'], XI0)
    run = lambda kern, order: refine_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['start'][0], MOUNT, sc['intr'][0],
                                                    kernel=kern, iters=10, order=order)
    kern = robust.Huber(1.0) if outliers else None
    return sc, kern, {o: run(kern, o) for o in ('sums', 'fwd', 'bwd')}, (run(None, 'sums') if outliers else None)


@pytest.mark.parametrize('outliers', [False, True], ids=['noise', 'outliers_huber'])
@pytest.mark.parametrize('H,W', [(24, 40), (72, 96)])
def test_refinement_matches_restatement(cuda, H, W, outliers):
    """Ten evaluations from 0.08 away from the planted motion: 0.3 px of flow noise and no kernel, or also 10 % of the pixels moved
    by up to +-20 px under Huber(1.0).  The device pose is held to the restatement's by 10 x max(the restatement's last step, the
    distance between the restatement run with forward and with backward summation).  In the first GPU run (last step, forward /
    backward distance, device to restatement):
      24x40 noise: 3.7e-11, 1.7e-16, 9.8e-17      72x96 noise: 1.9e-11, 2.0e-14, 1.9e-11
      24x40 Huber: 1.1e-10, 5.0e-09, 5.6e-15      72x96 Huber: 2.4e-10, 2.4e-10, 7.1e-17
    (a distance of the size of the last step means that one run took the last trial and the other did not).  Accept / reject traces
    are not compared: at the convergence floor they depend on the last bit."""
    sc, kern, ref, plain = _planted(H, W, outliers)
    r = ref['sums']
    end = _dist(sc['motion'][0], r['motion'])
    order_gap = _dist(ref['fwd']['motion'], ref['bwd']['motion'])
    print('%dx%d %s: restatement ends %.1f x closer (%.3e), last step %.3e, forward/backward gap %.3e' % (
        H, W, 'huber' if outliers else 'noise', 0.08 / end, end, r['last_step'], order_gap))
    assert r['status'] == OK and 5 * end <= 0.08 and r['last_step'] < 1e-6          # conditions on the restatement alone
    if outliers:
        assert 3 * end <= _dist(sc['motion'][0], plain['motion'])
    d = _dev_args(sc, sc['start'])
    out = ops.dense_reproj_refine(*d, rgb2imu=_dev(MOUNT), kernel=kern, iters=10, trace_cap=10)
    pose = out.motion[0].cpu().numpy()
    gap = _dist(r['motion'], pose)
    print('   device: %.3e from the restatement, accepted %d rejected %d, damping %.1e' % (gap, out.accepted.item(), out.rejected.item(), out.damping.item()))
    assert out.status.item() == OK and out.accepted.item() + out.rejected.item() == 9
    assert gap <= 10 * max(r['last_step'], order_gap)
    assert abs(np.linalg.norm(pose[3:]) - 1) < 1e-15
    tr = out.trace[:, 0].cpu().numpy()
    assert abs(tr[0] - r['trace'][0]) <= 1e-11 * r['trace'][0] and np.isfinite(tr).all()
    at = ops.dense_reproj_normal(d[0], d[1], d[2], out.motion, d[4], rgb2imu=_dev(MOUNT), kernel=kern)
    for k in ('H', 'g', 'cost', 'l1', 'count', 'sums'):
        assert torch.equal(getattr(out, k), getattr(at, k)), k


def test_one_evaluation_is_the_normal_equations(cuda):
    sc, _ = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    out = ops.dense_reproj_refine(*d, rgb2imu=_dev(MOUNT), iters=1)
    at = ops.dense_reproj_normal(*d, rgb2imu=_dev(MOUNT))
    assert torch.equal(out.motion, d[3]) and torch.equal(out.H, at.H) and torch.equal(out.sums, at.sums)
    assert not out.accepted.any() and not out.rejected.any() and not out.status.any()


def test_status_marks_links_that_cannot_be_refined(cuda):
    """A link with an all-zero mask, and a link with fewer valid pixels than min_count, beside healthy links: the bad link's status
    is set and its pose comes back unchanged, the healthy links match a batch without it bit for bit."""
    sc, _ = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    keep = [0, 2]
    healthy = ops.dense_reproj_refine(*(x[keep] for x in d), rgb2imu=_dev(MOUNT), iters=6)
    assert not healthy.status.any() and healthy.accepted.min().item() >= 1
    for case in ('empty', 'few'):
        mask = d[2].clone()
        mask[1] = 0
        min_count = 16
        if case == 'few':
            mask[1, 10:12, 17:22] = 1          # ten pixels in the middle of the image
            min_count = 40
        out = ops.dense_reproj_refine(d[0], d[1], mask, d[3], d[4], rgb2imu=_dev(MOUNT), iters=6, min_count=min_count)
        torch.cuda.synchronize()
        assert out.status.tolist() == [OK, FEW, OK]
        assert torch.equal(out.motion[1], d[3][1]) and out.accepted[1].item() == 0 and out.rejected[1].item() == 0
        assert out.count[1].item() == (0 if case == 'empty' else 10)
        for k in ('motion', 'H', 'g', 'cost', 'l1', 'count', 'sums', 'damping', 'accepted', 'rejected'):
            assert torch.equal(getattr(out, k)[keep], getattr(healthy, k)), (case, k)


def test_information_into_run_pvgo(cuda):
    """DenseReprojectionLoss.information on the 8 links of a 9-node chain -> PvgoInfo.from_dense_reproj -> run_pvgo(info=...)."""
    from islam_amd.pvgo import run_pvgo
    from tests.helpers import chain_problem
    prob, _ = chain_problem(9)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)
    sc = make_scene(8, 24, 40, seed=31, noise=0.3, motion=prob['vo_motions'], vary=False)
    fx, fy, cx, cy = sc['intr'][0]
    loss = DenseReprojectionLoss(_dev(sc['depth']), _dev(sc['flow']), fx, fy, cx, cy, _dev(sc['mask']), pp.SE3(_dev(MOUNT)), device='cuda')
    motion = pp.SE3(_dev(sc['motion']))
    ne = loss.normal_equations(motion)
    assert ne.count.min().item() > 300
    Hm = loss.information(motion, sigma_px=0.5)
    assert torch.equal(Hm, ne.H / 0.25)
    info = PvgoInfo.from_dense_reproj(Hm)
    assert np.array_equal(info.vo, Hm.cpu().numpy())
    assert np.array_equal(PvgoInfo.from_dense_reproj(ne.H, sigma_px=0.5).vo, info.vo)
    res_var = loss.information(motion, sigma_px='residual')
    want = ne.H / (ne.cost / (2 * ne.count - 6)).view(-1, 1, 1)
    assert torch.allclose(res_var, want, rtol=1e-14, atol=0)

    def run(info, **kw):
        return run_pvgo(pp.SE3(t(prob['init_nodes'])), t(prob['init_vels']), pp.SE3(t(prob['vo_motions'])), torch.tensor(prob['links']),
                        t(prob['dts']), pp.SO3(t(prob['imu_drots'])), t(prob['imu_dtrans']), t(prob['imu_dvels']), device='cuda',
                        loss_weight=(1, 1, 1, 1), info=info, **kw)

    # the LM's loss (unweighted sum |r|^2 over all factors) at the initial state, from the kernel the loop itself starts with
    g = lambda a: _dev(np.asarray(a, np.float64))
    first = ops.pvgo_linearize(g(prob['init_nodes']), g(prob['init_vels']), g(prob['vo_motions']), g(prob['imu_drots']), g(prob['imu_dtrans']),
                               g(prob['imu_dvels']), g(prob['dts']).reshape(-1))[1].sum().item()
    off = info.vo.copy()
    off[3] = 0.0                    # all-zero information on one edge: that factor is off, and run_pvgo accepts it
    for name, inf in (('all edges', info), ('edge 3 off', PvgoInfo.from_dense_reproj(off))):
        out = run(inf, return_info=True, marginals=True)
        nodes, vels, res, marg = out[2].tensor().numpy(), out[3].numpy(), out[5], out[6]
        print('run_pvgo under dense-reprojection information, %s: loss %.6e -> %.6e (%d steps, %d trials)' % (name, first, res.loss, res.steps, res.trials))
        assert np.isfinite(nodes).all() and np.isfinite(vels).all() and res.status == 0 and res.steps >= 1
        if inf is info:
            # (with an edge off the loss is not asserted: the accept-test loss is UNWEIGHTED, section 3.19, so it still counts the VO
            #  residual the weighted step no longer holds; every trial raises it, and after 16 rejections PyPose's reject limit takes the
            #  17th trial as it is: 1 step, 17 trials, 0.0469 -> 0.0610 here)
            assert res.loss <= first
        ev = np.linalg.eigvalsh(marg.pose_cov[1:].cpu().numpy())
        assert np.isfinite(ev).all() and (ev[:, 0] > 0).all()
