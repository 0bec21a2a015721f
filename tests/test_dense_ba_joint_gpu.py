"""Joint (pose, inverse depth) dense bundle adjustment on the MI355X (csrc/dense_ba.hip) against the float64
restatement of tests/dense_reproj_f64.py.

Shapes, seeds and scene conditions are section 3.23's (tests/test_dense_reproj_gpu.py), asserted again on the joint restatement; the
depth map is that scene's with sigma_rho = 0.02 /m of inverse-depth noise, and three of its pixels carry no prior (0, NaN, -1).

Tolerances.  All per-pixel arithmetic is float64 on both sides.  A term of a sum is the difference of two parts, c J^T J and
h_pd h_pd^T / h_dd, which cancel, so the yardstick is the sum of the two parts' magnitudes: |dev - ref| <= 2^-52 (K + n) sum|parts| with
K = 128 roundings per term (counted in tests/dense_reproj_f64.py and section 3.25) and n for any order of summation."""
import functools

import numpy as np
import pytest
import torch

from islam_amd import _lib, ops, robust
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseReprojectionLoss
from islam_amd.information import PvgoInfo
from tests.dense_reproj_f64 import (BADPRIOR, FEW, K_ROUND, KERNELS, MOUNT, NOTPD, OK, PRIOR_W, S_COST, S_COUNT, S_L1, SEEDS, SHAPES, SIGMA_RHO, U,
                                    _dev, _dev_args, ba_reference, make_scene, noisy_prior, planted_case, pose_dist, right_perturb)

pytestmark = pytest.mark.gpu
WEIGHTS = np.array([PRIOR_W, 400.0, 100.0])          # per-link prior weights
NO_PRIOR = {(2, 5): 0.0, (3, 1): np.nan, (1, 7): -1.0}          # pixels whose depth gives no prior


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """The scene of a shape with a noisy depth prior, evaluated 0.02 away from the planted motion at the prior and at perturbed inverse
    depths, and its restatement under each kernel (computed once)."""
    sc = noisy_prior(make_scene(B, H, W, seed=SEEDS[H], noise=0.3), seed=H)
    for (r, c), val in NO_PRIOR.items():
        sc['depth'][:, r, c] = val
    sc['start'] = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    sc['w'] = WEIGHTS[:B].copy()
    rng = np.random.default_rng(H)
    with np.errstate(divide='ignore', invalid='ignore'):
        rho0 = 1.0 / sc['depth'].astype(np.float64)
    sc['rho'] = np.where(np.isfinite(rho0) & (rho0 > 0), rho0 * (1.0 + 0.03 * rng.standard_normal(rho0.shape)), 0.0)
    args = (sc['depth'], sc['flow'], sc['mask'], sc['start'], sc['rgb2imu'], sc['intr'], sc['w'])
    refs = {(k, st): ba_reference(*args, rho=None if st == 'prior' else sc['rho'], kernel=kern) for k, kern in KERNELS.items()
            for st in ('prior', 'moved')}
    return sc, refs


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_scene_conditions(B, H, W):
    """On the restatement alone, at both states: every clause drops a pixel, at least half the pixels stay, no pixel lies within 1e-9
    of a clause's threshold (so the count must match exactly), and the three pixels without a prior are outside the valid set."""
    sc, refs = _case(B, H, W)
    for st in ('prior', 'moved'):
        for r in refs[('none', st)]:
            print('%dx%d %s: kept %d of %d, dropped by clause %s, closest margin %.2e' % (H, W, st, r['count'], H * W, r['rejects'], np.nanmin(r['margin'])))
            assert (r['rejects'] > 0).all()
            assert 2 * r['count'] >= H * W
            assert np.nanmin(r['margin']) > 1e-9
            assert not any(r['valid'][p] or r['prior'][p] for p in NO_PRIOR) and (r['rho0'][~r['prior']] == 0).all()
    assert fx_below_half_width(sc, W) and (~sc['mask']).any()


def fx_below_half_width(sc, W):
    return (sc['intr'][:, 0] < W / 2).all()


@pytest.mark.parametrize('kind', list(KERNELS))
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_sums_match_restatement(cuda, B, H, W, kind):
    sc, refs = _case(B, H, W)
    d = _dev_args(sc, sc['start'])
    for st in ('prior', 'moved'):
        call = lambda: ops.dense_ba_normal(*d, _dev(sc['w']), inv_depth=None if st == 'prior' else _dev(sc['rho']), rgb2imu=_dev(MOUNT),
                                           kernel=KERNELS[kind])
        out, again = call(), call()
        for x, y in zip(out, again):
            assert torch.equal(x, y)
        got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
        for b, r in enumerate(refs[(kind, st)]):
            n = r['count']
            bound = U * (K_ROUND + n)
            assert got['count'][b] == n == got['sums'][b, S_COUNT]
            err = np.abs(got['sums'][b] - r['sums'])
            print('%s link %d n %d: worst error / bound: camera-frame sums %.3f, S %.3f, g %.3f' % (
                st, b, n, (err / np.maximum(bound * r['abs'], 1e-300)).max(), (np.abs(got['S'][b] - r['S']) / (bound * r['Sabs'])).max(),
                (np.abs(got['g'][b] - r['g']) / (bound * r['gabs'])).max()))
            assert (err <= bound * r['abs']).all()
            assert (np.abs(got['S'][b] - r['S']) <= bound * r['Sabs']).all()
            assert (np.abs(got['g'][b] - r['g']) <= bound * r['gabs']).all()
            assert abs(got['cost'][b] - r['cost']) <= bound * r['abs'][S_COST] and got['cost'][b] == got['sums'][b, S_COST]
            assert abs(got['l1'][b] - r['l1']) <= bound * r['abs'][S_L1] and got['l1'][b] == got['sums'][b, S_L1]
            assert np.array_equal(got['S'][b], got['S'][b].T)
    # one missing pixel would show: the smallest single term of the count column is 1, far above the bound
    assert U * (K_ROUND + refs[(kind, 'prior')][0]['count']) * refs[(kind, 'prior')][0]['abs'][S_COUNT] < 1e-6


def test_marginalised_information_lies_below_the_pose_only_one(cuda):
    """On the device's own matrices: H - S is positive semi-definite and S tends to H as the prior weight grows."""
    sc, refs = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    Hm = ops.dense_reproj_normal(*d, rgb2imu=_dev(MOUNT)).H.cpu().numpy()
    S = ops.dense_ba_normal(*d, _dev(sc['w']), rgb2imu=_dev(MOUNT)).S.cpu().numpy()
    big = ops.dense_ba_normal(*d, 1e300, rgb2imu=_dev(MOUNT)).S.cpu().numpy()
    for b, r in enumerate(refs[('none', 'prior')]):
        ev = np.linalg.eigvalsh(Hm[b] - S[b])
        bound = U * (K_ROUND + r['count']) * 2 * r['Sabs']
        print('link %d: eig(H - S) %.3e .. %.3e' % (b, ev[0], ev[-1]))
        assert ev[0] >= -6 * bound.max() and ev[-1] > 1e3 * 6 * bound.max()
        assert (np.abs(big[b] - Hm[b]) <= bound).all()


@pytest.mark.parametrize('H,W', [(24, 40), (72, 96)])
def test_refinement_matches_restatement(cuda, H, W):
    """Twenty evaluations on the planted scene (sigma_rho = 0.02 /m, 0.3 px, start 0.08 away).  The device pose and inverse depths are
    held to the restatement's by 10 x max(the restatement's last step, the gap between the restatement run with forward and with
    backward summation), for the pose distance and for max |delta rho| over the valid pixels; S, g, cost, l1, count and sums are the
    bits dense_ba_normal gives at the returned state; a second run gives the same bits."""
    sc, w, ref, _ = planted_case(H, W)
    r = ref['sums']
    gap_pose = pose_dist(ref['fwd']['motion'], ref['bwd']['motion'])
    gap_rho = float(np.abs(ref['fwd']['rho'] - ref['bwd']['rho']).max())
    assert r['status'] == OK and r['last_step'] < 1e-6          # conditions on the restatement alone
    d = _dev_args(sc, sc['start'])
    out = ops.dense_ba_refine(*d, w, iters=20, trace_cap=20)
    pose, rho = out.motion[0].cpu().numpy(), out.inv_depth[0].cpu().numpy()
    dp, dr = pose_dist(r['motion'], pose), float(np.abs(rho - r['rho'])[r['valid']].max())
    print('%dx%d: restatement last step %.3e, forward/backward gap %.3e (pose) %.3e (rho); device: pose %.3e, rho %.3e from the restatement, '
          'accepted %d rejected %d, damping %.1e' % (H, W, r['last_step'], gap_pose, gap_rho, dp, dr, out.accepted.item(), out.rejected.item(),
                                                     out.damping.item()))
    assert out.status.item() == OK and out.accepted.item() + out.rejected.item() == 19
    assert dp <= 10 * max(r['last_step'], gap_pose)
    assert dr <= 10 * max(r['last_step'], gap_rho)
    assert abs(np.linalg.norm(pose[3:]) - 1) < 1e-15 and (rho > 0).all()
    tr = out.trace[:, 0].cpu().numpy()
    assert abs(tr[0] - r['trace'][0]) <= 1e-11 * r['trace'][0] and np.isfinite(tr).all()
    at = ops.dense_ba_normal(d[0], d[1], d[2], out.motion, d[4], w, inv_depth=out.inv_depth)
    for k in ('S', 'g', 'cost', 'l1', 'count', 'sums'):
        assert torch.equal(getattr(out, k), getattr(at, k)), k
    again = ops.dense_ba_refine(*d, w, iters=20, trace_cap=20)
    for x, y in zip(out, again):
        assert torch.equal(x, y)
    # the device's joint pose beats the device's pose-only pose, like the restatement's
    alone = ops.dense_reproj_refine(*d, iters=20)
    assert pose_dist(sc['motion'][0], pose) < pose_dist(sc['motion'][0], alone.motion[0].cpu().numpy())


def test_refine_joint_with_a_mount_and_pixels_without_a_prior(cuda):
    """The mount, a user mask, all clauses active and three pixels without a prior, through DenseReprojectionLoss: the returned
    state is the one dense_ba_normal reproduces bit for bit, the pixels without a prior come back with rho = 0 and ``depth`` equal to
    the stored bits, every other pixel's depth is 1 / rho, and one evaluation is the normal equations at the prior."""
    sc, refs = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    fx, fy, cx, cy = sc['intr'][0]
    loss = DenseReprojectionLoss(d[0][:1], d[1][:1], fx, fy, cx, cy, d[2][:1], pp.SE3(_dev(MOUNT)), device='cuda')       # link 0
    sig = _dev(0.3 / np.sqrt(sc['w'][:1]))
    out = loss.refine_joint(pp.SE3(d[3][:1]), sig, sigma_px=0.3, iters=8, kernel=robust.Huber(1.0))
    assert out.status.tolist() == [OK] and out.accepted.item() >= 1
    at = ops.dense_ba_normal(d[0][:1], d[1][:1], d[2][:1], out.motion, d[4][:1], (0.3 / sig) ** 2, inv_depth=out.inv_depth, rgb2imu=_dev(MOUNT),
                             kernel=robust.Huber(1.0))
    for k in ('S', 'g', 'cost', 'l1', 'count', 'sums'):
        assert torch.equal(getattr(out, k), getattr(at, k)), k
    rho, depth = out.inv_depth[0].cpu().numpy(), out.depth[0].cpu().numpy()
    assert out.depth.dtype == torch.float32
    for p in NO_PRIOR:
        assert rho[p] == 0
        assert depth[p].view(np.int32) == sc['depth'][0][p].view(np.int32)
    have = rho > 0
    assert have.sum() == rho.size - len(NO_PRIOR) and np.array_equal(depth[have], (1.0 / rho[have]).astype(np.float32))
    assert (np.abs(rho[have] * sc['depth'][0][have].astype(np.float64) - 1) > 1e-6).mean() > 0.4          # the depths moved
    one = ops.dense_ba_refine(*d, _dev(sc['w']), rgb2imu=_dev(MOUNT), iters=1)
    first = ops.dense_ba_normal(*d, _dev(sc['w']), rgb2imu=_dev(MOUNT))
    assert torch.equal(one.motion, d[3]) and torch.equal(one.S, first.S) and torch.equal(one.sums, first.sums)
    with np.errstate(divide='ignore', invalid='ignore'):
        rho0 = 1.0 / sc['depth'].astype(np.float64)
    assert np.array_equal(one.inv_depth.cpu().numpy(), np.where(np.isfinite(rho0) & (rho0 > 0), rho0, 0.0))


def test_status_marks_only_its_own_link(cuda):
    """FEW (an empty mask), NOTPD (an empty mask with min_count = 0: S = 0 is finite and has no positive pivot) and BADPRIOR (a prior
    weight of 0, -1 or NaN, a device value) on the middle link: its status is set and its pose comes back as given, its inverse depths
    as the prior; the healthy links match a batch without it bit for bit."""
    sc, _ = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    keep = [0, 2]
    w = _dev(sc['w'])
    healthy = ops.dense_ba_refine(*(x[keep] for x in d), w[keep], rgb2imu=_dev(MOUNT), iters=6)
    assert not healthy.status.any() and healthy.accepted.min().item() >= 1
    empty = d[2].clone()
    empty[1] = 0
    with np.errstate(divide='ignore', invalid='ignore'):
        rho0 = 1.0 / sc['depth'][1].astype(np.float64)
    rho0 = np.where(np.isfinite(rho0) & (rho0 > 0), rho0, 0.0)
    cases = [('few', empty, w, 16, FEW), ('notpd', empty, w, 0, NOTPD)]
    for bad in (0.0, -1.0, float('nan')):
        wb = w.clone()
        wb[1] = bad
        cases.append(('badprior %r' % bad, d[2], wb, 16, BADPRIOR))
    for name, mask, wt, min_count, want in cases:
        out = ops.dense_ba_refine(d[0], d[1], mask, d[3], d[4], wt, rgb2imu=_dev(MOUNT), iters=6, min_count=min_count)
        torch.cuda.synchronize()
        assert out.status.tolist() == [OK, want, OK], name
        assert torch.equal(out.motion[1], d[3][1]) and out.accepted[1].item() == 0 and out.rejected[1].item() == 0, name
        assert np.array_equal(out.inv_depth[1].cpu().numpy(), rho0), name
        if want == BADPRIOR:
            assert torch.isnan(out.S[1]).all() and torch.isnan(out.cost[1])
        else:
            assert out.count[1].item() == 0 and not out.S[1].any()
        for k in ('motion', 'inv_depth', 'S', 'g', 'cost', 'l1', 'count', 'sums', 'damping', 'accepted', 'rejected'):
            assert torch.equal(getattr(out, k)[keep], getattr(healthy, k)), (name, k)
    assert _lib.DENSE_REPROJ_BADPRIOR == BADPRIOR
    with pytest.raises(ValueError, match='prior_weight'):          # a host-side number is validated before the call
        ops.dense_ba_refine(*d, 0.0, rgb2imu=_dev(MOUNT))
    with pytest.raises(ValueError, match='prior_weight'):
        ops.dense_ba_normal(*d, torch.tensor([1.0, -1.0, 1.0]), rgb2imu=_dev(MOUNT))


def test_marginalised_information_into_run_pvgo(cuda):
    """information(sigma_inv_depth=...) on the 8 links of a 9-node chain -> PvgoInfo.from_dense_reproj -> run_pvgo(info=...,
    marginals=True): the covariances are positive definite and their translation blocks are, in trace, no smaller than with the depth
    taken as exact (sigma_inv_depth=None)."""
    from islam_amd.pvgo import run_pvgo
    from tests.helpers import chain_problem
    prob, _ = chain_problem(9)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)
    sc = make_scene(8, 24, 40, seed=31, noise=0.3, motion=prob['vo_motions'], vary=False)
    fx, fy, cx, cy = sc['intr'][0]
    loss = DenseReprojectionLoss(_dev(sc['depth']), _dev(sc['flow']), fx, fy, cx, cy, _dev(sc['mask']), pp.SE3(_dev(MOUNT)), device='cuda')
    motion = pp.SE3(_dev(sc['motion']))
    exact = loss.information(motion, sigma_px=0.5)
    marg = loss.information(motion, sigma_px=0.5, sigma_inv_depth=SIGMA_RHO)
    ne = ops.dense_ba_normal(_dev(sc['depth']), _dev(sc['flow']), _dev(sc['mask']), _dev(sc['motion']), _dev(sc['intr']), (0.5 / SIGMA_RHO) ** 2,
                             rgb2imu=_dev(MOUNT))
    assert torch.equal(marg, ne.S / 0.25) and torch.equal(exact, loss.normal_equations(motion).H / 0.25)
    res_var = loss.information(motion, sigma_px='residual', sigma_inv_depth=SIGMA_RHO)
    n1 = ops.dense_ba_normal(_dev(sc['depth']), _dev(sc['flow']), _dev(sc['mask']), _dev(sc['motion']), _dev(sc['intr']), (1.0 / SIGMA_RHO) ** 2,
                             rgb2imu=_dev(MOUNT))
    assert torch.allclose(res_var, n1.S / (n1.cost / (2 * n1.count - 6)).view(-1, 1, 1), rtol=1e-14, atol=0)
    assert (np.linalg.eigvalsh((exact - marg).cpu().numpy())[:, 0] > 0).all()

    def run(info):
        out = run_pvgo(pp.SE3(t(prob['init_nodes'])), t(prob['init_vels']), pp.SE3(t(prob['vo_motions'])), torch.tensor(prob['links']),
                       t(prob['dts']), pp.SO3(t(prob['imu_drots'])), t(prob['imu_dtrans']), t(prob['imu_dvels']), device='cuda',
                       loss_weight=(1, 1, 1, 1), info=info, return_info=True, marginals=True)
        assert np.isfinite(out[2].tensor().numpy()).all() and out[5].status == 0
        return out[6].pose_cov[1:].cpu().numpy()

    cov_exact, cov_marg = run(PvgoInfo.from_dense_reproj(exact)), run(PvgoInfo.from_dense_reproj(marg))
    for cov in (cov_exact, cov_marg):
        ev = np.linalg.eigvalsh(cov)
        assert np.isfinite(ev).all() and (ev[:, 0] > 0).all()
    tr_exact, tr_marg = np.trace(cov_exact[:, :3, :3], axis1=1, axis2=2), np.trace(cov_marg[:, :3, :3], axis1=1, axis2=2)
    print('translation covariance trace, marginalised / exact depth: %s' % (tr_marg / tr_exact))
    assert (tr_marg >= tr_exact).all()
