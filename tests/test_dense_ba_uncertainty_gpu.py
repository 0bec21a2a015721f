"""Per-pixel prior weights and the posterior variance of the inverse depths on the MI355X (csrc/dense_ba.hip: ba_wmap_partial_kernel,
depth_var_factor_kernel, depth_var_pixel_kernel) against the float64 restatement of tests/dense_ba_var_f64.py.

Shapes, seeds and scene conditions are section 3.25's (tests/test_dense_ba_joint_gpu.py): the mount, per-link intrinsics and weights,
every 17th depth at 0.05, the user mask, three pixels without a prior, and in addition three pixels whose map entry is 0, NaN and -1;
the map itself is 2^U(-2,2), float32.  The conditions are asserted again on the map restatement.

Tolerances.  The sums: |dev - ref| <= 2^-52 (K + n) sum|parts| with K = K_MAP = K_ROUND + 1, the one rounding of w_i = w_b m_i on top of
section 3.25's count.  The variance: |dev - ref| <= 2^-52 (K_v + 64 cond(S_cam)) v with K_v = K_VAR = 128 roundings on the longest path
of the pixel pass (counted in tests/dense_ba_var_f64.py) and 64 cond for the two solutions of S_cam x = h, both sides given the same
sums bits."""
import functools

import numpy as np
import pytest
import torch

from islam_amd import ops, robust
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseReprojectionLoss
from tests.dense_ba_var_f64 import (K_MAP, K_VAR, SIGMA_PX, ba_map_reference, chi2_band, rho_rms, scam_from_sums, two_level_case,
                                    variance_reference)
from tests.dense_reproj_f64 import (BADPRIOR, FEW, KERNELS, MOUNT, NOTPD, OK, S_COST, S_COUNT, S_L1, SEEDS, U, _dev, _dev_args, make_scene,
                                    noisy_prior, pose_dist, right_perturb)
from tests.test_dense_ba_joint_gpu import NO_PRIOR, WEIGHTS

pytestmark = pytest.mark.gpu
SHAPES = [(1, 7, 9), (3, 24, 40), (3, 136, 168)]          # below one wavefront; most workgroups idle; a ragged tail above 64 x 256 threads
NO_SCALE = {(4, 2): 0.0, (5, 6): np.nan, (6, 3): -1.0}          # pixels whose map entry gives no prior


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """test_dense_ba_joint_gpu's scene of a shape with a weight map, and the map restatement under each kernel at the prior and at
    perturbed inverse depths (computed once)."""
    sc = noisy_prior(make_scene(B, H, W, seed=SEEDS[H], noise=0.3), seed=H)
    for (r, c), val in NO_PRIOR.items():
        sc['depth'][:, r, c] = val
    sc['start'] = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    sc['w'] = WEIGHTS[:B].copy()
    rng = np.random.default_rng(H)
    with np.errstate(divide='ignore', invalid='ignore'):
        rho0 = 1.0 / sc['depth'].astype(np.float64)
    sc['rho'] = np.where(np.isfinite(rho0) & (rho0 > 0), rho0 * (1.0 + 0.03 * rng.standard_normal(rho0.shape)), 0.0)
    sc['m'] = np.exp2(np.random.default_rng(H + 1).uniform(-2.0, 2.0, (B, H, W))).astype(np.float32)
    for (r, c), val in NO_SCALE.items():
        sc['m'][:, r, c] = val
    args = (sc['depth'], sc['flow'], sc['mask'], sc['start'], sc['rgb2imu'], sc['intr'], sc['w'], sc['m'])
    refs = {(k, st): ba_map_reference(*args, rho=None if st == 'prior' else sc['rho'], kernel=kern) for k, kern in KERNELS.items()
            for st in ('prior', 'moved')}
    return sc, refs


def _same_bits(a, b):
    """torch.equal on the bit patterns: a variance map holds NaN where a pixel has no prior."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _normal(sc, kind, st, **kw):
    kw.setdefault('prior_scale', _dev(sc['m']))
    return ops.dense_ba_normal(*_dev_args(sc, sc['start']), _dev(sc['w']), inv_depth=None if st == 'prior' else _dev(sc['rho']), rgb2imu=_dev(MOUNT),
                               kernel=KERNELS[kind], **kw)


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_scene_conditions(B, H, W):
    """On the restatement alone, at both states: every clause drops a pixel, at least half the pixels stay, no pixel lies within 1e-9
    of a clause's threshold (so the count must match exactly), and the six pixels without a usable prior are outside the valid set."""
    sc, refs = _case(B, H, W)
    for st in ('prior', 'moved'):
        for r in refs[('none', st)]:
            print('%dx%d %s: kept %d of %d, dropped by clause %s, closest margin %.2e' % (H, W, st, r['count'], H * W, r['rejects'], np.nanmin(r['margin'])))
            assert (r['rejects'] > 0).all()
            assert 2 * r['count'] >= H * W
            assert np.nanmin(r['margin']) > 1e-9
            assert not any(r['valid'][p] or r['prior'][p] for p in list(NO_PRIOR) + list(NO_SCALE)) and (r['rho0'][~r['prior']] == 0).all()
            assert (~r['prior']).sum() == 6
    assert (sc['intr'][:, 0] < W / 2).all() and (~sc['mask']).any()


# ------------------------------------------------------------------------------------------------ 1. the sums with a map
@pytest.mark.parametrize('kind', list(KERNELS))
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_sums_with_a_map_match_restatement(cuda, B, H, W, kind):
    sc, refs = _case(B, H, W)
    worst = 0.0
    for st in ('prior', 'moved'):
        out, again = _normal(sc, kind, st), _normal(sc, kind, st)
        for x, y in zip(out, again):
            assert torch.equal(x, y)
        got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
        for b, r in enumerate(refs[(kind, st)]):
            n = r['count']
            bound = U * (K_MAP + n)
            assert got['count'][b] == n == got['sums'][b, S_COUNT]
            err = np.abs(got['sums'][b] - r['sums'])
            frac = max((err / np.maximum(bound * r['abs'], 1e-300)).max(), (np.abs(got['S'][b] - r['S']) / (bound * r['Sabs'])).max(),
                       (np.abs(got['g'][b] - r['g']) / (bound * r['gabs'])).max())
            worst = max(worst, frac)
            assert (err <= bound * r['abs']).all()
            assert (np.abs(got['S'][b] - r['S']) <= bound * r['Sabs']).all()
            assert (np.abs(got['g'][b] - r['g']) <= bound * r['gabs']).all()
            assert abs(got['cost'][b] - r['cost']) <= bound * r['abs'][S_COST] and got['cost'][b] == got['sums'][b, S_COST]
            assert abs(got['l1'][b] - r['l1']) <= bound * r['abs'][S_L1] and got['l1'][b] == got['sums'][b, S_L1]
            assert np.array_equal(got['S'][b], got['S'][b].T)
    print('%dx%dx%d %s: worst error / bound over sums, S and g: %.4f' % (B, H, W, kind, worst))


# ------------------------------------------------------------------------------------------------ 2. bit-equality with the existing path
@pytest.mark.parametrize('kind', list(KERNELS))
def test_unit_map_gives_the_bits_of_the_scalar_path(cuda, kind):
    """m = 1 everywhere: islam_dense_ba_normal_map gives the bits of islam_dense_ba_normal at both states, and a 20-evaluation
    islam_dense_ba_refine_map the bits of islam_dense_ba_refine; (225, 0.25) gives the bits of (56.25, 1), and (w_b, m) those of
    (4 w_b, m / 4)."""
    sc, _ = _case(3, 24, 40)
    one = torch.ones(sc['m'].shape, dtype=torch.float32, device='cuda')
    for st in ('prior', 'moved'):
        scalar, unit = _normal(sc, kind, st, prior_scale=None), _normal(sc, kind, st, prior_scale=one)
        for k in scalar._fields:
            assert torch.equal(getattr(scalar, k), getattr(unit, k)), (st, k)
    d = _dev_args(sc, sc['start'])
    kw = dict(rgb2imu=_dev(MOUNT), kernel=KERNELS[kind], iters=20, trace_cap=20)
    scalar, unit = ops.dense_ba_refine(*d, _dev(sc['w']), **kw), ops.dense_ba_refine(*d, _dev(sc['w']), prior_scale=one, **kw)
    assert scalar.status.tolist() == [OK] * 3 and scalar.accepted.min().item() >= 1
    for k in scalar._fields:
        assert torch.equal(getattr(scalar, k), getattr(unit, k)), k
    a, b = ops.dense_ba_refine(*d, 225.0, prior_scale=0.25 * one, **kw), ops.dense_ba_refine(*d, 56.25, **kw)
    for k in a._fields:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    m = _dev(sc['m'])
    a, b = ops.dense_ba_refine(*d, _dev(sc['w']), prior_scale=m, **kw), ops.dense_ba_refine(*d, _dev(4 * sc['w']), prior_scale=m / 4, **kw)
    assert a.accepted.min().item() >= 1 and not torch.equal(a.motion, scalar.motion)
    for k in a._fields:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------------------------------------ 3. the refinement with a map
@pytest.mark.parametrize('H,W', [(24, 40), (72, 96)])
def test_refinement_with_a_map_matches_restatement(cuda, H, W):
    """Twenty evaluations on the two-level scene.  Pose and inverse depths within 10 x max(the restatement's last step, the gap between
    its runs with forward and with backward summation) of the restatement's (section 3.25's bound); the returned sums are the bits
    dense_ba_normal(prior_scale=...) gives at the returned state; the inverse-depth RMS error is below the uniform-weight device run's."""
    sc, runs, _, _ = two_level_case(H, W)
    r = runs['sums']
    gap_pose = pose_dist(runs['fwd']['motion'], runs['bwd']['motion'])
    gap_rho = float(np.abs(runs['fwd']['rho'] - runs['bwd']['rho']).max())
    assert r['status'] == OK and r['last_step'] < 1e-6          # conditions on the restatement alone
    d = _dev_args(sc, sc['start'])
    m = _dev(sc['scale'])
    out = ops.dense_ba_refine(*d, SIGMA_PX ** 2, iters=20, prior_scale=m)
    pose, rho = out.motion[0].cpu().numpy(), out.inv_depth[0].cpu().numpy()
    dp, dr = pose_dist(r['motion'], pose), float(np.abs(rho - r['rho'])[r['valid']].max())
    uniform = ops.dense_ba_refine(*d, sc['w_uniform'], iters=20)
    e_map, e_uni = rho_rms(rho, sc), rho_rms(uniform.inv_depth[0].cpu().numpy(), sc)
    print('%dx%d: restatement last step %.3e, forward/backward gap %.3e (pose) %.3e (rho); device: pose %.3e, rho %.3e from the restatement, '
          'accepted %d rejected %d; rho RMS uniform %.4e -> map %.4e' % (H, W, r['last_step'], gap_pose, gap_rho, dp, dr, out.accepted.item(),
                                                                         out.rejected.item(), e_uni, e_map))
    assert out.status.item() == OK and uniform.status.item() == OK and out.accepted.item() + out.rejected.item() == 19
    assert dp <= 10 * max(r['last_step'], gap_pose)
    assert dr <= 10 * max(r['last_step'], gap_rho)
    at = ops.dense_ba_normal(d[0], d[1], d[2], out.motion, d[4], SIGMA_PX ** 2, inv_depth=out.inv_depth, prior_scale=m)
    for k in ('S', 'g', 'cost', 'l1', 'count', 'sums'):
        assert torch.equal(getattr(out, k), getattr(at, k)), k
    assert e_map < e_uni


# ------------------------------------------------------------------------------------------------ 4. the variance
@pytest.mark.parametrize('kind,st', [('none', 'prior'), ('huber', 'moved'), ('cauchy', 'moved')])
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_variance_matches_restatement(cuda, B, H, W, kind, st):
    """Both modes; the device and variance_reference are given the same sums bits (the device's own, from dense_ba_normal with the map).
    |dev - ref| <= 2^-52 (K_v + 64 cond(S_cam)) v with cond asserted below 1e9; the NaN pattern is exact, an invalid pixel with a prior
    carries exactly 1 / (w_b m_i), 1/h_dd <= v <= 1/w_i holds on the device's values up to the bound, a repeat gives equal bits."""
    sc, refs = _case(B, H, W)
    sums = _normal(sc, kind, st).sums
    sums_np = sums.cpu().numpy()
    call = lambda marginal: ops.dense_ba_depth_variance(*_dev_args(sc, sc['start']), _dev(sc['w']), inv_depth=None if st == 'prior' else _dev(sc['rho']),
                                                        sums=sums, prior_scale=_dev(sc['m']), rgb2imu=_dev(MOUNT), kernel=KERNELS[kind],
                                                        marginal=marginal)
    marg, cond_, again = call(True), call(False), call(True)
    assert _same_bits(marg.var, again.var) and marg.status.tolist() == cond_.status.tolist() == [OK] * B
    auto = ops.dense_ba_depth_variance(*_dev_args(sc, sc['start']), _dev(sc['w']), inv_depth=None if st == 'prior' else _dev(sc['rho']),
                                       prior_scale=_dev(sc['m']), rgb2imu=_dev(MOUNT), kernel=KERNELS[kind])
    assert _same_bits(auto.var, marg.var)          # sums=None: dense_ba_normal at the state, the same bits
    vm, vc = marg.var.cpu().numpy(), cond_.var.cpu().numpy()
    worst = 0.0
    for b, r in enumerate(refs[(kind, st)]):
        Scam = scam_from_sums(sums_np[b])
        cond = np.linalg.cond(Scam)
        assert cond < 1e9
        tol = U * (K_VAR + 64 * cond)
        for got, marginal in ((vm[b], True), (vc[b], False)):
            want = variance_reference(r, Scam, marginal)
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 6
            have = ~np.isnan(want)
            frac = (np.abs(got[have] - want[have]) / (tol * want[have])).max()
            worst = max(worst, frac)
            assert frac <= 1.0, (b, marginal, frac)
            inv = r['prior'] & ~r['valid']
            assert inv.sum() > 0 and np.array_equal(got[inv], 1.0 / (sc['w'][b] * sc['m'][b].astype(np.float64)[inv]))
        valid = r['valid']
        assert (vc[b][valid] <= vm[b][valid] * (1 + tol)).all() and (vm[b][valid] <= (1.0 / r['w'][valid]) * (1 + tol)).all()
        assert (vc[b][valid] <= 1.0 / r['w'][valid]).all() and (vm[b][valid] > vc[b][valid]).any()
        print('link %d: cond(S_cam) %.2e, tolerance %.2e relative' % (b, cond, tol))
    print('%dx%dx%d %s %s: worst error / bound %.4f' % (B, H, W, kind, st, worst))


def test_variance_without_a_map(cuda):
    """prior_scale=None is the per-link weight: the bits of m = 1."""
    sc, _ = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    one = torch.ones(sc['m'].shape, dtype=torch.float32, device='cuda')
    kw = dict(inv_depth=_dev(sc['rho']), rgb2imu=_dev(MOUNT), kernel=robust.Cauchy(1.0))
    for marginal in (True, False):
        a = ops.dense_ba_depth_variance(*d, _dev(sc['w']), marginal=marginal, **kw)
        b = ops.dense_ba_depth_variance(*d, _dev(sc['w']), prior_scale=one, marginal=marginal, **kw)
        assert _same_bits(a.var, b.var) and a.status.tolist() == [OK] * 3
        assert torch.isnan(a.var).sum().item() == 3 * len(NO_PRIOR)


# ------------------------------------------------------------------------------------------------ 5. status words
def test_status_marks_only_its_own_link(cuda):
    """NOTPD (an empty mask: S_cam = 0 is finite and has no positive pivot; through a refinement with min_count = 0 and from the sums
    alone), BADPRIOR (a device-side prior weight of 0) and an incoming FEW on the middle link: its status is set and its map is all NaN;
    the healthy links equal a batch without it bit for bit."""
    sc, _ = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    keep = [0, 2]
    w, m, C = _dev(sc['w']), _dev(sc['m']), _dev(MOUNT)
    hs = ops.dense_ba_normal(*(x[keep] for x in d), w[keep], rgb2imu=C, prior_scale=m[keep]).sums
    healthy = ops.dense_ba_depth_variance(*(x[keep] for x in d), w[keep], sums=hs, prior_scale=m[keep], rgb2imu=C)
    assert healthy.status.tolist() == [OK, OK]
    empty = d[2].clone()
    empty[1] = 0
    wb = w.clone()
    wb[1] = 0.0
    ref = ops.dense_ba_refine(d[0], d[1], empty, d[3], d[4], w, rgb2imu=C, iters=4, min_count=0, prior_scale=m)
    assert ref.status.tolist() == [OK, NOTPD, OK]
    full = ops.dense_ba_normal(*d, w, rgb2imu=C, prior_scale=m).sums
    few = torch.tensor([OK, FEW, OK], dtype=torch.int32, device='cuda')
    cases = [('notpd from the sums', empty, w, ops.dense_ba_normal(d[0], d[1], empty, d[3], d[4], w, rgb2imu=C, prior_scale=m).sums, None, NOTPD),
             ('notpd incoming', empty, w, None, 'refine', NOTPD),
             ('badprior', d[2], wb, ops.dense_ba_normal(*d, wb, rgb2imu=C, prior_scale=m).sums, None, BADPRIOR),
             ('few incoming', d[2], w, full, few, FEW)]
    for name, mask, wt, sums, status, want in cases:
        if status == 'refine':          # the state a refinement left: link 1 stands at the start
            out = ops.dense_ba_depth_variance(d[0], d[1], mask, ref.motion, d[4], wt, inv_depth=ref.inv_depth, sums=ref.sums, status=ref.status,
                                              prior_scale=m, rgb2imu=C)
            assert out.status.tolist() == [OK, want, OK] and torch.isnan(out.var[1]).all() and not torch.isnan(out.var[keep]).all()
            continue
        out = ops.dense_ba_depth_variance(d[0], d[1], mask, d[3], d[4], wt, sums=sums, status=status, prior_scale=m, rgb2imu=C)
        torch.cuda.synchronize()
        assert out.status.tolist() == [OK, want, OK], name
        assert torch.isnan(out.var[1]).all(), name
        assert _same_bits(out.var[keep], healthy.var), name
    # conditional on the pose S_cam is not factored: the empty link is all prior, v = 1 / w_i
    out = ops.dense_ba_depth_variance(d[0], d[1], empty, d[3], d[4], w, sums=cases[0][3], prior_scale=m, rgb2imu=C, marginal=False)
    r = _case(3, 24, 40)[1][('none', 'prior')][1]
    got = out.var[1].cpu().numpy()
    assert out.status.tolist() == [OK] * 3 and np.array_equal(got[r['prior']], 1.0 / r['w'][r['prior']]) and np.isnan(got[~r['prior']]).all()


# ------------------------------------------------------------------------------------------------ 6. through DenseReprojectionLoss
def test_depth_uncertainty_closes_the_loop(cuda):
    """The two-level 72 x 96 scene, three of its sigmas marked "no prior" (NaN, 0, -1): refine_joint(sigma map) then depth_uncertainty.
    chi^2/n of the device result over the n pixels with a prior lies in the band of the CPU test, sigma_depth is sigma_inv_depth / rho^2,
    and sigma_inv_depth, NaNs included, is accepted as the prior of a second refine_joint: the NaN pixels come back with rho = 0 and the
    stored depth bits, every status is OK."""
    H, W = 72, 96
    sc, _, _, _ = two_level_case(H, W)
    d = _dev_args(sc, sc['start'])
    fx, fy, cx, cy = sc['intr'][0]
    ident = pp.SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=torch.float64, device='cuda'))
    loss = DenseReprojectionLoss(d[0], d[1], fx, fy, cx, cy, d[2], ident, device='cuda')
    sigma = sc['sigma'].copy()
    none = [(0, 10, 11), (0, 40, 50), (0, 71, 95)]
    for p, val in zip(none, (np.nan, 0.0, -1.0)):
        sigma[p] = val
    sig = _dev(sigma)
    joint = loss.refine_joint(pp.SE3(d[3]), sig, sigma_px=SIGMA_PX, iters=20)
    unc = loss.depth_uncertainty(joint, sig, sigma_px=SIGMA_PX)
    assert joint.status.tolist() == [OK] and unc.status.tolist() == [OK]
    rho, var = joint.inv_depth.cpu().numpy(), unc.var_inv_depth.cpu().numpy()
    have = np.isfinite(var)
    assert (~have).sum() == 3 and all(np.isnan(var[p]) and rho[p] == 0 for p in none)
    chi2 = float(np.mean((rho[have] - sc['rho_true'][have]) ** 2 / var[have]))
    lo, hi = chi2_band(int(have.sum()))
    print('chi^2/n %.3f in %.2f .. %.2f; median sigma_depth %.3f m' % (chi2, lo, hi, float(np.nanmedian(unc.sigma_depth.cpu().numpy()))))
    assert lo <= chi2 <= hi
    assert torch.equal(unc.sigma_inv_depth[joint.inv_depth > 0], torch.sqrt(unc.var_inv_depth)[joint.inv_depth > 0])
    assert torch.equal(unc.sigma_depth[joint.inv_depth > 0], (unc.sigma_inv_depth / (joint.inv_depth * joint.inv_depth))[joint.inv_depth > 0])
    assert torch.isnan(unc.sigma_depth).sum().item() == 3 and torch.isnan(unc.sigma_inv_depth).sum().item() == 3
    conditional = loss.depth_uncertainty(joint, sig, sigma_px=SIGMA_PX, marginal=False)
    assert (conditional.var_inv_depth.cpu().numpy()[have] <= var[have]).all()
    second = loss.refine_joint(joint.motion, unc.sigma_inv_depth, sigma_px=SIGMA_PX, iters=5)
    assert second.status.tolist() == [OK]
    rho2, depth2 = second.inv_depth.cpu().numpy(), second.depth.cpu().numpy()
    for p in none:
        assert rho2[p] == 0 and depth2[p].view(np.int32) == sc['depth'][p].view(np.int32)
    assert (rho2[have] > 0).all()
