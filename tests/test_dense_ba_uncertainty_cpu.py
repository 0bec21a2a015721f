"""Per-pixel prior weights and the posterior variance of the inverse depths (include/islam_hip.h, islam_dense_ba_normal_map /
_refine_map / _depth_var): everything about the float64 numpy restatement (tests/dense_ba_var_f64.py) that can be
checked without a GPU -- the variance against the diagonal of the explicitly inverted joint matrix, the ordering 1/h_dd <= v <= 1/w_i,
the map restatement against the one-weight restatement, the calibration of the predicted variance on planted scenes -- and the
host-side argument errors, the Python plumbing and the register metadata of the new kernels."""
import os

import numpy as np
import pytest
import torch

from islam_amd import robust
from tests.dense_ba_var_f64 import (SIGMA_PX, ba_map_reference_link, chi2_band, dense_system_map, rho_rms, scam_from_sums, two_level_case,
                                    variance_reference)
from tests.dense_reproj_f64 import MOUNT, OK, PRIOR_W, ba_reference_link, make_scene, noisy_prior, right_perturb

EPS = np.finfo(np.float64).eps


def _schur_scene(mapped):
    """The scene of test_schur_sums_are_the_schur_complement_of_the_dense_system (tests/test_dense_ba_joint_cpu.py): 7 x 9, seed 107, the
    mount, a user mask, every clause dropping pixels, a perturbed rho, Cauchy(1.0), w = 1 -- with m = 1 or a map between 0.25 and 4."""
    sc = noisy_prior(make_scene(1, 7, 9, seed=107, noise=0.3), seed=1)
    start = right_perturb(sc['motion'][0], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    rho = (1.0 / sc['depth'][0].astype(np.float64)) * (1.0 + 0.03 * np.random.default_rng(4).standard_normal((7, 9)))
    m = np.exp2(np.random.default_rng(5).uniform(-2.0, 2.0, (7, 9))).astype(np.float32) if mapped else np.ones((7, 9), np.float32)
    r = ba_map_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], start, MOUNT, sc['intr'][0], 1.0, m, rho, robust.Cauchy(1.0))
    assert (r['rejects'] > 0).all() and 2 * r['count'] >= 63 and (~np.asarray(sc['mask'][0])).any() and r['prior'].all()
    assert mapped == (np.unique(r['w']).size > 10)
    return r


# ------------------------------------------------------------------------------------------------ 1. the variance is the inverse's diagonal
@pytest.mark.parametrize('mapped', [False, True], ids=['w=1', 'map'])
def test_variance_is_the_diagonal_of_the_inverted_joint_matrix(mapped):
    """The marginal v equals the depth part of the diagonal of the inverse of the explicit (6 + n) x (6 + n) matrix, the conditional v
    the diagonal of the inverse of its depth block, entry by entry to 64 eps cond relative (cond asserted below 1e9; measured 1.4e3 and
    errors of a few 1e-16)."""
    r = _schur_scene(mapped)
    Mx, idx = dense_system_map(r)
    assert Mx.shape[0] == 6 + 63
    cond = np.linalg.cond(Mx)
    Scam = scam_from_sums(r['sums'])
    want_marg = np.diag(np.linalg.inv(Mx))[6:]
    want_cond = np.diag(np.linalg.inv(Mx[6:, 6:]))
    got_marg = variance_reference(r, Scam, True).ravel()[idx]
    got_cond = variance_reference(r, Scam, False).ravel()[idx]
    errs = [np.abs(got_marg / want_marg - 1).max(), np.abs(got_cond / want_cond - 1).max()]
    print('cond %.3e, bound %.3e; relative errors: marginal %.3e, conditional %.3e' % (cond, 64 * EPS * cond, *errs))
    assert cond < 1e9
    assert max(errs) <= 64 * EPS * cond
    assert (got_marg[r['valid'].ravel()[idx]] > 1.01 * got_cond[r['valid'].ravel()[idx]]).any()          # the pose's uncertainty matters


# ------------------------------------------------------------------------------------------------ 2. ordering
@pytest.mark.parametrize('mapped', [False, True], ids=['w=1', 'map'])
def test_variances_are_ordered(mapped):
    """1/h_dd <= v <= 1/w_i at every valid pixel (a measurement never removes information), with the slack of test 1's bound, and
    v = 1/w_i exactly at an invalid pixel with a prior."""
    r = _schur_scene(mapped)
    Scam = scam_from_sums(r['sums'])
    slack = 64 * EPS * np.linalg.cond(dense_system_map(r)[0])
    valid, inv = r['valid'], r['prior'] & ~r['valid']
    assert valid.sum() > 20 and inv.sum() > 5
    for marginal in (True, False):
        v = variance_reference(r, Scam, marginal)
        assert (v[valid] >= (1.0 / r['hdd'][valid]) * (1 - slack)).all()
        assert (v[valid] <= (1.0 / r['w'][valid]) * (1 + slack)).all()
        assert np.array_equal(v[inv], 1.0 / r['w'][inv])
    assert (variance_reference(r, Scam, True)[valid] < 0.99 / r['w'][valid]).any()


# ------------------------------------------------------------------------------------------------ 3. the map restatement
def test_map_restatement_against_the_one_weight_restatement():
    """m = 1 gives the 30 sums of ba_reference_link bit for bit; (w_b, m) and (4 w_b, m / 4) give equal bits; a pixel whose m is 0, NaN
    or negative is outside the valid set and carries rho0 = 0."""
    sc = noisy_prior(make_scene(1, 24, 40, seed=124, noise=0.3), seed=24)
    start = right_perturb(sc['motion'][0], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    args = (sc['depth'][0], sc['flow'][0], sc['mask'][0], start, MOUNT, sc['intr'][0])
    rho = (1.0 / sc['depth'][0].astype(np.float64)) * (1.0 + 0.03 * np.random.default_rng(24).standard_normal((24, 40)))
    for kern in (None, robust.Huber(1.0)):
        one = ba_reference_link(*args, PRIOR_W, rho, kern)
        same = ba_map_reference_link(*args, PRIOR_W, np.ones((24, 40), np.float32), rho, kern)
        for k in ('sums', 'abs', 'fwd', 'bwd', 'hdd', 'gd', 'hpd'):
            assert np.array_equal(one[k], same[k]), k
        assert one['count'] == same['count'] > 400
    m = np.exp2(np.random.default_rng(7).uniform(-2.0, 2.0, (24, 40))).astype(np.float32)
    a, b = ba_map_reference_link(*args, 100.0, m, rho), ba_map_reference_link(*args, 400.0, m / np.float32(4), rho)
    for k in ('sums', 'fwd', 'bwd', 'hdd', 'gd', 'w'):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a['sums'], ba_reference_link(*args, 100.0, rho)['sums'])
    where = np.argwhere(a['valid'])[[5, 200, 400]]          # three pixels that are valid with the map as it stands
    gone = {tuple(p): val for p, val in zip(where, (0.0, np.nan, -1.0))}
    for p, val in gone.items():
        m[p] = val
    c = ba_map_reference_link(*args, 100.0, m, rho)
    assert c['count'] == a['count'] - 3 and not any(c['valid'][p] or c['prior'][p] or c['rho0'][p] for p in gone)


# ------------------------------------------------------------------------------------------------ 4. calibration and the use of the map
@pytest.mark.parametrize('H,W', [(24, 40), (72, 96)])
def test_map_lowers_the_depth_error_and_the_variance_is_calibrated(H, W):
    """The two-level scene (sigma = 0.01 / 0.03 on even / odd columns, 0.3 px of flow noise), 20 evaluations, seed 0: the inverse-depth
    RMS error with the map is strictly below the one with the uniform weight 0.09 / mean(sigma^2), and the mean over the n = H W pixels
    of (rho - rho_true)^2 / (sigma_px^2 v), v marginal at the map run's final state, lies within 1 +- 4 sqrt(2 / n).  Measured with the
    restatement: 24 x 40  2.0202e-2 -> 2.0106e-2, chi^2/n 0.965 (band 0.82 .. 1.18);  72 x 96  1.7444e-2 -> 1.6292e-2, 0.987 (0.93 .. 1.07)."""
    sc, runs, uniform, at = two_level_case(H, W)
    r = runs['sums']
    assert r['status'] == OK and uniform['status'] == OK and r['accepted'] + r['rejected'] == 19
    e_map, e_uni = rho_rms(r['rho'], sc), rho_rms(uniform['rho'], sc)
    v = variance_reference(at, scam_from_sums(at['sums']), True)
    assert np.isfinite(v).all()
    chi2 = float(np.mean((r['rho'] - sc['rho_true'][0]) ** 2 / (SIGMA_PX ** 2 * v)))
    lo, hi = chi2_band(H * W)
    print('%dx%d: rho RMS uniform %.4e -> map %.4e; chi^2/n %.3f in %.2f .. %.2f; last step %.1e' % (H, W, e_uni, e_map, chi2, lo, hi, r['last_step']))
    assert e_map < e_uni
    assert lo <= chi2 <= hi


# ------------------------------------------------------------------------------------------------ 5. error paths and plumbing
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    one = 1        # any non-NULL address: a refused call never reads it

    def normal(B=1, H=2, W=2, kind=0, delta=1.0, depth=one, out=one, scratch=one, prior=one, scale=one):
        return lib.islam_dense_ba_normal_map(depth, one, None, one, None, one, prior, scale, None, kind, delta, out, one, one, one, one, one, scratch,
                                             B, H, W, None)

    def refine(B=1, H=2, W=2, kind=0, delta=1.0, iters=3, status=one, trace=None, cap=0, damping=1e-4, prior=one, rho=one, scale=one):
        return lib.islam_dense_ba_refine_map(one, one, None, one, None, one, prior, scale, kind, delta, iters, damping, 16.0, one, rho, one, one, one,
                                             one, one, one, one, one, one, status, trace, cap, one, B, H, W, None)

    def var(B=1, H=2, W=2, kind=0, delta=1.0, mode=0, depth=one, prior=one, sums=one, out=one, status=one, scratch=one):
        return lib.islam_dense_ba_depth_var(depth, one, None, one, None, one, prior, None, None, sums, None, kind, delta, mode, out, status, scratch,
                                            B, H, W, None)

    common = ((dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
              (dict(kind=3), b'robust kind'), (dict(kind=-1), b'robust kind'), (dict(kind=1, delta=0.0), b'delta'), (dict(delta=-2.0), b'delta'),
              (dict(delta=float('nan')), b'delta'), (dict(prior=None), b'prior_weight'))
    for call, name, more in ((normal, b'islam_dense_ba_normal_map', ((dict(scale=None), b'prior_scale'), (dict(depth=None), b'NULL'),
                                                                       (dict(out=None), b'NULL'), (dict(scratch=None), b'NULL'))),
                             (refine, b'islam_dense_ba_refine_map', ((dict(scale=None), b'prior_scale'), (dict(iters=0), b'iters'),
                                                                       (dict(status=None), b'NULL'), (dict(cap=4), b'trace'),
                                                                       (dict(damping=-1.0), b'damping'), (dict(rho=None), b'out_inv_depth'))),
                             (var, b'islam_dense_ba_depth_var', ((dict(mode=2), b'mode'), (dict(mode=-1), b'mode'), (dict(depth=None), b'NULL'),
                                                                  (dict(sums=None), b'NULL sums'), (dict(out=None), b'NULL sums'),
                                                                  (dict(status=None), b'NULL sums'), (dict(scratch=None), b'NULL sums')))):
        for kw, what in common + more:
            assert call(**kw) == -1, (name, kw)
            msg = lib.islam_last_error()
            assert name in msg and what in msg, (kw, msg)
    assert lib.islam_dense_ba_depth_var_scratch_bytes(0) == 0 and lib.islam_dense_ba_depth_var_scratch_bytes(3) >= 3 * 21 * 8


def _cpu_loss(sc):
    from islam_amd import lietensor as pp
    from islam_amd.dense_ba import DenseReprojectionLoss
    fx, fy, cx, cy = sc['intr'][0]
    return DenseReprojectionLoss(torch.from_numpy(sc['depth']), torch.from_numpy(sc['flow']), fx, fy, cx, cy, torch.from_numpy(sc['mask']),
                                 pp.SE3(torch.from_numpy(MOUNT)), device='cpu')


def test_ops_refuse_cpu_tensors():
    from islam_amd import ops
    from islam_amd.dense_ba import DenseBAJoint
    sc = make_scene(2, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (t(sc['depth']), t(sc['flow']), t(sc['mask']), t(sc['motion']), t(sc['intr']))
    m = torch.ones(2, 7, 9)
    with pytest.raises(RuntimeError):
        ops.dense_ba_normal(*args, 2500.0, prior_scale=m)
    with pytest.raises(RuntimeError):
        ops.dense_ba_refine(*args, 2500.0, iters=3, prior_scale=m)
    with pytest.raises(RuntimeError):
        ops.dense_ba_depth_variance(*args, 2500.0)
    with pytest.raises(RuntimeError):
        ops.dense_ba_depth_variance(*args, 2500.0, sums=torch.ones(2, 30, dtype=torch.float64), prior_scale=m, marginal=False)
    loss = _cpu_loss(sc)
    with pytest.raises(RuntimeError):
        loss.refine_joint(t(sc['motion']), 0.02 * m)
    joint = DenseBAJoint(*([None] * 14))._replace(motion=t(sc['motion']), inv_depth=1.0 / t(sc['depth']).double(),
                                                  sums=torch.ones(2, 30, dtype=torch.float64), status=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        loss.depth_uncertainty(joint, 0.02 * m)


def test_python_argument_rules(monkeypatch):
    """A (B,H,W) sigma is accepted and becomes prior_weight = sigma_px^2, prior_scale = float32(1 / sigma^2) with 0 where sigma is not
    finite or not positive (information and refine_joint, seen by patching ops); a (2,2) sigma still raises; differentiable=True with a
    map raises NotImplementedError; numbers and (B,) tensors reach ops without a prior_scale."""
    from islam_amd import ops
    sc = make_scene(2, 7, 9, seed=1)
    loss, motion = _cpu_loss(sc), torch.from_numpy(sc['motion'])
    sig = torch.from_numpy(np.random.default_rng(3).uniform(0.01, 0.05, (2, 7, 9)))
    sig[0, 2, 5], sig[1, 3, 1], sig[0, 1, 7], sig[1, 0, 0] = 0.0, float('nan'), -1.0, float('inf')
    ok = torch.isfinite(sig) & (sig > 0)
    want = torch.where(ok, 1.0 / torch.where(ok, sig, torch.ones_like(sig)) ** 2, torch.zeros_like(sig)).to(torch.float32)
    assert (want == 0).sum() == 4
    calls = []
    Hm = torch.arange(72, dtype=torch.float64).reshape(2, 6, 6)

    def normal(depth, flow, mask, mo, intr, w, inv_depth=None, rgb2imu=None, kernel=None, **kw):
        calls.append(('normal', w, kw))
        return ops.DenseBANormal(Hm, None, None, None, None, None)

    def refine(depth, flow, mask, mo, intr, w, rgb2imu=None, kernel=None, iters=20, damping=1e-4, min_count=16, trace_cap=0, **kw):
        calls.append(('refine', w, kw))
        rho = torch.ones(2, 7, 9, dtype=torch.float64)
        return ops.DenseBARefined(mo, rho, *([None] * 11))

    monkeypatch.setattr(ops, 'dense_ba_normal', normal)
    monkeypatch.setattr(ops, 'dense_ba_refine', refine)
    assert torch.equal(loss.information(motion, sigma_px=0.5, sigma_inv_depth=sig), Hm / 0.25)
    loss.refine_joint(motion, sig, sigma_px=0.5)
    loss.refine_joint(motion, sig.float(), sigma_px=0.5)
    assert [c[0] for c in calls] == ['normal', 'refine', 'refine']
    for name, w, kw in calls[:2]:
        assert w == 0.25 and list(kw) == ['prior_scale'], name
        assert kw['prior_scale'].dtype == torch.float32 and torch.equal(kw['prior_scale'], want), name
    assert calls[2][1] == 0.25 and torch.equal(calls[2][2]['prior_scale'] == 0, want == 0)
    del calls[:]
    loss.refine_joint(motion, 0.02, sigma_px=0.5)
    loss.information(motion, sigma_px=0.5, sigma_inv_depth=torch.tensor([0.02, 0.04], dtype=torch.float64))
    assert calls[0][1:] == ((0.5 / 0.02) ** 2, {}) and calls[1][2] == {}
    assert torch.equal(calls[1][1], (0.5 / torch.tensor([0.02, 0.04], dtype=torch.float64)) ** 2)
    for bad in (torch.ones(2, 2), torch.ones(2, 7, 8), torch.ones(1, 7, 9), torch.ones(2, 7, 9, 1)):
        with pytest.raises(ValueError, match='sigma_inv_depth'):
            loss.refine_joint(motion, bad)
        with pytest.raises(ValueError, match='sigma_inv_depth'):
            loss.information(motion, sigma_inv_depth=bad)
    with pytest.raises(NotImplementedError, match='map'):
        loss.refine_joint(motion, sig, differentiable=True)


def test_new_kernels_have_no_private_segment_and_no_spill(lib):
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = _kernels()
    for want in ('ba_wmap_partial_kernel', 'depth_var_factor_kernel', 'depth_var_pixel_kernel'):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        blk = ks[found[0]]
        print(want, 'vgpr', _field(blk, 'vgpr_count'), 'sgpr', _field(blk, 'sgpr_count'), 'lds', _field(blk, 'group_segment_fixed_size'))
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, want
