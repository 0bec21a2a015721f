"""Depth propagation on the MI355X (csrc/depth_prop.hip: depth_splat_kernel, depth_fuse_kernel) against the
float64 restatement of tests/dense_ba_prop_f64.py.

Scenes: the family's at (1,7,9) (with the large motion of the CPU file's first test, so that several sources land on one target at the
smallest shape too), (3,24,40) and (3,136,168) -- the mount, per-link intrinsics, the user mask, every 17th depth at 0.05 -- with a state
rho = 1/depth (1 + 0.05 U(-1,1)), variances 2^U(-14,-8) of which three are 0, NaN and -1, and a measurement made of the scene's own
depth.  The conditions under which source indices and flags can be compared exactly are asserted on the restatement alone
(test_scene_conditions here and in the CPU file).

Tolerances.  rho' within 2^-52 K_RHO rho', s' within 2^-52 K_VAR s', fused values within 2^-52 K_FUSE of theirs, with K_RHO = 256,
K_VAR = 4 K_RHO + 64, K_FUSE = 2 K_VAR + 4 counted from the definition block in tests/dense_ba_prop_f64.py: the per-pixel arithmetic is
the same sequence of individually rounded operations on both sides, and what differs is T^-1 (32 roundings on an entry), amplified by
the cancellation in Q.z = a / rho + t_z (kappa < 5.5, asserted per scene)."""
import numpy as np
import pytest
import torch

from islam_amd import ops
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseReprojectionLoss
from tests import dense_ba_prop_f64 as prop
from tests.dense_ba_prop_f64 import (FLAG_GATED, FLAG_MEAS, FLAG_PROP, K_FUSE, K_RHO, K_VAR, KAPPA_MAX, SHAPES, SIGMA_PX, SIGMA_STEREO, filter_reference,
                                     gate_margin, multi_targets, prop_case, propagate_reference, scene_margins)
from tests.dense_reproj_f64 import BADPRIOR, FEW, MOUNT, OK, U, _dev

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    """torch.equal on the bit patterns: a variance map holds NaN where nothing is known."""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype in (torch.float64, torch.float32):
        view = torch.int64 if a.dtype == torch.float64 else torch.int32
        a, b = a.view(view), b.view(view)
    return a.shape == b.shape and torch.equal(a, b)


def _call(sc, links=None, **kw):
    pick = (lambda a: a) if links is None else (lambda a: a[links])
    for k in ('depth_next', 'var_next', 'status', 'process_var'):
        if k in kw and kw[k] is not None and not np.isscalar(kw[k]):
            kw[k] = pick(_dev(kw[k]))
    return ops.dense_ba_depth_propagate(pick(_dev(sc['rho'])), pick(_dev(sc['var'])), pick(_dev(sc['motion'])), pick(_dev(sc['intr'])),
                                        mask=pick(_dev(sc['mask'])), rgb2imu=_dev(MOUNT), **kw)


def _np(out):
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


def _check(got, refs, k_rho, k_var, exact=lambda r: np.zeros(r['flags'].shape, bool)):
    """source, flags and the NaN pattern exact; values within their bounds, bit-equal where ``exact`` says so (the measurement alone).
    Returns the worst used share of the bound."""
    worst = 0.0
    for b, r in enumerate(refs):
        assert np.array_equal(got['source'][b], r['source']) and np.array_equal(got['flags'][b], r['flags']), b
        assert got['status'][b] == r['status']
        have = r['flags'] != 0
        assert np.array_equal(np.isnan(got['var_inv_depth'][b]), ~have) and (got['inv_depth'][b][~have] == 0).all()
        ex = exact(r)
        assert np.array_equal(got['inv_depth'][b][ex], r['inv_depth'][ex]) and np.array_equal(got['var_inv_depth'][b][ex], r['var_inv_depth'][ex])
        fr = np.abs(got['inv_depth'][b] - r['inv_depth'])[have] / (U * k_rho * r['inv_depth'][have])
        fs = np.abs(got['var_inv_depth'][b] - r['var_inv_depth'])[have] / (U * k_var * r['var_inv_depth'][have])
        assert fr.max() <= 1.0 and fs.max() <= 1.0, (b, fr.max(), fs.max())
        worst = max(worst, float(fr.max()), float(fs.max()))
        # the float32 depth: the rounding of 1 / rho_f (of the device's own rho_f), or the bits standing in for "nothing"
        with np.errstate(divide='ignore'):
            assert np.array_equal(got['depth'][b][have], (1.0 / got['inv_depth'][b][have]).astype(np.float32))
    return worst


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_scene_conditions(B, H, W):
    """On the restatement alone (the CPU file prints the figures): rounding distance > 1e-9, relative z-gap > 1e-5, no gate decision
    within 1e-9 of gate^2, kappa below the bound in K_RHO, at least 40 % of the targets hit at the two larger shapes, several
    candidates on one target at every shape."""
    sc, refs = prop_case(B, H, W)
    for b in range(B):
        m = scene_margins(refs['pure'][b])
        assert m.rounding > 1e-9 and m.zgap > 1e-5 and m.qz > 1e-9 and m.kappa < KAPPA_MAX
        assert gate_margin(refs['gate3'][b], sc['depth_next'][b], sc['var_next'][b], 3.0) > 1e-9
        assert (m.hit >= 0.4 or H == 7) and multi_targets(refs['pure'][b]) >= (5 if H == 7 else 50)


# ------------------------------------------------------------------------------------------------ 1. pure propagation
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_pure_propagation_matches_restatement(cuda, B, H, W):
    """source and flags equal the restatement's exactly, rho' and s' lie within 2^-52 K |value|, a repeat gives the same bits, and
    without a measurement out_depth is the float32 of 1 / rho' or 0."""
    sc, refs = prop_case(B, H, W)
    out, again = _call(sc), _call(sc)
    for x, y in zip(out, again):
        assert _same_bits(x, y)
    got = _np(out)
    worst = _check(got, refs['pure'], K_RHO, K_VAR)
    assert (got['depth'][got['source'] < 0] == 0).all() and (got['flags'] <= FLAG_PROP).all() and got['status'].tolist() == [OK] * B
    print('%dx%dx%d: worst error / bound over rho\' and s\': %.4f' % (B, H, W, worst))
    # a process variance adds to s' and changes nothing else
    q = np.array([1e-6, 3e-5, 2e-4][:B])
    moved = _np(_call(sc, process_var=q))
    assert np.array_equal(moved['source'], got['source']) and np.array_equal(moved['inv_depth'], got['inv_depth'])
    hit = got['source'] >= 0
    assert np.array_equal(moved['var_inv_depth'][hit], (got['var_inv_depth'] + q[:, None, None])[hit])


def test_equal_fp32_keys_go_to_the_smaller_source_index(cuda):
    """The hand-placed tie of the CPU file: two sources whose rho' agree after rounding to fp32 land on one target; the smaller index
    wins although the other is nearer in fp64.  A gap fp32 can see goes to the nearer one."""
    from tests.test_depth_propagate_cpu import tie_scene
    for rel, want in ((1e-12, 5), (-1e-12, 5), (1e-3, 6), (-1e-3, 5)):
        rho, var, _, motion, _, intr = tie_scene(rel)
        out = ops.dense_ba_depth_propagate(_dev(rho[None]), _dev(var[None]), _dev(motion[None]), _dev(intr))
        assert out.source[0, 0].tolist() == [-1, -1, -1, -1, want, -1, -1], rel
        ref = prop.propagate_reference_link(rho, var, None, motion, None, intr)
        assert np.array_equal(out.inv_depth[0].cpu().numpy(), ref['inv_depth'])          # identity pose: the same bits


# ------------------------------------------------------------------------------------------------ 2. fusion with a measurement
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_fusion_matches_restatement(cuda, B, H, W):
    """gate = 3: flags exact (no decision within 1e-9 of the threshold, asserted on the restatement), fused values within the bound, the
    measurement's bits where it stands alone or wins the gate; gate = 0 sets bit 2 nowhere."""
    sc, refs = prop_case(B, H, W)
    meas = dict(depth_next=sc['depth_next'], var_next=sc['var_next'])
    alone = lambda r: (r['flags'] == FLAG_MEAS) | ((r['flags'] & FLAG_GATED) != 0)
    g3 = _np(_call(sc, gate=3.0, **meas))
    worst = _check(g3, refs['gate3'], K_FUSE, K_FUSE, exact=alone)
    g0 = _np(_call(sc, gate=0.0, **meas))
    worst = max(worst, _check(g0, refs['gate0'], K_FUSE, K_FUSE, exact=lambda r: r['flags'] == FLAG_MEAS))
    assert not (g0['flags'] & FLAG_GATED).any() and (g3['flags'] & FLAG_GATED).sum() >= 10
    for b, r in enumerate(refs['gate3']):
        own = alone(r)
        assert np.array_equal(g3['depth'][b][own].view(np.int32), sc['depth_next'][b][own].view(np.int32))
        none = r['flags'] == 0
        assert np.array_equal(g3['depth'][b][none].view(np.int32), sc['depth_next'][b][none].view(np.int32))          # 0, NaN, -1 pass through
    print('%dx%dx%d: worst error / bound over the fused values: %.4f; gated %d of %d with both' % (
        B, H, W, worst, (g3['flags'] & FLAG_GATED).astype(bool).sum(), ((g3['flags'] & 3) == 3).sum()))


# ------------------------------------------------------------------------------------------------ 3. a planted moving patch
def test_planted_patch_is_gated(cuda):
    """24 x 40, the measurement equal to the propagated depth (float32) with small variances, except an 8 x 8 block at half its depth: a
    moving object.  Inside the block exactly the restatement's pixels are gated (at least 20 per link; a propagated value whose own variance is large
    stays) and carry the measurement's bits; outside nothing is."""
    sc, refs = prop_case(3, 24, 40)
    pure = refs['pure']
    with np.errstate(divide='ignore'):
        dn = np.stack([np.where(r['source'] >= 0, 1.0 / r['inv_depth'], sc['depth'][b]) for b, r in enumerate(pure)]).astype(np.float32)
    block = np.zeros(dn.shape, bool)
    block[:, 8:16, 16:24] = True
    dn[block] *= np.float32(0.5)
    vn = np.full(dn.shape, 2.0 ** -12, np.float32)
    want = propagate_reference(sc['rho'], sc['var'], sc['mask'], sc['motion'], MOUNT, sc['intr'], depth_next=dn, var_next=vn, gate=3.0)
    got = _np(_call(sc, depth_next=dn, var_next=vn, gate=3.0))
    _check(got, want, K_FUSE, K_FUSE, exact=lambda r: (r['flags'] & FLAG_GATED) != 0)
    for b, r in enumerate(want):
        assert gate_margin(r, dn[b], vn[b], 3.0) > 1e-9          # a condition on the restatement
        gated = (r['flags'] & FLAG_GATED) != 0
        assert gated[block[b]].sum() >= 20 and not gated[~block[b]].any()
        assert np.array_equal((got['flags'][b] & FLAG_GATED) != 0, gated)
        assert np.array_equal(got['depth'][b][gated].view(np.int32), dn[b][gated].view(np.int32))
        assert np.array_equal(got['inv_depth'][b][gated], 1.0 / dn[b][gated].astype(np.float64)) and (got['var_inv_depth'][b][gated] == 2.0 ** -12).all()


# ------------------------------------------------------------------------------------------------ 4. status words
def test_status_marks_only_its_own_link(cuda):
    """An incoming FEW, and a device-side process_var of -1 (BADPRIOR), on the middle link: it propagates nothing and returns the
    measurement alone; the healthy links equal a batch without it bit for bit."""
    sc, _ = prop_case(3, 24, 40)
    meas = dict(depth_next=sc['depth_next'], var_next=sc['var_next'], gate=3.0)
    keep = [0, 2]
    healthy = _call(sc, links=keep, **meas)
    assert healthy.status.tolist() == [OK, OK]
    for name, kw, want in (('few', dict(status=np.array([OK, FEW, OK], np.int32)), FEW), ('badprior', dict(process_var=np.array([0.0, -1.0, 0.0])), BADPRIOR),
                           ('nan', dict(process_var=np.array([0.0, np.nan, 0.0])), BADPRIOR)):
        out = _call(sc, **kw, **meas)
        assert out.status.tolist() == [OK, want, OK], name
        for k in ('inv_depth', 'var_inv_depth', 'depth', 'source', 'flags'):
            assert _same_bits(getattr(out, k)[keep], getattr(healthy, k)), (name, k)
        assert (out.source[1] == -1).all() and ((out.flags[1] | FLAG_MEAS) == FLAG_MEAS).all(), name
        assert _same_bits(out.depth[1], _dev(sc['depth_next'][1])), name
        present = out.flags[1] == FLAG_MEAS
        assert present.sum().item() == 24 * 40 - 3 and torch.isnan(out.var_inv_depth[1][~present]).all()
        assert torch.equal(out.var_inv_depth[1][present], _dev(sc['var_next'][1]).double()[present]), name
    out = _call(sc, status=np.array([OK, FEW, OK], np.int32))          # without a measurement: nothing at all
    assert out.status.tolist() == [OK, FEW, OK] and (out.flags[1] == 0).all() and (out.inv_depth[1] == 0).all() and (out.depth[1] == 0).all()
    assert torch.isnan(out.var_inv_depth[1]).all() and (out.flags[keep] == FLAG_PROP).any()


# ------------------------------------------------------------------------------------------------ 5. through DenseReprojectionLoss
def test_recursive_filter_through_the_loss(cuda):
    """plane_sequence 48 x 64, three links: refine_joint(sigma map) -> depth_uncertainty -> propagate -> the next link's
    DenseReprojectionLoss(depth=prior.depth) and refine_joint(sigma_inv_depth=prior.sigma_inv_depth), NaNs included.  Every status is
    OK; over the last frame's pixels flagged "both, not gated" the fused inverse-depth RMS error is strictly below the stereo map's;
    RMS and chi^2/n agree with the CPU restatement's to section 3.27's refinement bound, 10 x the restatement's own last step (the
    largest over the three links).  Every 37th pixel of the later frames' stereo maps carries no measurement, so every prior has pixels
    with a propagated value only and pixels with nothing at all (sigma NaN, asserted on the restatement and on the device), and the
    next link's refine_joint takes them as "no prior at this pixel"."""
    H, W, K = 48, 64, 3
    seq, priors, runs, want = filter_reference(H, W, K)
    fx, fy, cx, cy = seq['intr']
    ident = pp.SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=torch.float64, device='cuda'))
    depth, sigma = _dev(seq['stereo'][0])[None], torch.full((1, H, W), SIGMA_STEREO, dtype=torch.float64, device='cuda')
    for k in range(K):
        loss = DenseReprojectionLoss(depth, _dev(seq['flow'][k])[None], fx, fy, cx, cy, None, ident, device='cuda')
        joint = loss.refine_joint(pp.SE3(_dev(seq['start'][k])[None]), sigma, sigma_px=SIGMA_PX, iters=20)
        unc = loss.depth_uncertainty(joint, sigma, sigma_px=SIGMA_PX)
        no_prior = torch.isnan(sigma)          # from the second link on: the pixels the previous propagate left with nothing
        assert (no_prior.sum().item() > 0) == (k > 0) and (joint.inv_depth[no_prior] == 0).all() and torch.isnan(unc.var_inv_depth[no_prior]).all()
        assert (joint.inv_depth[~no_prior] > 0).all()
        prior = loss.propagate(joint, unc, depth_next=_dev(seq['stereo'][k + 1])[None], sigma_inv_depth_next=SIGMA_STEREO,
                               process_sigma=float(np.sqrt(seq['process_var'][k + 1])), gate=3.0)
        assert joint.status.tolist() == [OK] and unc.status.tolist() == [OK] and prior.status.tolist() == [OK], k
        none = prop.filter_stats(priors[k], seq, k + 1)['none']
        assert none > 0 and (priors[k]['flags'] == FLAG_PROP).sum() > 0          # conditions on the restatement
        assert torch.isnan(prior.sigma_inv_depth).sum().item() == (prior.flags == 0).sum().item() == none
        assert _same_bits(prior.sigma_inv_depth, torch.sqrt(prior.var_inv_depth))
        depth, sigma = prior.depth, prior.sigma_inv_depth
    got = prop.filter_stats({k: getattr(prior, k)[0].cpu().numpy() for k in ('flags', 'inv_depth', 'var_inv_depth')}, seq, K)
    step = max(r['last_step'] for r in runs)
    print('last frame: %.1f %% fused; rho RMS stereo %.4e -> fused %.4e (restatement %.4e); chi^2/n %.4f (restatement %.4f); '
          'bound %.2e; differences %.2e and %.2e' % (
              100 * got['share'], got['rms_stereo'], got['rms'], want['rms'], got['chi2'], want['chi2'], 10 * step,
              abs(got['rms'] - want['rms']), abs(got['chi2'] - want['chi2'])))
    assert got['share'] >= 0.5 and got['n'] == want['n']
    assert got['rms'] < got['rms_stereo']
    assert abs(got['rms'] - want['rms']) <= 10 * step
    assert abs(got['chi2'] - want['chi2']) <= 10 * step
