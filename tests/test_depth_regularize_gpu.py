"""Regularisation of a propagated inverse-depth map on the MI355X (csrc/depth_prop.hip: depth_regularize_kernel; DESIGN.md section
3.29) against the float64 restatement of tests/dense_ba_reg_f64.py.

Inputs: the restatement's own pure propagations of the family's scenes at (1,7,9) (below one 32 x 8 tile), (3,24,40) and (3,136,168)
(6 x 17 tiles, the last column 8 pixels wide; a crop to 21 x 37 makes the last row of tiles ragged as well), as numpy arrays: 26 - 44 %
holes, several surfaces side by side.  The device and the
restatement start from the same bits and run the same individually rounded IEEE operations in the same order (the kernel contracts
nothing, the restatement never reduces pairwise), so every comparison here is exact: rho_f and s_f bit for bit, the float32 depth,
source and flags."""
import math

import numpy as np
import pytest
import torch

from islam_amd import ops
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseReprojectionLoss, DepthRegularizer
from tests import dense_ba_prop_f64 as prop
from tests import dense_ba_reg_f64 as reg
from tests.dense_ba_prop_f64 import FLAG_MEAS, SHAPES, SIGMA_PX, SIGMA_STEREO, filter_reference, prop_case
from tests.dense_ba_reg_f64 import DEFAULTS, FLAG_FILLED, FLAG_REMOVED, filter_reference_reg, leak_counts, leak_scene, regularize_reference
from tests.dense_reproj_f64 import BADPRIOR, FEW, OK, _dev
from tests.test_depth_propagate_gpu import _np, _same_bits

pytestmark = pytest.mark.gpu

RADII = [(1, 1, 1), (2, 2, 2), (0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0)]
DIST_VAR = np.array([2.0 ** -14, 0.0, 3e-6])          # per link: the smoothing weights differ from link to link


def _stages(radii, **kw):
    return dict(DEFAULTS, occl_radius=radii[0], fill_radius=radii[1], smooth_radius=radii[2], **kw)


def _call(pure, links=None, **kw):
    """ops.dense_ba_depth_regularize on the pure propagation of a scene (a list of propagate_reference_link dicts), or on some links."""
    links = list(range(len(pure))) if links is None else links
    stack = lambda k: _dev(np.stack([pure[b][k] for b in links]))
    for k in ('depth_next', 'var_next', 'status', 'dist_var'):
        if k in kw and kw[k] is not None and not np.isscalar(kw[k]):
            kw[k] = _dev(np.asarray(kw[k])[links])
    kw.setdefault('status', _dev(np.array([pure[b]['status'] for b in links], np.int32)))
    return ops.dense_ba_depth_regularize(stack('inv_depth'), stack('var_inv_depth'), source=stack('source'), **kw)


def _equal(got, refs):
    """Every output of every link against the restatement: exact."""
    for b, r in enumerate(refs):
        assert got['status'][b] == r['status'], b
        assert np.array_equal(got['flags'][b], r['flags']) and np.array_equal(got['source'][b], r['source']), b
        for k in ('inv_depth', 'var_inv_depth'):
            diff = got[k][b].view(np.int64) != np.ascontiguousarray(r[k]).view(np.int64)
            assert not diff.any(), (b, k, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(got['depth'][b].view(np.int32), r['depth'].view(np.int32)), b


# ------------------------------------------------------------------------------------------------ 1. the stages against the restatement
@pytest.mark.parametrize('radii', RADII)
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_regularisation_matches_restatement_bit_for_bit(cuda, B, H, W, radii):
    """Without a measurement, and with the scene's measurement at gate 3 and gate 0: flags, source, rho_f, s_f and the float32 depth equal
    the restatement's exactly; a repeat gives the same bits; every link of the batch equals its single-link run; with all radii 0 and no
    measurement the output is the input."""
    sc, refs = prop_case(B, H, W)
    pure, dv = refs['pure'], DIST_VAR[:B]
    cfg = _stages(radii, fill_inflate=1.25 if radii[1] == 2 else 1.0)
    seen = 0
    for meas in (dict(), dict(depth_next=sc['depth_next'], var_next=sc['var_next'], gate=3.0), dict(depth_next=sc['depth_next'], var_next=sc['var_next'], gate=0.0)):
        want = regularize_reference(pure, dist_var=dv, **meas, **cfg)
        out, again = _call(pure, dist_var=dv, **meas, **cfg), _call(pure, dist_var=dv, **meas, **cfg)
        for x, y in zip(out, again):
            assert _same_bits(x, y)
        _equal(_np(out), want)
        for b in range(B if B > 1 else 0):
            single = _call(pure, links=[b], dist_var=dv, **meas, **cfg)
            for k in out._fields:
                assert _same_bits(getattr(single, k)[0], getattr(out, k)[b]), (b, k)
        seen |= int(np.bitwise_or.reduce(np.stack([r['flags'] for r in want]).ravel()))
    if radii == (0, 0, 0):
        alone = _np(_call(pure, dist_var=dv, **cfg))
        for b, p in enumerate(pure):
            _equal({k: v[b:b + 1] for k, v in alone.items()}, [p])
    # what the scene shows at these radii (a condition on the restatement): every stage that is on did something
    assert bool(seen & FLAG_REMOVED) == (radii[0] > 0) and bool(seen & FLAG_FILLED) == (radii[1] > 0) and (seen & 7) == 7
    if radii[2] > 0:
        flat = regularize_reference(pure, dist_var=dv, **dict(cfg, smooth_radius=0))
        assert sum(int((a['inv_depth'] != c['inv_depth']).sum()) for a, c in zip(regularize_reference(pure, dist_var=dv, **cfg), flat)) > 10 * B


def test_ragged_last_row_of_tiles(cuda):
    """136 and 24 are multiples of the tile's 8 rows: the 24 x 40 maps cropped to 21 x 37 give three rows of tiles of which the last holds
    five image rows, and a last column five pixels wide.  Radii 2, with the measurement at gate 3: exact as above."""
    sc, refs = prop_case(3, 24, 40)
    crop = lambda a: np.ascontiguousarray(a[..., :21, :37])
    pure = [dict(p, **{k: crop(p[k]) for k in ('inv_depth', 'var_inv_depth', 'source')}) for p in refs['pure']]
    kw = dict(dist_var=DIST_VAR, depth_next=crop(sc['depth_next']), var_next=crop(sc['var_next']), gate=3.0, **_stages((2, 2, 2)))
    want = regularize_reference(pure, **kw)
    _equal(_np(_call(pure, **kw)), want)
    assert all(r['filled'][20].any() and r['filled'][:, 36].any() for r in want)          # the ragged edges are not idle


# ------------------------------------------------------------------------------------------------ 2. status words
def test_status_marks_only_its_own_link(cuda):
    """An incoming FEW, and a device-side dist_var of -1 and of NaN (BADPRIOR), on the middle link: it returns the measurement alone at
    every pixel; the healthy links equal a batch without it bit for bit."""
    sc, refs = prop_case(3, 24, 40)
    pure = refs['pure']
    meas = dict(depth_next=sc['depth_next'], var_next=sc['var_next'], gate=3.0)
    keep = [0, 2]
    healthy = _call(pure, links=keep, dist_var=DIST_VAR, **meas)
    assert healthy.status.tolist() == [OK, OK] and (healthy.flags & FLAG_FILLED).any()
    for name, kw, want in (('few', dict(status=np.array([OK, FEW, OK], np.int32), dist_var=DIST_VAR), FEW),
                           ('negative', dict(dist_var=np.array([DIST_VAR[0], -1.0, DIST_VAR[2]])), BADPRIOR),
                           ('nan', dict(dist_var=np.array([DIST_VAR[0], np.nan, DIST_VAR[2]])), BADPRIOR)):
        out = _call(pure, **kw, **meas)
        assert out.status.tolist() == [OK, want, OK], name
        for k in ('inv_depth', 'var_inv_depth', 'depth', 'source', 'flags'):
            assert _same_bits(getattr(out, k)[keep], getattr(healthy, k)), (name, k)
        assert (out.source[1] == -1).all() and ((out.flags[1] | FLAG_MEAS) == FLAG_MEAS).all(), name
        assert _same_bits(out.depth[1], _dev(sc['depth_next'][1])), name
        present = out.flags[1] == FLAG_MEAS
        assert present.sum().item() == 24 * 40 - 3 and torch.isnan(out.var_inv_depth[1][~present]).all()
        assert torch.equal(out.var_inv_depth[1][present], _dev(sc['var_next'][1]).double()[present]), name
        _equal(_np(out), regularize_reference(pure, status=kw.get('status'), dist_var=kw['dist_var'], **meas, **DEFAULTS))


# ------------------------------------------------------------------------------------------------ 3. the planted leak scene
def test_leak_scene_equals_the_restatement(cuda):
    """The planted scene of the CPU file on the device: the same maps as the restatement's, bit for bit, hence the same counts -- 42 pixels
    removed, all of them leaks, 303 of the 315 interior targets at the patch's inverse depth."""
    sc = leak_scene()
    want = regularize_reference([sc['pure']], **DEFAULTS)
    got = _np(_call([sc['pure']], **DEFAULTS))
    _equal(got, want)
    c = leak_counts(sc, {k: v[0] for k, v in got.items()})
    n_leak, n_in = int(sc['leak'].sum()), int(sc['interior'].sum())
    print('removed %d (%d leaks of %d), %d of %d interior targets at the patch' % (c['removed'], c['removed_leaks'], n_leak, c['at_fg'], n_in))
    assert c == leak_counts(sc, want[0]) and c['removed'] == c['removed_leaks'] and 3 * c['removed_leaks'] >= 2 * n_leak and c['at_fg'] >= 0.9 * n_in


# ------------------------------------------------------------------------------------------------ 4. through DenseReprojectionLoss
def _device_filter(seq, K, stages):
    """The recursive filter of test_depth_propagate_gpu's test 5 with propagate(regularize=...): stages None, or the record's fields.
    Returns (the last prior, every status seen)."""
    H, W = seq['stereo'][0].shape
    fx, fy, cx, cy = seq['intr']
    ident = pp.SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=torch.float64, device='cuda'))
    depth, sigma = _dev(seq['stereo'][0])[None], torch.full((1, H, W), SIGMA_STEREO, dtype=torch.float64, device='cuda')
    status = []
    for k in range(K):
        loss = DenseReprojectionLoss(depth, _dev(seq['flow'][k])[None], fx, fy, cx, cy, None, ident, device='cuda')
        joint = loss.refine_joint(pp.SE3(_dev(seq['start'][k])[None]), sigma, sigma_px=SIGMA_PX, iters=20)
        unc = loss.depth_uncertainty(joint, sigma, sigma_px=SIGMA_PX)
        cfg = None if stages is None else DepthRegularizer(dist_sigma=float(np.sqrt((seq['grad'][k + 1] ** 2).sum())), **stages)
        prior = loss.propagate(joint, unc, depth_next=_dev(seq['stereo'][k + 1])[None], sigma_inv_depth_next=SIGMA_STEREO,
                               process_sigma=float(np.sqrt(seq['process_var'][k + 1])), gate=3.0, regularize=cfg)
        status += joint.status.tolist() + unc.status.tolist() + prior.status.tolist()
        assert _same_bits(prior.sigma_inv_depth, torch.sqrt(prior.var_inv_depth))
        depth, sigma = prior.depth, prior.sigma_inv_depth
    return {k: getattr(prior, k)[0].cpu().numpy() for k in ('flags', 'inv_depth', 'var_inv_depth')}, status


def test_regularised_filter_through_the_loss(cuda):
    """plane_sequence 48 x 64, three links, refine_joint -> depth_uncertainty -> propagate(regularize=DepthRegularizer(dist_sigma = the
    gradient of the target frame's inverse depth)) -> the next link.  Every status is OK; the last frame's share, RMS and chi^2/n agree
    with the CPU restatement's (filter_reference_reg) within the refinement bound of test_depth_propagate_gpu's test 5, 10 x the
    restatement's own last LM step; against a device run with regularize=None the stages cover more, filling lowers the RMS, smoothing
    lowers it again, chi^2/n stays at or below 1 + 4 sqrt(2/n), and no more pixels are left without a prior."""
    H, W, K = 48, 64, 3
    seq = filter_reference(H, W, K)[0]
    base, status = _device_filter(seq, K, None)
    assert status == [OK] * (3 * K)
    base = prop.filter_stats(base, seq, K)
    got = {}
    for mode in ('fill', 'all'):
        _, _, runs, want = filter_reference_reg(H, W, mode, K)
        prior, status = _device_filter(seq, K, reg.MODES[mode])
        assert status == [OK] * (3 * K), mode
        st = got[mode] = reg.reg_filter_stats(prior, seq, K)
        step = max(r['last_step'] for r in runs)
        print('%-4s share %.4f (restatement %.4f)  rho RMS %.4e (%.4e)  chi^2/n %.4f (%.4f)  bound %.2e  without a prior %d; regularize=None: share %.4f RMS %.4e' % (
            mode, st['share'], want['share'], st['rms'], want['rms'], st['chi2'], want['chi2'], 10 * step, st['none'], base['share'], base['rms']))
        for k in ('share', 'rms', 'chi2'):
            assert abs(st[k] - want[k]) <= 10 * step, (mode, k)
        assert st['share'] > base['share'] and st['none'] <= base['none']
        assert st['chi2'] <= 1 + 4 * math.sqrt(2.0 / st['n'])
    assert got['fill']['rms'] < base['rms']
    assert got['all']['rms'] < got['fill']['rms']
