"""The gradient of depth propagation on the MI355X (csrc/depth_prop.hip: depth_prop_vjp_kernel, depth_prop_pose_kernel; DESIGN.md
section 3.31) against the float64 closed forms of tests/dense_ba_prop_grad_f64.py, and its wiring into
DenseReprojectionLoss.propagate(differentiable=True).

Scenes, state, variances and measurement are those of tests/test_depth_propagate_gpu.py (prop_scene: the mount, per-link intrinsics,
the user mask, every 17th depth at 0.05, three unusable variances, three absent measurements) at (1,7,9), (3,24,40) and (3,136,168),
the smallest shape at which the grid-stride loop takes a second pass (22 848 pixels against 64 x 256 threads).  The op is given the
device forward's own source and flags, which section 3.28's tests hold equal to the restatement's.

Tolerances.  A float64 output lies within 2^-52 K_GRAD of the sum of the magnitudes of its terms, a float32 output within that plus
one float32 rounding of the value, grad_motion within 2^-52 K_MOTION of the pose chain's magnitudes applied to the sums of the
magnitudes of the pixel terms; K_GRAD = K_FUSE + K_VAR + 7 K_RHO + 128 and K_MOTION = K_GRAD + 256 are counted in the helper's
docstring.  An element without terms is an exact zero."""
import numpy as np
import pytest
import torch

from islam_amd import ops
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseBADepthUncertainty, DenseBAJoint, DenseReprojectionLoss
from tests import dense_ba_prop_grad_f64 as pg
from tests.dense_ba_prop_f64 import FLAG_GATED, FLAG_MEAS, FLAG_PROP, SHAPES, SIGMA_PX, SIGMA_STEREO, plane_sequence, prop_scene
from tests.dense_reproj_f64 import BADPRIOR, FEW, MOUNT, OK, U, _dev
from tests.test_depth_propagate_gpu import _same_bits

pytestmark = pytest.mark.gpu
FIELDS = ('grad_inv_depth', 'grad_var_inv_depth', 'grad_motion', 'grad_depth_next', 'grad_var_next')


def _cotangents(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), 1e3 * rng.standard_normal(shape)


def _forward(sc, links=None, status=None, process_var=0.0):
    pick = (lambda a: a) if links is None else (lambda a: a[links])
    kw = dict(mask=pick(_dev(sc['mask'])), rgb2imu=_dev(MOUNT), depth_next=pick(_dev(sc['depth_next'])), var_next=pick(_dev(sc['var_next'])), gate=3.0,
              process_var=process_var if np.isscalar(process_var) else pick(_dev(process_var)))
    if status is not None:
        kw['status'] = pick(_dev(status))
    return ops.dense_ba_depth_propagate(pick(_dev(sc['rho'])), pick(_dev(sc['var'])), pick(_dev(sc['motion'])), pick(_dev(sc['intr'])), **kw)


def _vjp(sc, fwd, gr, gs, links=None, process_var=0.0, meas=True):
    pick = (lambda a: a) if links is None else (lambda a: a[links])
    kw = dict(depth_next=pick(_dev(sc['depth_next'])), var_next=pick(_dev(sc['var_next']))) if meas else {}
    return ops.dense_ba_depth_propagate_vjp(pick(_dev(sc['rho'])), pick(_dev(sc['var'])), pick(_dev(sc['motion'])), pick(_dev(sc['intr'])), fwd.source, fwd.flags,
                                            fwd.status, grad_inv_depth=None if gr is None else pick(_dev(gr)),
                                            grad_var_inv_depth=None if gs is None else pick(_dev(gs)), rgb2imu=_dev(MOUNT),
                                            process_var=process_var if np.isscalar(process_var) else pick(_dev(process_var)), **kw)


def _np(out):
    return {k: getattr(out, k).cpu().numpy() for k in out._fields}


def _share(got, want, scale, k, extra=0.0):
    """The largest |got - want| / (2^-52 k scale + extra |want|) over the elements with terms; the others must be exact zeros."""
    d = np.abs(got.astype(np.float64) - want)
    none = scale == 0
    assert (got[none] == 0).all()
    bound = U * k * scale + extra * np.abs(want)
    return float((d[~none] / bound[~none]).max()) if (~none).any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. the op against the closed forms
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_op_matches_closed_forms(cuda, B, H, W):
    """ops.dense_ba_depth_propagate_vjp on the device forward's own source and flags against propagate_vjp_reference on the same.
    Measured shares of the bounds (float64 pixel outputs / float32 measurement outputs / grad_motion): see DESIGN.md section 3.31."""
    sc = prop_scene(B, H, W)
    fwd = _forward(sc)
    f = _np(fwd)
    assert f['status'].tolist() == [OK] * B and (np.bincount(f['flags'].ravel(), minlength=8)[[0, 1, 2, 3, 7]] > 0).all()
    gr, gs = _cotangents((B, H, W), 300 + H)
    got = _np(_vjp(sc, fwd, gr, gs))
    refs = pg.propagate_vjp_reference(sc['rho'], sc['var'], sc['motion'], MOUNT, sc['intr'], 0.0, sc['depth_next'], sc['var_next'], f['source'], f['flags'],
                                      f['status'], gr, gs)
    worst = dict.fromkeys(FIELDS, 0.0)
    for b, r in enumerate(refs):
        for name in FIELDS:
            assert np.isfinite(got[name][b]).all(), (b, name)
            k, extra = (pg.K_MOTION, 0.0) if name == 'grad_motion' else (pg.K_GRAD, pg.U32 if name.endswith('_next') else 0.0)
            worst[name] = max(worst[name], _share(got[name][b], r[name], r['scale'][name], k, extra))
        won = np.zeros(H * W, bool)
        won[f['source'][b][f['source'][b] >= 0]] = True
        assert (got['grad_inv_depth'][b].ravel()[~won] == 0).all() and (got['grad_var_inv_depth'][b].ravel()[~won] == 0).all()
        assert (got['grad_inv_depth'][b] != 0).sum() >= 0.3 * won.sum() and np.abs(got['grad_motion'][b]).min() > 0
    print('%dx%dx%d: worst share of the bound: %s' % (B, H, W, {k: '%.4f' % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst
    # without a measurement: the propagated-only row, no measurement gradients
    pure = ops.dense_ba_depth_propagate(_dev(sc['rho']), _dev(sc['var']), _dev(sc['motion']), _dev(sc['intr']), mask=_dev(sc['mask']), rgb2imu=_dev(MOUNT))
    g = _vjp(sc, pure, gr, gs, meas=False)
    assert g.grad_depth_next is None and g.grad_var_next is None
    p = _np(pure)
    refs = pg.propagate_vjp_reference(sc['rho'], sc['var'], sc['motion'], MOUNT, sc['intr'], 0.0, None, None, p['source'], p['flags'], p['status'], gr, gs)
    for b, r in enumerate(refs):
        for name in FIELDS[:3]:
            k = pg.K_MOTION if name == 'grad_motion' else pg.K_GRAD
            assert _share(getattr(g, name)[b].cpu().numpy(), r[name], r['scale'][name], k) <= 1.0, (b, name)


# ------------------------------------------------------------------------------------------------ 2. repeatability and independence
def test_repeat_gives_the_same_bits_and_cotangents_are_independent(cuda):
    sc = prop_scene(3, 136, 168)
    fwd = _forward(sc)
    gr, gs = _cotangents((3, 136, 168), 401)
    one, two = _vjp(sc, fwd, gr, gs), _vjp(sc, fwd, gr, gs)
    for x, y in zip(one, two):
        assert _same_bits(x, y)
    zero = np.zeros_like(gr)
    for given, padded in (((gr, None), (gr, zero)), ((None, gs), (zero, gs)), ((None, None), (zero, zero))):
        a, b = _vjp(sc, fwd, *given), _vjp(sc, fwd, *padded)
        for name, x, y in zip(FIELDS, a, b):
            assert _same_bits(x, y), (given[0] is None, given[1] is None, name)
    nothing = _vjp(sc, fwd, None, None)
    assert all(not x.any() for x in nothing)
    assert one.grad_depth_next.dtype == torch.float32 and one.grad_var_next.dtype == torch.float32 and one.grad_motion.shape == (3, 7)


# ------------------------------------------------------------------------------------------------ 3. status on the middle link
def test_status_zeroes_only_its_own_link(cuda):
    """An incoming FEW, then a device-side process_var of -1 (BADPRIOR), on the middle link: its three state gradients are exact zeros,
    its measurement gradients those of the measured-only row (-rho_m^2 gr and gs rounded once to float32, exact zeros where the
    measurement is absent), and the healthy links equal a batch without it bit for bit."""
    sc = prop_scene(3, 24, 40)
    gr, gs = _cotangents((3, 24, 40), 402)
    keep = [0, 2]
    healthy = _vjp(sc, _forward(sc, links=keep), gr, gs, links=keep)
    for name, kw, want in (('few', dict(status=np.array([OK, FEW, OK], np.int32)), FEW), ('badprior', dict(process_var=np.array([0.0, -1.0, 0.0])), BADPRIOR)):
        fwd = _forward(sc, **kw)
        assert fwd.status.tolist() == [OK, want, OK], name
        out = _vjp(sc, fwd, gr, gs, process_var=kw.get('process_var', 0.0))
        for field, x, y in zip(FIELDS, out, healthy):
            assert _same_bits(x[keep], y), (name, field)
        assert not out.grad_inv_depth[1].any() and not out.grad_var_inv_depth[1].any() and not out.grad_motion[1].any(), name
        present = (fwd.flags[1] == FLAG_MEAS).cpu().numpy()
        assert present.sum() == 24 * 40 - 3 and ((fwd.flags[1] | FLAG_MEAS) == FLAG_MEAS).all()
        rm = 1.0 / sc['depth_next'][1].astype(np.float64)[present]
        gdn, gvn = out.grad_depth_next[1].cpu().numpy(), out.grad_var_next[1].cpu().numpy()
        assert np.array_equal(gdn[present], (-(rm * rm) * gr[1][present]).astype(np.float32)) and (gdn[~present] == 0).all(), name
        assert np.array_equal(gvn[present], gs[1][present].astype(np.float32)) and (gvn[~present] == 0).all(), name


# ------------------------------------------------------------------------------------------------ 4. NaN cotangents
@pytest.mark.parametrize('B,H,W', SHAPES[:2])
def test_nan_cotangents_where_nothing_is_known(cuda, B, H, W):
    """Cotangents that are NaN exactly where flags == 0 (what torch.sqrt's backward hands over there): every output is finite and
    equals the one with zeros there, bit for bit."""
    sc = prop_scene(B, H, W)
    fwd = _forward(sc)
    nothing = (fwd.flags == 0).cpu().numpy()
    assert nothing.any()
    gr, gs = _cotangents((B, H, W), 403)
    bad = _vjp(sc, fwd, np.where(nothing, np.nan, gr), np.where(nothing, np.nan, gs))
    good = _vjp(sc, fwd, np.where(nothing, 0.0, gr), np.where(nothing, 0.0, gs))
    for name, x, y in zip(FIELDS, bad, good):
        assert torch.isfinite(x).all() and _same_bits(x, y), name


# ------------------------------------------------------------------------------------------------ 5. wiring
def _plane_chain(seq, differentiable):
    """Two links of plane_sequence through refine_joint -> depth_uncertainty -> propagate -> refine_joint."""
    fx, fy, cx, cy = seq['intr']
    H, W = seq['stereo'].shape[1:]
    ident = pp.SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=torch.float64, device='cuda'))
    kw = dict(differentiable=True, hessian='exact') if differentiable else {}
    depth0, flow0 = _dev(seq['stereo'][0])[None].requires_grad_(differentiable), _dev(seq['flow'][0])[None].requires_grad_(differentiable)
    loss0 = DenseReprojectionLoss(depth0, flow0, fx, fy, cx, cy, None, ident, device='cuda')
    sigma0 = torch.full((1, H, W), SIGMA_STEREO, dtype=torch.float64, device='cuda')
    j0 = loss0.refine_joint(pp.SE3(_dev(seq['start'][0])[None]), sigma0, sigma_px=SIGMA_PX, iters=20, **kw)
    unc = loss0.depth_uncertainty(j0, sigma0, sigma_px=SIGMA_PX)
    meas = dict(depth_next=_dev(seq['stereo'][1])[None], sigma_inv_depth_next=SIGMA_STEREO, process_sigma=float(np.sqrt(seq['process_var'][1])), gate=3.0)
    prior = loss0.propagate(j0, unc, differentiable=differentiable, **meas)
    loss1 = DenseReprojectionLoss(prior.depth, _dev(seq['flow'][1])[None], fx, fy, cx, cy, None, ident, device='cuda')
    j1 = loss1.refine_joint(pp.SE3(_dev(seq['start'][1])[None]), prior.sigma_inv_depth.detach(), sigma_px=SIGMA_PX, iters=20, **kw)
    return dict(depth0=depth0, flow0=flow0, j0=j0, unc=unc, prior=prior, j1=j1, loss0=loss0, meas=meas)


def test_one_backward_runs_through_two_links(cuda):
    """plane_sequence(24, 40, K=2, seed=0): link 0 refine_joint(differentiable=True, hessian='exact') -> depth_uncertainty ->
    propagate(differentiable=True) -> link 1 built from prior.depth -> refine_joint(sigma = prior.sigma_inv_depth.detach(),
    differentiable=True, hessian='exact'), L = c . motion_1 + sum d rho_1.  One L.backward() to link 0's stored depth and flow equals,
    bit for bit, the chain done by hand on the same graph: autograd.grad of link 1 to prior.depth, its chain to rho_f in torch,
    ops.dense_ba_depth_propagate_vjp, autograd.grad of link 0 with those cotangents.  The stored depth's gradient is non-zero on at least
    half of the pixels of link 0 that won a target flagged propagated, and the forward outputs equal those of the chain run with
    differentiable=False, bit for bit."""
    seq = plane_sequence(24, 40, K=2, seed=0)
    ch = _plane_chain(seq, True)
    j0, j1, prior, unc, depth0, flow0 = ch['j0'], ch['j1'], ch['prior'], ch['unc'], ch['depth0'], ch['flow0']
    assert j0.status.tolist() == [OK] and unc.status.tolist() == [OK] and prior.status.tolist() == [OK] and j1.status.tolist() == [OK]
    assert prior.depth.grad_fn is not None and prior.inv_depth.grad_fn is not None and prior.var_inv_depth.grad_fn is not None
    assert prior.sigma_inv_depth.grad_fn is not None and not prior.source.requires_grad and not prior.flags.requires_grad
    rng = np.random.default_rng(17)
    c, d = _dev(rng.standard_normal((1, 7))), _dev(rng.standard_normal((1, 24, 40)))
    L = (j1.motion * c).sum() + (j1.inv_depth * d).sum()
    # by hand
    g_depth, = torch.autograd.grad(L, prior.depth, retain_graph=True)
    g_rho_f, = torch.autograd.grad(prior.depth, prior.inv_depth, g_depth, retain_graph=True)
    m = ch['meas']
    var_next = ch['loss0']._variance_next(SIGMA_STEREO, 'propagate')          # what propagate hands the kernel
    g = ops.dense_ba_depth_propagate_vjp(j0.inv_depth, unc.var_inv_depth, j0.motion, torch.tensor(ch['loss0'].K4, dtype=torch.float64), prior.source,
                                         prior.flags, prior.status, grad_inv_depth=g_rho_f, rgb2imu=pp._plain(ch['loss0'].rgb2imu_pose),
                                         process_var=m['process_sigma'] * m['process_sigma'], depth_next=m['depth_next'], var_next=var_next)
    hand_depth, hand_flow = torch.autograd.grad([j0.inv_depth, j0.motion], [depth0, flow0], [g.grad_inv_depth, g.grad_motion], retain_graph=True)
    L.backward()
    assert depth0.grad is not None and flow0.grad is not None
    assert _same_bits(depth0.grad, hand_depth) and _same_bits(flow0.grad, hand_flow)
    assert torch.isfinite(depth0.grad).all() and torch.isfinite(flow0.grad).all() and flow0.grad.abs().max() > 0
    winners = prior.source[(prior.flags & FLAG_PROP) != 0].long()
    share = (depth0.grad.reshape(-1)[winners] != 0).double().mean().item()
    print('propagated targets: %d of %d; the stored depth of link 0 has a gradient at %.1f %% of their sources; |grad_motion| %.3e' % (
        winners.numel(), 24 * 40, 100 * share, g.grad_motion.abs().max().item()))
    assert winners.numel() >= 0.5 * 24 * 40 and share >= 0.5 and g.grad_motion.abs().min() > 0
    # the forward pass is the default one's
    plain = _plane_chain(seq, False)
    assert plain['prior'].depth.grad_fn is None and plain['j1'].motion.grad_fn is None
    for name in ('depth', 'sigma_inv_depth', 'inv_depth', 'var_inv_depth', 'source', 'flags', 'status'):
        assert _same_bits(getattr(prior, name).detach(), getattr(plain['prior'], name)), name
    for name in ('motion', 'inv_depth', 'depth', 'status'):
        assert _same_bits(getattr(j1, name).detach(), getattr(plain['j1'], name)), name


# ------------------------------------------------------------------------------------------------ 6. forward bits
def test_differentiable_forward_has_the_default_bits(cuda):
    """propagate(differentiable=True) returns depth, sigma_inv_depth, inv_depth, var_inv_depth, source, flags and status bit-equal to
    differentiable=False on the (3,24,40) case with a measurement (absent, NaN and negative entries included), and its depth and
    sigma_inv_depth carry a graph over the state, the pose and depth_next."""
    sc = prop_scene(3, 24, 40)
    fx, fy, cx, cy = sc['intr'][0]
    loss = DenseReprojectionLoss(_dev(sc['depth']), _dev(sc['flow']), fx, fy, cx, cy, _dev(sc['mask']), pp.SE3(_dev(MOUNT)), device='cuda')
    ok = torch.zeros(3, dtype=torch.int32, device='cuda')
    leaf = lambda a: _dev(a).requires_grad_()
    rho, var, motion, dn = leaf(sc['rho']), leaf(sc['var']), leaf(sc['motion']), leaf(sc['depth_next'])
    joint = DenseBAJoint(*([None] * 14))._replace(motion=motion, inv_depth=rho, status=ok)
    unc = DenseBADepthUncertainty(var, None, None, ok)
    kw = dict(depth_next=dn, sigma_inv_depth_next=_dev(np.sqrt(sc['var_next'].astype(np.float64))), process_sigma=1e-3, gate=3.0)
    a, b = loss.propagate(joint, unc, differentiable=True, **kw), loss.propagate(joint, unc, **kw)
    assert (np.bincount(b.flags.cpu().numpy().ravel(), minlength=8)[[0, 1, 2, 3, 7]] > 0).all()
    for name in a._fields:
        assert _same_bits(getattr(a, name).detach(), getattr(b, name)), name
        assert not getattr(b, name).requires_grad
    assert a.depth.dtype == torch.float32 and a.depth.grad_fn is not None and a.sigma_inv_depth.grad_fn is not None
    known = a.flags != 0
    (a.depth[known].double().sum() + a.sigma_inv_depth[known].sum()).backward()
    for t in (rho, var, motion, dn):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0
    assert dn.grad.dtype == torch.float32
    # the NaN that torch.sqrt's backward forms where nothing is known never reaches a gradient
    rho.grad = var.grad = motion.grad = dn.grad = None
    a = loss.propagate(joint, unc, differentiable=True, **kw)
    (torch.nan_to_num(a.sigma_inv_depth).sum() + a.depth.double().sum()).backward()
    for t in (rho, var, motion, dn):
        assert torch.isfinite(t.grad).all()
