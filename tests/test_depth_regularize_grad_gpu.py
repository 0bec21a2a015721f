"""The gradient of the depth regularisation on the MI355X (csrc/depth_prop.hip: depth_reg_front_kernel, depth_reg_smooth_adj_kernel,
depth_reg_fill_adj_kernel) against the float64 closed forms of tests/dense_ba_reg_grad_f64.py, and its wiring
into DenseReprojectionLoss.propagate(regularize_grad='piecewise').

The device is fed prop_case(...)['pure'] as tests/test_depth_regularize_gpu.py feeds it: (1,7,9) below one tile; (3,24,40), two tile
columns of 32 and 8 and three tile rows, so every gather crosses a tile border; the 24 x 40 maps cropped to 21 x 37, whose last tile
row holds five rows; (3,136,168), 6 x 17 tiles.  The op is given the device forward's own flags, which section 3.29's tests hold
equal to the restatement's.

Tolerances.  A float64 output lies within 2^-52 K_DEVICE of its scale (the sum of the magnitudes of its terms, differences split), a
float32 output within that plus one float32 rounding of the value; K_DEVICE = 108 is counted in the helper's docstring.  An element
without terms is an exact zero.  Measured shares of the bounds: DESIGN.md section 3.33."""
import numpy as np
import pytest
import torch

from islam_amd import ops
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseReprojectionLoss, DepthRegularizer
from tests import dense_ba_reg_grad_f64 as rg
from tests.dense_ba_prop_f64 import FLAG_MEAS, FLAG_PROP, SHAPES, SIGMA_PX, SIGMA_STEREO, plane_sequence, prop_case
from tests.dense_ba_reg_f64 import DEFAULTS, FLAG_FILLED, regularize_reference
from tests.dense_reproj_f64 import FEW, OK, _dev
from tests.test_depth_propagate_gpu import _same_bits

pytestmark = pytest.mark.gpu

RADII = [(1, 1, 1), (2, 2, 2), (0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0)]
DIST_VAR = np.array([2.0 ** -14, 0.0, 3e-6])          # per link: the smoothing weights differ from link to link
FIELDS = ('grad_inv_depth', 'grad_var_inv_depth', 'grad_depth_next', 'grad_var_next')


def _stages(radii, **kw):
    return dict(DEFAULTS, occl_radius=radii[0], fill_radius=radii[1], smooth_radius=radii[2], **kw)


def _cotangents(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), 1e3 * rng.standard_normal(shape)


def _args(pure, links, kw):
    stack = lambda k: _dev(np.stack([pure[b][k] for b in links]))
    kw = dict(kw)
    for k in ('depth_next', 'var_next', 'status', 'dist_var'):
        if k in kw and kw[k] is not None and not np.isscalar(kw[k]):
            kw[k] = _dev(np.asarray(kw[k])[links])
    kw.setdefault('status', _dev(np.array([pure[b]['status'] for b in links], np.int32)))
    return stack, kw


def _forward(pure, links=None, **kw):
    links = list(range(len(pure))) if links is None else links
    stack, kw = _args(pure, links, kw)
    return ops.dense_ba_depth_regularize(stack('inv_depth'), stack('var_inv_depth'), source=stack('source'), **kw)


def _vjp(pure, fwd, gr, gs, links=None, **kw):
    """ops.dense_ba_depth_regularize_vjp on the pure propagation of a scene (or on some links) with the forward's flags and status."""
    links = list(range(len(pure))) if links is None else links
    stack, kw = _args(pure, links, kw)
    kw['status'] = fwd.status
    pick = lambda g: None if g is None else _dev(np.asarray(g)[links])
    return ops.dense_ba_depth_regularize_vjp(stack('inv_depth'), stack('var_inv_depth'), fwd.flags, grad_inv_depth=pick(gr),
                                             grad_var_inv_depth=pick(gs), **kw)


def _same(a, b):
    return all((x is None and y is None) or _same_bits(x, y) for x, y in zip(a, b))


def _against_closed_forms(tag, pure, refs, fwd, out, gr, gs, dist_var, meas, cfg):
    """Every output of every link within its bound; exact zeros off valid1.  Returns the largest share per field."""
    worst = dict.fromkeys(FIELDS, 0.0)
    flags = fwd.flags.cpu().numpy()
    got = {k: None if getattr(out, k) is None else getattr(out, k).cpu().numpy() for k in FIELDS}
    for b, ref in enumerate(refs):
        assert np.array_equal(flags[b], ref['flags']), (tag, b)
        cf = rg.regularize_vjp_reference_link(ref, flags[b], dist_var[b], None if 'depth_next' not in meas else meas['depth_next'][b],
                                              None if 'var_next' not in meas else meas['var_next'][b], gr[b], gs[b], **cfg)
        off = ~cf['valid1']
        assert (got['grad_inv_depth'][b][off] == 0).all() and (got['grad_var_inv_depth'][b][off] == 0).all(), (tag, b)
        for k in FIELDS:
            if got[k] is None:
                assert cf[k] is None
                continue
            f32 = got[k].dtype == np.float32
            extra = (rg.U24 * np.abs(cf[k]) + 2.0 ** -149) if f32 else None
            s = rg.share('%s link %d %s' % (tag, b, k), got[k][b], cf[k], cf['scale' + k[4:]], rg.K_DEVICE, extra)
            worst[k] = max(worst[k], s)
    return worst


def _run_case(tag, sc, pure, radii, crop=None):
    B = len(pure)
    dv = DIST_VAR[:B]
    cfg = _stages(radii, fill_inflate=1.25 if radii[1] == 2 else 1.0)
    c = (lambda a: a) if crop is None else crop
    dn, vn = c(sc['depth_next']), c(sc['var_next'])
    H, W = pure[0]['inv_depth'].shape
    gr, gs = _cotangents((B, H, W), 500 + H)
    worst = dict.fromkeys(FIELDS, 0.0)
    for name, meas in (('none', dict()), ('gate3', dict(depth_next=dn, var_next=vn, gate=3.0)), ('gate0', dict(depth_next=dn, var_next=vn, gate=0.0))):
        refs = regularize_reference(pure, dist_var=dv, **meas, **cfg)
        fwd = _forward(pure, dist_var=dv, **meas, **cfg)
        out, again = _vjp(pure, fwd, gr, gs, dist_var=dv, **meas, **cfg), _vjp(pure, fwd, gr, gs, dist_var=dv, **meas, **cfg)
        assert _same(out, again), (tag, name)                                       # a repeat gives the same bits
        w = _against_closed_forms('%s %s %s' % (tag, radii, name), pure, refs, fwd, out, gr, gs, dv, meas, cfg)
        worst = {k: max(worst[k], w[k]) for k in FIELDS}
        # a NULL cotangent equals zeros in its place
        assert _same(_vjp(pure, fwd, gr, None, dist_var=dv, **meas, **cfg), _vjp(pure, fwd, gr, np.zeros_like(gs), dist_var=dv, **meas, **cfg)), (tag, name)
        assert _same(_vjp(pure, fwd, None, gs, dist_var=dv, **meas, **cfg), _vjp(pure, fwd, np.zeros_like(gr), gs, dist_var=dv, **meas, **cfg)), (tag, name)
        for b in range(B if B > 1 else 0):                                          # every link equals its single-link run
            f1 = _forward(pure, links=[b], dist_var=dv, **meas, **cfg)
            single = _vjp(pure, f1, gr, gs, links=[b], dist_var=dv, **meas, **cfg)
            for k in FIELDS:
                x = getattr(single, k)
                assert (x is None and getattr(out, k) is None) or _same_bits(x[0], getattr(out, k)[b]), (tag, name, b, k)
        if radii == (0, 0, 0) and not meas:                                         # nothing to differentiate: the cotangents come back
            present = (fwd.flags & FLAG_PROP) != 0
            assert _same_bits(out.grad_inv_depth[present], _dev(gr)[present]) and _same_bits(out.grad_var_inv_depth[present], _dev(gs)[present])
    print('%s radii %s: largest shares %s' % (tag, radii, {k: round(v, 4) for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 1, 2. closed forms, determinism
@pytest.mark.parametrize('radii', RADII)
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_op_matches_closed_forms(cuda, B, H, W, radii):
    """ops.dense_ba_depth_regularize_vjp on the device forward's own flags against regularize_vjp_reference_link: without a measurement,
    with the scene's at gate 3 and at gate 0; a repeat, a NULL cotangent against zeros, every link against its single-link run."""
    sc, refs = prop_case(B, H, W)
    _run_case('%dx%dx%d' % (B, H, W), sc, refs['pure'], radii)


@pytest.mark.parametrize('radii', [(2, 2, 2), (1, 1, 1)])
def test_ragged_last_row_of_tiles(cuda, radii):
    """The 24 x 40 maps cropped to 21 x 37: the last tile row holds five image rows and the last tile column five pixels."""
    sc, refs = prop_case(3, 24, 40)
    crop = lambda a: np.ascontiguousarray(a[..., :21, :37])
    pure = [dict(p, **{k: crop(p[k]) for k in ('inv_depth', 'var_inv_depth', 'source')}) for p in refs['pure']]
    _run_case('3x21x37', sc, pure, radii, crop)


# ------------------------------------------------------------------------------------------------ 3. a marked link
def test_status_marks_only_its_own_link(cuda):
    """An incoming FEW, and a device-side dist_var of -1 and of NaN, on the middle link: zeros on its state gradients, the float32 of
    -rho_m^2 g_rho and of g_s on its measurement where there is one, bit for bit; the healthy links equal a batch without it."""
    sc, refs = prop_case(3, 24, 40)
    pure = refs['pure']
    meas = dict(depth_next=sc['depth_next'], var_next=sc['var_next'], gate=3.0)
    gr, gs = _cotangents((3, 24, 40), 77)
    keep = [0, 2]
    hf = _forward(pure, links=keep, dist_var=DIST_VAR, **meas)
    healthy = _vjp(pure, hf, gr, gs, links=keep, dist_var=DIST_VAR, **meas)
    assert (hf.flags & FLAG_FILLED).any() and healthy.grad_inv_depth.abs().max() > 0
    for name, kw in (('few', dict(status=np.array([OK, FEW, OK], np.int32), dist_var=DIST_VAR)),
                     ('negative', dict(dist_var=np.array([DIST_VAR[0], -1.0, DIST_VAR[2]]))),
                     ('nan', dict(dist_var=np.array([DIST_VAR[0], np.nan, DIST_VAR[2]])))):
        fwd = _forward(pure, **kw, **meas)
        assert fwd.status[1].item() != OK and fwd.status[0].item() == OK
        out = _vjp(pure, fwd, gr, gs, **kw, **meas)
        for k in FIELDS:
            assert _same_bits(getattr(out, k)[keep], getattr(healthy, k)), (name, k)
        assert (out.grad_inv_depth[1] == 0).all() and (out.grad_var_inv_depth[1] == 0).all(), name
        measured = (fwd.flags[1] & FLAG_MEAS) != 0
        assert measured.sum().item() == 24 * 40 - 3
        rm = 1.0 / _dev(sc['depth_next'][1]).double()
        want_dn = torch.where(measured, (-(rm * rm) * _dev(gr[1])).float(), torch.zeros((), device='cuda'))
        want_vn = torch.where(measured, _dev(gs[1]).float(), torch.zeros((), device='cuda'))
        assert _same_bits(out.grad_depth_next[1], want_dn) and _same_bits(out.grad_var_next[1], want_vn), name
    # the status the forward call was given marks the link as well as the one it returned
    fwd = _forward(pure, status=np.array([OK, FEW, OK], np.int32), dist_var=DIST_VAR, **meas)
    stack, kw = _args(pure, [0, 1, 2], dict(dist_var=DIST_VAR, status=np.array([OK, FEW, OK], np.int32), **meas))
    a = ops.dense_ba_depth_regularize_vjp(stack('inv_depth'), stack('var_inv_depth'), fwd.flags, grad_inv_depth=_dev(gr), grad_var_inv_depth=_dev(gs), **kw)
    assert (a.grad_inv_depth[1] == 0).all() and _same_bits(a.grad_inv_depth[keep], healthy.grad_inv_depth)


# ------------------------------------------------------------------------------------------------ 4. NaN cotangents
@pytest.mark.parametrize('B,H,W', SHAPES[:2])
def test_nan_cotangents_where_nothing_is_known(cuda, B, H, W):
    """NaN cotangents where (flags & 3) == 0: all outputs finite and bit-equal to the run with zeros there."""
    sc, refs = prop_case(B, H, W)
    pure = refs['pure']
    for meas in (dict(), dict(depth_next=sc['depth_next'], var_next=sc['var_next'], gate=3.0)):
        kw = dict(dist_var=DIST_VAR[:B], **meas, **DEFAULTS)
        fwd = _forward(pure, **kw)
        nothing = ((fwd.flags & 3) == 0).cpu().numpy()
        assert nothing.any()
        gr, gs = _cotangents((B, H, W), 403)
        bad = _vjp(pure, fwd, np.where(nothing, np.nan, gr), np.where(nothing, np.nan, gs), **kw)
        good = _vjp(pure, fwd, np.where(nothing, 0.0, gr), np.where(nothing, 0.0, gs), **kw)
        for name, x, y in zip(FIELDS, bad, good):
            assert (x is None and y is None) or (torch.isfinite(x).all() and _same_bits(x, y)), name


# ------------------------------------------------------------------------------------------------ 5. the forward is untouched
def test_function_forward_has_the_ops_bits(cuda):
    """ops._DenseBARegularize.apply returns all six fields bit-equal to ops.dense_ba_depth_regularize, with a graph on the two maps only."""
    sc, refs = prop_case(3, 24, 40)
    pure = refs['pure']
    stack, kw = _args(pure, [0, 1, 2], dict(dist_var=DIST_VAR, depth_next=sc['depth_next'], var_next=sc['var_next'], gate=3.0))
    rho, var, dn = stack('inv_depth').requires_grad_(), stack('var_inv_depth').requires_grad_(), kw['depth_next'].clone().requires_grad_()
    stages = _stages((2, 1, 2), fill_inflate=1.5)
    plain = ops.dense_ba_depth_regularize(rho, var, source=stack('source'), **dict(kw, **stages))
    out = ops.DenseBARegularized(*ops._DenseBARegularize.apply(rho, var, stack('source'), kw['status'], kw['dist_var'], dn, kw['var_next'], 3.0, stages))
    for k in out._fields:
        assert _same_bits(getattr(out, k).detach(), getattr(plain, k)), k
    assert out.inv_depth.grad_fn is not None and out.var_inv_depth.grad_fn is not None
    assert not any(getattr(out, k).requires_grad for k in ('depth', 'source', 'flags', 'status'))
    known = (out.flags & 3) != 0
    gr, gs = _cotangents((3, 24, 40), 9)
    (out.inv_depth[known] * _dev(gr)[known]).sum().backward()          # the cotangent of var_inv_depth arrives as None
    g = ops.dense_ba_depth_regularize_vjp(rho, var, out.flags, grad_inv_depth=torch.where(known, _dev(gr), torch.zeros((), dtype=torch.float64, device='cuda')),
                                          **dict(kw, status=out.status, **stages))
    assert _same_bits(rho.grad, g.grad_inv_depth) and _same_bits(var.grad, g.grad_var_inv_depth) and _same_bits(dn.grad, g.grad_depth_next)
    assert dn.grad.dtype == torch.float32 and rho.grad.abs().max() > 0 and var.grad.abs().max() > 0


# ------------------------------------------------------------------------------------------------ 6. wiring
def _plane_chain(seq, differentiable, cfg):
    """Two links of plane_sequence through refine_joint -> depth_uncertainty -> propagate(regularize) -> refine_joint."""
    fx, fy, cx, cy = seq['intr']
    H, W = seq['stereo'].shape[1:]
    ident = pp.SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=torch.float64, device='cuda'))
    kw = dict(differentiable=True, hessian='exact') if differentiable else {}
    depth0, flow0 = _dev(seq['stereo'][0])[None].requires_grad_(differentiable), _dev(seq['flow'][0])[None].requires_grad_(differentiable)
    loss0 = DenseReprojectionLoss(depth0, flow0, fx, fy, cx, cy, None, ident, device='cuda')
    sigma0 = torch.full((1, H, W), SIGMA_STEREO, dtype=torch.float64, device='cuda')
    j0 = loss0.refine_joint(pp.SE3(_dev(seq['start'][0])[None]), sigma0, sigma_px=SIGMA_PX, iters=20, **kw)
    unc = loss0.depth_uncertainty(j0, sigma0, sigma_px=SIGMA_PX, differentiable=differentiable)
    meas = dict(depth_next=_dev(seq['stereo'][1])[None], sigma_inv_depth_next=SIGMA_STEREO, process_sigma=float(np.sqrt(seq['process_var'][1])), gate=3.0)
    pkw = dict(differentiable=True, regularize_grad='piecewise') if differentiable else {}
    prior = loss0.propagate(j0, unc, regularize=cfg, **meas, **pkw)
    loss1 = DenseReprojectionLoss(prior.depth, _dev(seq['flow'][1])[None], fx, fy, cx, cy, None, ident, device='cuda')
    j1 = loss1.refine_joint(pp.SE3(_dev(seq['start'][1])[None]), prior.sigma_inv_depth.detach(), sigma_px=SIGMA_PX, iters=20, **kw)
    return dict(depth0=depth0, flow0=flow0, j0=j0, unc=unc, prior=prior, j1=j1, loss0=loss0, meas=meas)


def test_one_backward_runs_through_the_regularised_filter(cuda):
    """plane_sequence(24, 40, K=2, seed=0): link 0 refine_joint(differentiable=True, hessian='exact') -> depth_uncertainty(
    differentiable=True) -> propagate(differentiable=True, regularize=DepthRegularizer(dist_sigma=...), regularize_grad='piecewise') ->
    link 1 built from prior.depth, L = c . motion_1 + sum d rho_1.  One L.backward() to link 0's stored depth and flow equals, bit for
    bit, the chain done by hand on the same graph through ops.dense_ba_depth_regularize_vjp and ops.dense_ba_depth_propagate_vjp; the
    forward outputs of both links equal the differentiable=False regularised chain bit for bit."""
    seq = plane_sequence(24, 40, K=2, seed=0)
    cfg = DepthRegularizer(dist_sigma=float(np.sqrt((seq['grad'][1] ** 2).sum())))
    ch = _plane_chain(seq, True, cfg)
    j0, j1, prior, unc, depth0, flow0, loss0 = ch['j0'], ch['j1'], ch['prior'], ch['unc'], ch['depth0'], ch['flow0'], ch['loss0']
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
    var_next = loss0._variance_next(SIGMA_STEREO, 'propagate')          # what propagate hands the kernels
    K4 = torch.tensor(loss0.K4, dtype=torch.float64)
    pv = m['process_sigma'] * m['process_sigma']
    pure = ops.dense_ba_depth_propagate(j0.inv_depth, unc.var_inv_depth, j0.motion, K4, mask=loss0.mask, status=unc.status, rgb2imu=loss0.rgb2imu_pose,
                                        process_var=pv)
    stages = cfg._asdict()
    dist_var = stages.pop('dist_sigma') ** 2
    gq = ops.dense_ba_depth_regularize_vjp(pure.inv_depth, pure.var_inv_depth, prior.flags, status=prior.status, grad_inv_depth=g_rho_f, dist_var=dist_var,
                                           depth_next=m['depth_next'], var_next=var_next, gate=3.0, **stages)
    g = ops.dense_ba_depth_propagate_vjp(j0.inv_depth, unc.var_inv_depth, j0.motion, K4, pure.source, pure.flags, pure.status,
                                         grad_inv_depth=gq.grad_inv_depth, grad_var_inv_depth=gq.grad_var_inv_depth,
                                         rgb2imu=pp._plain(loss0.rgb2imu_pose), process_var=pv)
    hand_depth, hand_flow = torch.autograd.grad([j0.inv_depth, j0.motion, unc.var_inv_depth], [depth0, flow0],
                                                [g.grad_inv_depth, g.grad_motion, g.grad_var_inv_depth], retain_graph=True)
    L.backward()
    assert depth0.grad is not None and flow0.grad is not None
    assert torch.isfinite(depth0.grad).all() and torch.isfinite(flow0.grad).all() and flow0.grad.abs().max() > 0
    exact = _same_bits(depth0.grad, hand_depth) and _same_bits(flow0.grad, hand_flow)
    filled = (prior.flags & FLAG_FILLED) != 0
    ref_free = ops.dense_ba_depth_regularize_vjp(pure.inv_depth, pure.var_inv_depth, prior.flags, status=prior.status,
                                                 grad_inv_depth=torch.where(filled, g_rho_f, torch.zeros_like(g_rho_f)), dist_var=dist_var,
                                                 depth_next=m['depth_next'], var_next=var_next, gate=3.0, **dict(stages, smooth_radius=0))
    passing = int(((g_rho_f != 0) & filled).sum().item())
    print('one backward against the chain by hand: %s; filled targets %d, of which %d carry a cotangent; sources reached from filled targets alone %d' % (
        'bit for bit' if exact else 'NOT bit for bit', int(filled.sum().item()), passing, int((ref_free.grad_inv_depth != 0).sum().item())))
    assert exact
    assert int(filled.sum().item()) > 0 and int((ref_free.grad_inv_depth != 0).sum().item()) > 0
    # the forward pass is the default one's
    plain = _plane_chain(seq, False, cfg)
    assert plain['prior'].depth.grad_fn is None and plain['j1'].motion.grad_fn is None
    for name in ('depth', 'sigma_inv_depth', 'inv_depth', 'var_inv_depth', 'source', 'flags', 'status'):
        assert _same_bits(getattr(prior, name).detach(), getattr(plain['prior'], name)), name
    for name in ('motion', 'inv_depth', 'depth', 'status'):
        assert _same_bits(getattr(j1, name).detach(), getattr(plain['j1'], name)), name
