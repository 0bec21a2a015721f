"""The gradient of the posterior depth variance on the MI355X (csrc/dense_ba.hip: depth_var_adj_partial_kernel, depth_var_vjp_kernel,
depth_var_pose_kernel) against the float64 closed forms of tests/dense_ba_var_grad_f64.py, and its wiring into
DenseReprojectionLoss.depth_uncertainty(differentiable=True).

Scenes are those of tests/test_dense_ba_uncertainty_gpu.py (the mount, per-link intrinsics and weights, the user mask, pixels without a
prior, a map with entries 0, NaN and -1) at (1,7,9), (3,24,40) and (3,136,168), the smallest shape at which the 64 x 256 grid-stride
loop takes a second pass.  The op is given the device forward's own sums.

Tolerances.  An output lies within 2^-52 (K + 64 cond(S_cam)) of the sum of the magnitudes of its terms, K = K_GRAD for the pixel
outputs (the float32 grad_flow adds one float32 rounding of the value) and K_MOTION for grad_motion; both are counted in the helper's
docstring.  An element without terms is an exact zero."""
import numpy as np
import pytest
import torch

from islam_amd import ops
from islam_amd import lietensor as pp
from islam_amd.dense_ba import DenseBAJoint, DenseReprojectionLoss
from tests import dense_ba_var_grad_f64 as vg
from tests.dense_ba_prop_f64 import SIGMA_PX, SIGMA_STEREO, plane_sequence
from tests.dense_ba_var_f64 import scam_from_sums
from tests.dense_reproj_f64 import BADPRIOR, FEW, KERNELS, MOUNT, NOTPD, OK, _dev, _dev_args
from tests.test_dense_ba_uncertainty_gpu import SHAPES, _case, _normal
from tests.test_depth_propagate_gpu import _same_bits

pytestmark = pytest.mark.gpu
STATES = [('none', 'prior'), ('huber', 'moved'), ('cauchy', 'moved')]


def _state(sc, refs, kind, st):
    """The inverse depths of a state as the op takes them: the perturbed ones, or the prior's 1 / depth (0 without a prior)."""
    return sc['rho'] if st == 'moved' else np.stack([r['rho0'] for r in refs[(kind, st)]])


def _vjp(sc, rho, sums, g, kind='none', marginal=True, links=None, **kw):
    pick = (lambda a: a) if links is None else (lambda a: a[links])
    kw.setdefault('prior_scale', pick(_dev(sc['m'])))
    kw.setdefault('mask', pick(_dev(sc['mask'])))
    kw.setdefault('prior_weight', pick(_dev(sc['w'])))
    mask, w = kw.pop('mask'), kw.pop('prior_weight')
    return ops.dense_ba_depth_variance_vjp(pick(_dev(sc['depth'])), pick(_dev(sc['flow'])), mask, pick(_dev(sc['start'])), pick(_dev(sc['intr'])), w,
                                           pick(_dev(rho)), sums, pick(_dev(g)), rgb2imu=_dev(MOUNT), kernel=KERNELS[kind], marginal=marginal, **kw)


def _reference(sc, b, rho, kind, Scam, marginal, g):
    r = vg.link_terms(sc['depth'][b], sc['flow'][b], sc['mask'][b], sc['start'][b], MOUNT, sc['intr'][b], sc['w'][b], sc['m'][b], rho[b], KERNELS[kind])
    return r, vg.variance_vjp_reference_link(r, Scam, marginal, g[b], sc['start'][b], MOUNT)


# ------------------------------------------------------------------------------------------------ 1. the op against the closed forms
@pytest.mark.parametrize('kind,st', STATES)
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_op_matches_closed_forms(cuda, B, H, W, kind, st):
    """ops.dense_ba_depth_variance_vjp on the device forward's own sums against variance_vjp_reference_link given the same sums bits, in
    both modes.  Measured shares of the bounds: see DESIGN.md section 3.32."""
    sc, refs = _case(B, H, W)
    rho = _state(sc, refs, kind, st)
    sums = _normal(sc, kind, st).sums
    sums_np = sums.cpu().numpy()
    g = np.random.default_rng(500 + H).standard_normal((B, H, W))
    for marginal in (True, False):
        out = _vjp(sc, rho, sums, g, kind, marginal)
        got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
        assert got['status'].tolist() == [OK] * B and out.grad_flow.dtype == torch.float32 and out.grad_motion.shape == (B, 7)
        worst = dict.fromkeys(vg.NAMES, 0.0)
        for b in range(B):
            Scam = scam_from_sums(sums_np[b])
            cond = np.linalg.cond(Scam)
            assert cond < 1e9
            r, ref = _reference(sc, b, rho, kind, Scam, marginal, g)
            assert np.array_equal(r['valid'], refs[(kind, st)][b]['valid'])
            for name in vg.NAMES:
                assert np.isfinite(got[name][b]).all(), (b, name)
                k, extra = (vg.K_MOTION, 0.0) if name == 'grad_motion' else (vg.K_GRAD, vg.U32 if name == 'grad_flow' else 0.0)
                worst[name] = max(worst[name], vg.used(got[name][b], ref[name], ref['scale'][name], k, cond, extra))
            assert (got['grad_inv_depth'][b][~r['valid']] == 0).all() and (got['grad_flow'][b][:, ~r['valid']] == 0).all()
            assert (got['grad_inv_depth'][b][r['valid']] != 0).all() and np.abs(got['grad_motion'][b]).min() > 0
            if kind == 'huber' and H > 7:          # both branches occur (at 7 x 9 no residual reaches 1 px); the inner one has c' = 0
                assert r['out'].any() and (r['valid'] & ~r['out']).any()
            moved = {'none': np.zeros_like(r['valid']), 'huber': r['out'], 'cauchy': r['valid']}[kind]
            assert (got['grad_flow'][b][:, moved] != 0).all() and (got['grad_flow'][b][:, ~moved] == 0).all()
        print('%dx%dx%d %s %s %s: worst share of the bound: %s' % (B, H, W, kind, st, 'marginal' if marginal else 'conditional',
                                                                    {k: '%.2e' % v for k, v in worst.items()}))
        assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 2. repeatability, no map
def test_repeat_gives_the_same_bits_and_no_map_is_the_unit_map(cuda):
    sc, refs = _case(3, 136, 168)
    sums = _normal(sc, 'cauchy', 'moved').sums
    g = np.random.default_rng(601).standard_normal((3, 136, 168))
    for marginal in (True, False):
        one, two = _vjp(sc, sc['rho'], sums, g, 'cauchy', marginal), _vjp(sc, sc['rho'], sums, g, 'cauchy', marginal)
        for name, x, y in zip(one._fields, one, two):
            assert _same_bits(x, y), (marginal, name)
    sc, refs = _case(3, 24, 40)
    unit = torch.ones(sc['m'].shape, dtype=torch.float32, device='cuda')
    sums = _normal(sc, 'cauchy', 'moved', prior_scale=None).sums
    g = np.random.default_rng(602).standard_normal((3, 24, 40))
    for marginal in (True, False):
        a, b = _vjp(sc, sc['rho'], sums, g, 'cauchy', marginal, prior_scale=None), _vjp(sc, sc['rho'], sums, g, 'cauchy', marginal, prior_scale=unit)
        for name, x, y in zip(a._fields, a, b):
            assert _same_bits(x, y), (marginal, name)
        assert a.status.tolist() == [OK] * 3 and a.grad_inv_depth.abs().max() > 0


# ------------------------------------------------------------------------------------------------ 3. status on the middle link
def test_status_zeroes_only_its_own_link(cuda):
    """An incoming FEW, NOTPD from an empty mask and a device-side prior weight of 0 on the middle link: its three gradients are exact
    zeros, and the healthy links equal a batch without it bit for bit."""
    sc, _ = _case(3, 24, 40)
    d = _dev_args(sc, sc['start'])
    keep = [0, 2]
    w, m, C = _dev(sc['w']), _dev(sc['m']), _dev(MOUNT)
    g = np.random.default_rng(603).standard_normal((3, 24, 40))
    rho = _dev(sc['rho'])
    hs = ops.dense_ba_normal(*(x[keep] for x in d), w[keep], inv_depth=rho[keep], rgb2imu=C, prior_scale=m[keep]).sums
    healthy = _vjp(sc, sc['rho'], hs, g, links=keep)
    assert healthy.status.tolist() == [OK, OK] and healthy.grad_inv_depth.abs().max() > 0
    empty = d[2].clone()
    empty[1] = 0
    wb = w.clone()
    wb[1] = 0.0
    sums_of = lambda mask, wt: ops.dense_ba_normal(d[0], d[1], mask, d[3], d[4], wt, inv_depth=rho, rgb2imu=C, prior_scale=m).sums
    few = torch.tensor([OK, FEW, OK], dtype=torch.int32, device='cuda')
    for name, mask, wt, status, want in (('few incoming', d[2], w, few, FEW), ('notpd from an empty mask', empty, w, None, NOTPD),
                                         ('badprior', d[2], wb, None, BADPRIOR)):
        out = _vjp(sc, sc['rho'], sums_of(mask, wt), g, mask=mask, prior_weight=wt, status=status)
        assert out.status.tolist() == [OK, want, OK], name
        assert not out.grad_inv_depth[1].any() and not out.grad_flow[1].any() and not out.grad_motion[1].any(), name
        for field in ('grad_inv_depth', 'grad_flow', 'grad_motion'):
            assert _same_bits(getattr(out, field)[keep], getattr(healthy, field)), (name, field)


# ------------------------------------------------------------------------------------------------ 4. NaN cotangents
@pytest.mark.parametrize('B,H,W', SHAPES[:2])
def test_nan_cotangents_where_the_variance_is_nan(cuda, B, H, W):
    """Cotangents that are NaN exactly where v is NaN (what torch.sqrt's backward hands over there): every output is finite and equals
    the one with zeros there, bit for bit."""
    sc, _ = _case(B, H, W)
    sums = _normal(sc, 'cauchy', 'moved').sums
    fwd = ops.dense_ba_depth_variance(*_dev_args(sc, sc['start']), _dev(sc['w']), inv_depth=_dev(sc['rho']), sums=sums, prior_scale=_dev(sc['m']),
                                      rgb2imu=_dev(MOUNT), kernel=KERNELS['cauchy'])
    nan = torch.isnan(fwd.var).cpu().numpy()
    assert nan.sum() == 6 * B
    g = np.random.default_rng(604).standard_normal((B, H, W))
    for marginal in (True, False):
        bad = _vjp(sc, sc['rho'], sums, np.where(nan, np.nan, g), 'cauchy', marginal)
        good = _vjp(sc, sc['rho'], sums, np.where(nan, 0.0, g), 'cauchy', marginal)
        for name, x, y in zip(bad._fields, bad, good):
            assert torch.isfinite(x.double()).all() and _same_bits(x, y), (marginal, name)


# ------------------------------------------------------------------------------------------------ 5. wiring
def _plane_chain(seq, differentiable, variance=True):
    """Two links of plane_sequence through refine_joint -> depth_uncertainty -> propagate -> refine_joint.  differentiable: the
    refinements and the propagation carry their gradients; variance: depth_uncertainty does too."""
    fx, fy, cx, cy = seq['intr']
    H, W = seq['stereo'].shape[1:]
    ident = pp.SE3(torch.tensor([0, 0, 0, 0, 0, 0, 1.0], dtype=torch.float64, device='cuda'))
    kw = dict(differentiable=True, hessian='exact') if differentiable else {}
    depth0, flow0 = _dev(seq['stereo'][0])[None].requires_grad_(differentiable), _dev(seq['flow'][0])[None].requires_grad_(differentiable)
    loss0 = DenseReprojectionLoss(depth0, flow0, fx, fy, cx, cy, None, ident, device='cuda')
    sigma0 = torch.full((1, H, W), SIGMA_STEREO, dtype=torch.float64, device='cuda')
    j0 = loss0.refine_joint(pp.SE3(_dev(seq['start'][0])[None]), sigma0, sigma_px=SIGMA_PX, iters=20, **kw)
    unc = loss0.depth_uncertainty(j0, sigma0, sigma_px=SIGMA_PX, **(dict(differentiable=True) if differentiable and variance else {}))
    meas = dict(depth_next=_dev(seq['stereo'][1])[None], sigma_inv_depth_next=SIGMA_STEREO, process_sigma=float(np.sqrt(seq['process_var'][1])), gate=3.0)
    prior = loss0.propagate(j0, unc, differentiable=differentiable, **meas)
    loss1 = DenseReprojectionLoss(prior.depth, _dev(seq['flow'][1])[None], fx, fy, cx, cy, None, ident, device='cuda')
    j1 = loss1.refine_joint(pp.SE3(_dev(seq['start'][1])[None]), prior.sigma_inv_depth.detach(), sigma_px=SIGMA_PX, iters=20, **kw)
    return dict(depth0=depth0, flow0=flow0, j0=j0, unc=unc, prior=prior, j1=j1, loss0=loss0, meas=meas, sigma0=sigma0)


def _losses(ch, seq, c, e):
    """The three terms of the loss: on the propagated variance (where something is known), the Gaussian negative log-likelihood of link
    0's refined inverse depths under their own variance, and on link 1's refined pose."""
    known = ch['prior'].flags != 0
    on_prior = 1e3 * (ch['prior'].var_inv_depth * e)[known].sum()
    var, rho = ch['unc'].var_inv_depth, ch['j0'].inv_depth
    nll = ((rho - _dev(seq['rho_true'][0])[None]) ** 2 / var + torch.log(var)).mean()
    return on_prior, nll, (ch['j1'].motion * c).sum()


def test_one_backward_runs_through_the_variance(cuda):
    """plane_sequence(24, 40, K=2, seed=0): link 0 refine_joint(differentiable=True, hessian='exact') ->
    depth_uncertainty(differentiable=True) -> propagate(differentiable=True) -> link 1's refinement; L = a term on prior.var_inv_depth
    + the Gaussian NLL of unc.var_inv_depth against the scene's true rho + a term on link 1's refined pose.  One L.backward() to link
    0's stored depth and flow equals the chain done by hand, bit for bit: autograd.grad stage by stage, with
    ops.dense_ba_depth_propagate_vjp and ops.dense_ba_depth_variance_vjp called directly, the cotangents of a tensor added in the order
    the autograd engine adds them (the most recently created consumer first).  The gradient differs from the one obtained with
    depth_uncertainty(differentiable=False), and every stage's forward outputs equal those of the non-differentiable chain, bit for
    bit."""
    seq = plane_sequence(24, 40, K=2, seed=0)
    ch = _plane_chain(seq, True)
    j0, j1, prior, unc, depth0, flow0, loss0 = ch['j0'], ch['j1'], ch['prior'], ch['unc'], ch['depth0'], ch['flow0'], ch['loss0']
    assert j0.status.tolist() == [OK] and unc.status.tolist() == [OK] and prior.status.tolist() == [OK] and j1.status.tolist() == [OK]
    assert unc.var_inv_depth.grad_fn is not None and unc.sigma_inv_depth.grad_fn is not None and unc.sigma_depth.grad_fn is not None
    assert not unc.status.requires_grad and torch.isfinite(unc.var_inv_depth).all()
    rng = np.random.default_rng(23)
    c, e = _dev(rng.standard_normal((1, 7))), _dev(rng.standard_normal((1, 24, 40)))
    on_prior, nll, on_pose = _losses(ch, seq, c, e)
    L = on_prior + nll + on_pose
    # by hand
    K4 = torch.tensor(loss0.K4, dtype=torch.float64)
    g_pvar, g_prho = torch.autograd.grad(L, [prior.var_inv_depth, prior.inv_depth], retain_graph=True)
    m = ch['meas']
    gp = ops.dense_ba_depth_propagate_vjp(j0.inv_depth, unc.var_inv_depth, j0.motion, K4, prior.source, prior.flags, prior.status, grad_inv_depth=g_prho,
                                          grad_var_inv_depth=g_pvar, rgb2imu=pp._plain(loss0.rgb2imu_pose),
                                          process_var=m['process_sigma'] * m['process_sigma'], depth_next=m['depth_next'],
                                          var_next=loss0._variance_next(SIGMA_STEREO, 'propagate'))
    n_var, = torch.autograd.grad(nll, unc.var_inv_depth, retain_graph=True)
    # the NLL's own partial in rho: the same operations on the variance without its graph (through the variance it is gv below)
    n_rho, = torch.autograd.grad(_losses(dict(ch, unc=unc._replace(var_inv_depth=unc.var_inv_depth.detach())), seq, c, e)[1], j0.inv_depth)
    g_var = (n_var + gp.grad_var_inv_depth) * SIGMA_PX ** 2          # var_inv_depth = sigma_px^2 v
    gv = ops.dense_ba_depth_variance_vjp(loss0.z, loss0.flow, loss0.mask, j0.motion, K4, SIGMA_PX ** 2, j0.inv_depth, j0.sums, g_var, status=j0.status,
                                         prior_scale=loss0._prior_weight(ch['sigma0'], SIGMA_PX, 'test')[1], rgb2imu=pp._plain(loss0.rgb2imu_pose))
    assert gv.status.tolist() == [OK] and gv.grad_inv_depth.abs().max() > 0 and gv.grad_motion.abs().min() > 0
    cot_rho = (n_rho + gp.grad_inv_depth) + gv.grad_inv_depth
    cot_motion = gp.grad_motion + gv.grad_motion
    hand_depth, hand_flow = torch.autograd.grad([j0.inv_depth, j0.motion], [depth0, flow0], [cot_rho, cot_motion], retain_graph=True)
    hand_flow = gv.grad_flow + hand_flow
    L.backward()
    assert depth0.grad is not None and flow0.grad is not None and torch.isfinite(depth0.grad).all() and torch.isfinite(flow0.grad).all()
    print('max |one backward - by hand|: depth %.3e of %.3e, flow %.3e of %.3e' % (
        (depth0.grad - hand_depth).abs().max().item(), hand_depth.abs().max().item(), (flow0.grad - hand_flow).abs().max().item(),
        hand_flow.abs().max().item()))
    assert _same_bits(depth0.grad, hand_depth) and _same_bits(flow0.grad, hand_flow)
    # the variance branch contributes: the same loss with depth_uncertainty(differentiable=False)
    dead = _plane_chain(seq, True, variance=False)
    assert dead['unc'].var_inv_depth.grad_fn is None
    sum(_losses(dead, seq, c, e)).backward()
    diff_d, diff_f = (depth0.grad - dead['depth0'].grad).abs().max().item(), (flow0.grad - dead['flow0'].grad).abs().max().item()
    print('the variance branch moves the gradient by %.3e (depth, of %.3e) and %.3e (flow, of %.3e)' % (
        diff_d, depth0.grad.abs().max().item(), diff_f, flow0.grad.abs().max().item()))
    assert diff_d > 0 and diff_f > 0
    # the forward pass is the default one's
    plain = _plane_chain(seq, False)
    for stage, names in (('j0', ('motion', 'inv_depth', 'sums', 'depth', 'status')), ('unc', ('var_inv_depth', 'sigma_inv_depth', 'sigma_depth', 'status')),
                         ('prior', ('depth', 'sigma_inv_depth', 'inv_depth', 'var_inv_depth', 'source', 'flags', 'status')),
                         ('j1', ('motion', 'inv_depth', 'depth', 'status'))):
        for name in names:
            assert not getattr(plain[stage], name).requires_grad
            assert _same_bits(getattr(ch[stage], name).detach(), getattr(plain[stage], name)), (stage, name)
            assert _same_bits(getattr(dead[stage], name).detach(), getattr(plain[stage], name)), (stage, name)


# ------------------------------------------------------------------------------------------------ 6. forward bits
def test_differentiable_forward_has_the_default_bits(cuda):
    """depth_uncertainty(differentiable=True) returns all four fields bit-equal to the default path on the (3,24,40) case with a sigma
    map (NaN, 0 and -1 entries and pixels without a depth included), in both modes; its three maps carry a graph over the state, the
    pose and the stored flow, and the NaN that torch.sqrt's backward forms where the variance is NaN never reaches a gradient."""
    sc, _ = _case(3, 24, 40)
    fx, fy, cx, cy = sc['intr'][0]
    leaf = lambda a: _dev(a).requires_grad_()
    flow, rho, motion = leaf(sc['flow']), leaf(sc['rho']), leaf(sc['start'])
    loss = DenseReprojectionLoss(_dev(sc['depth']), flow, fx, fy, cx, cy, _dev(sc['mask']), pp.SE3(_dev(MOUNT)), device='cuda')
    with np.errstate(divide='ignore', invalid='ignore'):
        sigma = _dev(1.0 / np.sqrt(sc['m'].astype(np.float64)))          # the map m = 1 / sigma^2; its 0, NaN and -1 give inf, NaN, NaN
    w, m = loss._prior_weight(sigma, SIGMA_PX, 'test')
    sums = ops.dense_ba_normal(loss.z, loss.flow, loss.mask, motion, torch.tensor(loss.K4, dtype=torch.float64), w, inv_depth=rho, prior_scale=m,
                               rgb2imu=pp._plain(loss.rgb2imu_pose), kernel=KERNELS['cauchy']).sums
    joint = DenseBAJoint(*([None] * 14))._replace(motion=motion, inv_depth=rho, sums=sums, status=torch.zeros(3, dtype=torch.int32, device='cuda'))
    for marginal in (True, False):
        kw = dict(sigma_px=SIGMA_PX, kernel=KERNELS['cauchy'], marginal=marginal)
        a, b = loss.depth_uncertainty(joint, sigma, differentiable=True, **kw), loss.depth_uncertainty(joint, sigma, **kw)
        assert b.status.tolist() == [OK] * 3 and torch.isnan(b.var_inv_depth).sum().item() == 18
        for name in a._fields:
            assert _same_bits(getattr(a, name).detach(), getattr(b, name).detach()), (marginal, name)
        assert b.var_inv_depth.grad_fn is None and not a.status.requires_grad
        assert a.var_inv_depth.grad_fn is not None and a.sigma_inv_depth.grad_fn is not None and a.sigma_depth.grad_fn is not None
        flow.grad = rho.grad = motion.grad = None
        torch.nan_to_num(a.sigma_inv_depth).sum().backward(retain_graph=True)
        for t in (flow, rho, motion):
            assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0, marginal
        assert flow.grad.dtype == torch.float32
        # sigma_depth = sigma_inv_depth / rho^2 is formed in torch: where it is NaN its own quotient rule hands rho a NaN, nothing else
        flow.grad = rho.grad = motion.grad = None
        have = torch.isfinite(b.var_inv_depth)
        a.sigma_depth[have].sum().backward()
        assert torch.isfinite(flow.grad).all() and torch.isfinite(motion.grad).all() and torch.isfinite(rho.grad[have]).all()
