"""The gradient of the joint (pose, inverse depth) refinement in depth and flow on the MI355X (csrc/dense_ba.hip, joint_adj_partial_kernel,
joint_adj_solve_kernel and joint_adj_vjp_kernel) against the float64 restatement of tests/dense_ba_grad_f64.py.

Shapes, seeds and scene conditions are section 3.25's (the scenes ARE those of tests/test_dense_ba_joint_gpu.py, at its perturbed
inverse depths), asserted again: 7 x 9 is below one workgroup, so most workgroups store empty rows; 24 x 40 is below the grid;
136 x 168 = 22848 takes a second trip of the grid-stride loop; B = 1 and 3 with per-link poses, intrinsics and prior weights; the mount,
the user mask, and three pixels without a prior.

Tolerances.  The VJP kernel computes in float64 and rounds once to float32 at the store, so per element
|got - ref| <= 2^-24 |ref| + 2^-40 sum|term| (section 3.24's bound: the store, and 4096 float64 roundings of head-room on the sum of the
magnitudes of the products the value is summed from).  lambda_p is held to numpy on the device's own S and the restatement's u_cam:
64 eps cond(S) |lambda| for the Cholesky solve plus the reduction bound of u_cam, 2^-52 (K + n) sum|parts| with K = 128 roundings per
term (counted in tests/dense_ba_grad_f64.py), pushed through |A^T| and |S^-1|."""
import functools

import numpy as np
import pytest
import torch

from islam_amd import lietensor as pp
from islam_amd import ops
from islam_amd.dense_ba import DenseReprojectionLoss
from tests.dense_ba_grad_f64 import K_ADJ, ba_adjoint_reference_link, ba_implicit_gradient, ba_vjp_reference_link
from tests.dense_reproj_f64 import (BADPRIOR, FEW, KERNELS, MOUNT, NOTPD, OK, PRIOR_W, SHAPES, U, _dev, _dev_args, make_scene, noisy_prior,
                                    right_perturb, tangent_from_pose_grad)
from tests.test_dense_ba_joint_gpu import NO_PRIOR, WEIGHTS
from tests.test_dense_ba_joint_gpu import _case as _joint_case

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """Section 3.25's scene of a shape at its perturbed inverse depths, with a lambda_p per link and a gradient on every inverse depth and
    on the pose, and the restatement of the VJP under each kernel (computed once)."""
    sc, joint = _joint_case(B, H, W)
    rng = np.random.default_rng(5 + H)
    sc = dict(sc, lam=rng.standard_normal((B, 6)), v_d=rng.standard_normal((B, H, W)), grad7=rng.standard_normal((B, 7)))
    refs = {k: [ba_vjp_reference_link(*_link(sc, b), sc['lam'][b], sc['v_d'][b], kern) for b in range(B)] for k, kern in KERNELS.items()}
    return sc, refs, joint


def _link(sc, b):
    return (sc['depth'][b], sc['flow'][b], sc['mask'][b], sc['start'][b], MOUNT, sc['intr'][b], float(sc['w'][b]), sc['rho'][b])


def _state(sc):
    """The device arguments both ops take ahead of their own: depth, flow, mask, motion, intr, prior_weight, inv_depth."""
    return _dev_args(sc, sc['start']) + (_dev(sc['w']), _dev(sc['rho']))


def _check(name, got_depth, got_flow, ref, extra_depth=0.0, extra_flow=0.0):
    """One link against the restatement: exact zeros where the formulas give zero (the flow gradient outside the valid set, the depth
    gradient without a prior), the bound everywhere else; returns the worst use of the bound."""
    worst = 0.0
    for what, got, want, mag, extra, live in (('depth', got_depth, ref['grad_depth'], ref['abs_depth'], extra_depth, ref['prior']),
                                              ('flow', got_flow, ref['grad_flow'], ref['abs_flow'], extra_flow, ref['valid'])):
        live = np.broadcast_to(live, want.shape)
        assert not got[~live].any(), '%s: %s is not zero where the formulas give zero' % (name, what)
        bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -40 * mag + extra
        err = np.abs(got.astype(np.float64) - want)
        use = float((err[live] / np.maximum(bound[live], 1e-300)).max())
        print('%s grad_%s: worst error / bound %.3f (largest |value| %.3e)' % (name, what, use, np.abs(want).max()))
        assert (err <= bound).all(), (name, what)
        worst = max(worst, use)
    return worst


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_scene_conditions(B, H, W):
    """On the restatement alone, at the state the tests use: every clause drops a pixel, at least half the pixels stay, none lies within
    1e-9 of a clause's threshold (so the zeros must sit exactly where the restatement's do), the three pixels without a prior are
    outside the valid set, and the user mask drops pixels that have a prior."""
    sc, refs, joint = _case(B, H, W)
    assert sc['w'].tolist() == WEIGHTS[:B].tolist() and (sc['intr'][:, 0] < W / 2).all()
    for b, r in enumerate(joint[('none', 'moved')]):
        assert (r['rejects'] > 0).all() and 2 * r['count'] >= H * W and np.nanmin(r['margin']) > 1e-9
        assert not any(r['valid'][p] or r['prior'][p] for p in NO_PRIOR)
        assert np.array_equal(r['valid'], refs['none'][b]['valid']) and np.array_equal(r['prior'], refs['none'][b]['prior'])
        assert (~sc['mask'][b] & r['prior']).any() and (~r['prior']).sum() == len(NO_PRIOR)


@pytest.mark.parametrize('kind', list(KERNELS))
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_vjp_matches_restatement(cuda, B, H, W, kind):
    sc, refs, _ = _case(B, H, W)
    call = lambda: ops.dense_ba_vjp(*_state(sc), _dev(sc['lam']), grad_inv_depth=_dev(sc['v_d']), rgb2imu=_dev(MOUNT), kernel=KERNELS[kind])
    gd, gf = call()
    assert gd.dtype == gf.dtype == torch.float32 and tuple(gd.shape) == (B, H, W) and tuple(gf.shape) == (B, 2, H, W)
    for x, y in zip((gd, gf), call()):          # a second call: the same bits
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    gd, gf = gd.cpu().numpy(), gf.cpu().numpy()
    for b, r in enumerate(refs[kind]):
        _check('%dx%d %s link %d' % (H, W, kind, b), gd[b], gf[b], r)
        assert np.abs(r['grad_depth']).max() > 0 and np.abs(r['grad_flow']).max() > 0
    if kind == 'huber' and H >= 24:          # both branches of the kernel are in use
        s = np.concatenate([r['s'][r['valid']] for r in refs[kind]])
        assert (s > 1.0).any() and (s <= 1.0).any()


def test_vjp_without_a_depth_gradient_and_without_mount_or_mask(cuda):
    """grad_inv_depth=None is v_d = 0; the identity mount and a missing mask take their own branches."""
    sc, _, _ = _case(1, 24, 40)
    d = _state(sc)
    gd, gf = ops.dense_ba_vjp(d[0], d[1], None, d[3], d[4], d[5], d[6], _dev(sc['lam']), kernel=KERNELS['cauchy'])
    a = _link(sc, 0)
    ref = ba_vjp_reference_link(a[0], a[1], None, a[3], None, *a[5:], sc['lam'][0], None, KERNELS['cauchy'])
    _check('identity mount, no mask, no depth gradient', gd[0].cpu().numpy(), gf[0].cpu().numpy(), ref)
    assert not gd[0].cpu().numpy()[~ref['valid']].any()          # without v_d an invalid pixel's lambda_d is 0


def test_a_link_with_a_status_gets_zeros(cuda):
    """status != 0 on the middle link: its gradients are all zero, its neighbours' bits are those of a call without a status and of a
    batch without it."""
    sc, _, _ = _case(3, 136, 168)
    args = _state(sc) + (_dev(sc['lam']),)
    kw = dict(grad_inv_depth=_dev(sc['v_d']), rgb2imu=_dev(MOUNT))
    plain = ops.dense_ba_vjp(*args, **kw)
    zeros = ops.dense_ba_vjp(*args, status=torch.zeros(3, dtype=torch.int32), **kw)
    marked = ops.dense_ba_vjp(*args, status=torch.tensor([OK, FEW, OK], dtype=torch.int32), **kw)
    keep = [0, 2]
    without = ops.dense_ba_vjp(*(x[keep] for x in args), grad_inv_depth=kw['grad_inv_depth'][keep], rgb2imu=_dev(MOUNT))
    for p, z, m, wo in zip(plain, zeros, marked, without):
        assert torch.equal(p, z)
        assert not m[1].any() and p[1].any()
        assert torch.equal(m[keep], p[keep]) and torch.equal(m[keep], wo)


def _lambda_bound(adj, cond, n):
    """How far the device's lambda_p may lie from numpy's on the same S (norm): the Cholesky solve, 64 eps cond |lambda|, and the
    reduction of u_cam, 2^-52 (K + n) sum|parts|, pushed through |A^T| and |S^-1|."""
    du = U * (K_ADJ + n) * adj['u_abs']
    return 64 * EPS * cond * np.linalg.norm(adj['lam_p']) + np.linalg.norm(np.abs(np.linalg.inv(adj['S'])) @ (np.abs(adj['A']).T @ du))


@pytest.mark.parametrize('kind', list(KERNELS))
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_ift_weights_match_numpy_on_the_device_S(cuda, B, H, W, kind):
    """lambda_p with and without a gradient on inv_depth, against numpy on the S the device returned at this state and the
    restatement's u_cam; cond(S) from numpy, asserted below 1e10.  A second call gives the same bits."""
    sc, _, _ = _case(B, H, W)
    st = _state(sc)
    S = ops.dense_ba_normal(*st[:6], inv_depth=st[6], rgb2imu=_dev(MOUNT), kernel=KERNELS[kind]).S
    Sd = S.cpu().numpy()
    for v_d in (sc['v_d'], None):
        call = lambda: ops.dense_ba_ift_weights(*st, S, _dev(sc['grad7']), grad_inv_depth=None if v_d is None else _dev(v_d), rgb2imu=_dev(MOUNT),
                                                kernel=KERNELS[kind])
        lam, status = call()
        again = call()
        assert lam.dtype == torch.float64 and status.dtype == torch.int32 and status.tolist() == [OK] * B and tuple(lam.shape) == (B, 6)
        assert torch.equal(lam, again[0]) and torch.equal(status, again[1])
        for b in range(B):
            adj = ba_adjoint_reference_link(*_link(sc, b), tangent_from_pose_grad(sc['start'][b], sc['grad7'][b]), None if v_d is None else v_d[b],
                                            KERNELS[kind], S=Sd[b])
            cond = np.linalg.cond(Sd[b])
            err, bound = np.linalg.norm(lam[b].cpu().numpy() - adj['lam_p']), _lambda_bound(adj, cond, adj['count'])
            print('%dx%d %s link %d, %s: cond(S) %.3e, |lambda| %.3e, |u| %.3e, error %.3e = %.4f of the bound' % (
                H, W, kind, b, 'v_d' if v_d is not None else 'no v_d', cond, np.linalg.norm(adj['lam_p']), np.linalg.norm(adj['u_cam']), err, err / bound))
            assert cond < 1e10
            assert err <= bound
            assert (np.abs(adj['u_cam']).max() > 0) == (v_d is not None)
            # the part of lambda_p that u_cam carries is far above the bound: a wrong or missing reduction would show
            if v_d is not None:
                assert np.linalg.norm(np.linalg.solve(Sd[b], adj['A'].T @ adj['u_cam'])) > 1e3 * bound


def test_ift_status_marks_only_its_own_link(cuda):
    """An indefinite S, an incoming status and (a device value) a prior weight of 0 on the middle link: that link alone is marked and
    gets lambda_p = 0."""
    sc, _, _ = _case(3, 24, 40)
    st = _state(sc)
    S = ops.dense_ba_normal(*st[:6], inv_depth=st[6], rgb2imu=_dev(MOUNT)).S
    kw = dict(grad_inv_depth=_dev(sc['v_d']), rgb2imu=_dev(MOUNT))
    lam, status = ops.dense_ba_ift_weights(*st, S, _dev(sc['grad7']), **kw)
    bad = S.clone()
    bad[1, 2, 2] = -bad[1, 2, 2]
    wb = st[5].clone()
    wb[1] = 0.0
    for name, (lx, sx), want in (('indefinite', ops.dense_ba_ift_weights(*st, bad, _dev(sc['grad7']), **kw), NOTPD),
                                 ('incoming', ops.dense_ba_ift_weights(*st, S, _dev(sc['grad7']), status=torch.tensor([OK, FEW, OK], dtype=torch.int32), **kw), FEW),
                                 ('bad prior', ops.dense_ba_ift_weights(*st[:5], wb, st[6], S, _dev(sc['grad7']), **kw), BADPRIOR)):
        assert sx.tolist() == [OK, want, OK], name
        assert not lx[1].any() and torch.equal(lx[0], lam[0]) and torch.equal(lx[2], lam[2]), name
    assert status.tolist() == [OK, OK, OK] and lam[1].any()


# ------------------------------------------------------------------------------------------------ end to end
SIGMA_PX = 0.3


@functools.lru_cache(maxsize=None)
def _loss_scene():
    sc = noisy_prior(make_scene(3, 24, 40, seed=124, noise=0.3, vary=False), seed=24)          # DenseReprojectionLoss holds one set of intrinsics
    for (r, c), val in NO_PRIOR.items():
        sc['depth'][:, r, c] = val
    sc['start'] = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    rng = np.random.default_rng(6)
    sc['coeff'], sc['coeff_depth'] = rng.standard_normal((3, 7)), rng.standard_normal((3, 24, 40)).astype(np.float32)
    sc['w'] = WEIGHTS.copy()
    return sc


def _loss(sc, mask=None):
    fx, fy, cx, cy = sc['intr'][0]
    depth, flow = _dev(sc['depth']).requires_grad_(), _dev(sc['flow']).requires_grad_()
    return depth, flow, DenseReprojectionLoss(depth, flow, fx, fy, cx, cy, _dev(sc['mask']) if mask is None else mask, pp.SE3(_dev(MOUNT)), device='cuda')


def _sigma(sc):
    return _dev(SIGMA_PX / np.sqrt(sc['w']))          # (B,) on the device: w = (sigma_px / sigma)^2


@pytest.mark.parametrize('what', ['motion', 'depth', 'both'])
@pytest.mark.parametrize('kind', ['none', 'huber'])
def test_backward_through_the_joint_refinement(cuda, kind, what):
    """refine_joint(differentiable=True) on leaf depth and flow, L = sum coeff . motion, L = sum coeff . depth (the refined depth MAP, so
    the gradient on inv_depth is autograd's own chain rule through 1 / rho) or both, backward(): .grad against the restatement evaluated
    at the device's returned state with the device's S.  Composed as section 3.24's end-to-end test composes its bounds: on top of the
    store's bound the device's lambda_p may differ from numpy's by the bound of test_ift_weights_match_numpy_on_the_device_S, and the
    gradient is linear in lambda_p, so the restatement's sum|term| at lambda_p = that difference in every component is added."""
    sc = _loss_scene()
    depth, flow, loss = _loss(sc)
    out = loss.refine_joint(pp.SE3(_dev(sc['start'])), _sigma(sc), sigma_px=SIGMA_PX, iters=20, kernel=KERNELS[kind], differentiable=True)
    assert out.motion.grad_fn is not None and out.inv_depth.grad_fn is not None and out.depth.grad_fn is not None and out.status.tolist() == [OK] * 3
    assert not out.S.requires_grad and not out.cost.requires_grad and out.depth.dtype == torch.float32
    L = 0.0
    if what in ('motion', 'both'):
        L = L + (out.motion * _dev(sc['coeff'])).sum()
    if what in ('depth', 'both'):
        L = L + (out.depth * _dev(sc['coeff_depth'])).sum()
    L.backward()
    assert depth.grad is not None and flow.grad is not None and depth.grad.dtype == flow.grad.dtype == torch.float32
    pose, rho, Sd = out.motion.detach().cpu().numpy(), out.inv_depth.detach().cpu().numpy(), out.S.cpu().numpy()
    gd, gf = depth.grad.cpu().numpy(), flow.grad.cpu().numpy()
    for b in range(3):
        grad7 = sc['coeff'][b] if what != 'depth' else np.zeros(7)
        with np.errstate(divide='ignore'):          # d(1/rho)/drho where the depth map follows rho; a pixel without a prior has rho = 0
            v_d = None if what == 'motion' else np.where(rho[b] > 0, -sc['coeff_depth'][b].astype(np.float64) / rho[b] ** 2, 0.0)
        args = (sc['depth'][b], sc['flow'][b], sc['mask'][b], pose[b], MOUNT, sc['intr'][b], float(sc['w'][b]), rho[b])
        ref = ba_implicit_gradient(*args, grad7, v_d, KERNELS[kind], S=Sd[b])
        cond = np.linalg.cond(Sd[b])
        assert cond < 1e10
        dl = _lambda_bound(ref, cond, ref['count'])
        dw = ba_vjp_reference_link(*args, np.full(6, dl), None, KERNELS[kind])
        _check('backward %s, loss on %s, link %d' % (kind, what, b), gd[b], gf[b], ref, dw['abs_depth'], dw['abs_flow'])
        assert np.abs(ref['grad_depth']).max() > 0 and np.abs(ref['grad_flow']).max() > 0
        assert (ref['u_cam'].any()) == (what != 'motion')


def test_default_path_has_no_graph_and_the_bits_of_the_op(cuda):
    """differentiable=False (and no argument at all): no grad_fn, the bits of ops.dense_ba_refine, which are also the differentiable
    run's."""
    sc = _loss_scene()
    depth, flow, loss = _loss(sc)
    motion = pp.SE3(_dev(sc['start']))
    kw = dict(sigma_px=SIGMA_PX, iters=8, kernel=KERNELS['huber'])
    plain, off, on = loss.refine_joint(motion, _sigma(sc), **kw), loss.refine_joint(motion, _sigma(sc), differentiable=False, **kw), \
        loss.refine_joint(motion, _sigma(sc), differentiable=True, **kw)
    direct = ops.dense_ba_refine(*_dev_args(sc, sc['start'])[:4], torch.tensor(loss.K4, dtype=torch.float64), (SIGMA_PX / _sigma(sc)) ** 2,
                                 rgb2imu=_dev(MOUNT), kernel=KERNELS['huber'], iters=8)
    for r in (plain, off):
        assert r.motion.grad_fn is None and not r.motion.requires_grad and r.inv_depth.grad_fn is None and r.depth.grad_fn is None
    for k in direct._fields[:-1]:
        for r in (plain, off, on):
            assert torch.equal(getattr(r, k).detach(), getattr(direct, k)), k
    assert torch.equal(plain.depth.view(torch.int32), on.depth.detach().view(torch.int32))


def test_backward_with_links_that_could_not_be_refined(cuda):
    """A FEW link (fewer valid pixels than min_count) and, in a second run, a BADPRIOR link (sigma = inf on the device, so w = 0 there
    and nothing is read back): that link's gradient is zero, the others' bits are those of the healthy batch, and nothing raises."""
    sc = _loss_scene()
    motion = pp.SE3(_dev(sc['start']))

    def run(mask=None, sigma=None):
        depth, flow, loss = _loss(sc, mask)
        out = loss.refine_joint(motion, _sigma(sc) if sigma is None else sigma, sigma_px=SIGMA_PX, iters=6, min_count=40, differentiable=True)
        ((out.motion * _dev(sc['coeff'])).sum() + (out.depth * _dev(sc['coeff_depth'])).sum()).backward()
        return out.status.tolist(), depth.grad, flow.grad

    st0, gd0, gf0 = run()
    assert st0 == [OK, OK, OK] and gd0[1].any() and gf0[1].any()
    mask = _dev(sc['mask']).clone()
    mask[1] = 0
    mask[1, 10:12, 17:22] = 1
    sigma = _sigma(sc).clone()
    sigma[1] = float('inf')
    for name, (st, gd, gf), want in (('few', run(mask=mask), FEW), ('bad prior', run(sigma=sigma), BADPRIOR)):
        assert st == [OK, want, OK], name
        assert not gd[1].any() and not gf[1].any(), name
        for b in (0, 2):
            assert gd[b].any() and torch.equal(gd[b], gd0[b]) and torch.equal(gf[b], gf0[b]), name
