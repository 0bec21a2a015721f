"""The gradient of the refined dense-reprojection pose in depth and flow on the MI355X (csrc/dense_reproj.hip, reproj_vjp_kernel and
reproj_ift_kernel) against the float64 restatement of tests/dense_reproj_f64.py.

Shapes as in tests/test_dense_reproj_gpu.py (the kernel is laid out like the partial kernel: 256 threads, 64 workgroups per link):
7 x 9 is below one wavefront, 24 x 40 leaves most workgroups idle, 136 x 168 = 22848 is above one grid stride of 16384 with a ragged
tail; B = 1 and 3, per-link poses and intrinsics, the non-identity mount, low depths and a 10 % user mask.

Tolerances.  The kernel computes in float64 and rounds once to float32 at the store, so per element
|got - ref| <= 2^-24 |ref| + 2^-40 sum|term|: the rounding of the store, and 4096 float64 roundings of head-room on the sum of the
magnitudes of the products the value is summed from (vjp_reference_link); a dropped term is O(1) of sum|term|."""
import functools

import numpy as np
import pytest
import torch

from islam_amd import lietensor as pp
from islam_amd import ops, robust
from islam_amd.dense_ba import DenseReprojectionLoss
from tests.dense_reproj_f64 import (FEW, KERNELS, MOUNT, NOTPD, OK, SEEDS, SHAPES, _dev, _dev_args, ift_weights_reference, make_scene,
                                    reproj_reference, right_perturb, scene_args, vjp_reference_link)

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _case(B, H, W):
    """The scene of a shape 0.02 away from the planted motion, a w per link, and the restatement under each kernel (computed once)."""
    sc = make_scene(B, H, W, seed=SEEDS[H], noise=0.3)
    sc['start'] = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    sc['w'] = np.random.default_rng(5).standard_normal((B, 6))
    refs = {k: [vjp_reference_link(sc['depth'][b], sc['flow'][b], sc['mask'][b], sc['start'][b], MOUNT, sc['intr'][b], sc['w'][b], kern)
                for b in range(B)] for k, kern in KERNELS.items()}
    return sc, refs


def _check(name, got_depth, got_flow, ref, extra_depth=0.0, extra_flow=0.0):
    """One link against the restatement; returns the worst use of the bound."""
    worst = 0.0
    for what, got, want, mag, extra in (('depth', got_depth, ref['grad_depth'], ref['abs_depth'], extra_depth),
                                        ('flow', got_flow, ref['grad_flow'], ref['abs_flow'], extra_flow)):
        valid = np.broadcast_to(ref['valid'], want.shape)
        assert not got[~valid].any(), '%s: %s is not zero at an invalid pixel' % (name, what)
        bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -40 * mag + extra
        err = np.abs(got.astype(np.float64) - want)
        use = float((err[valid] / bound[valid]).max())
        off = int((got[valid] != want[valid].astype(np.float32)).sum())
        print('%s grad_%s: worst error / bound %.3f (largest |value| %.3e); %d of %d values are not the float32 nearest to the restatement' % (
            name, what, use, np.abs(want).max(), off, int(valid.sum())))
        assert (err <= bound).all(), (name, what)
        worst = max(worst, use)
    return worst


@pytest.mark.parametrize('B,H,W', SHAPES)
def test_scene_conditions(B, H, W):
    """On the restatement alone: every validity clause drops a pixel on every link, at least half the pixels stay, and none lies
    within 1e-9 of a clause's threshold (so the zeros of the gradient must sit exactly where the restatement's do)."""
    sc, refs = _case(B, H, W)
    for b, r in enumerate(reproj_reference(*scene_args(sc, sc['start']))):
        print('%dx%d link %d: kept %d of %d, dropped by clause %s, closest margin %.2e' % (H, W, b, r['count'], H * W, r['rejects'], np.nanmin(r['margin'])))
        assert (r['rejects'] > 0).all() and not sc['mask'][b].all()
        assert 2 * r['count'] >= H * W
        assert np.nanmin(r['margin']) > 1e-9
        assert np.array_equal(r['valid'], refs['none'][b]['valid'])


@pytest.mark.parametrize('kind', list(KERNELS))
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_vjp_matches_restatement(cuda, B, H, W, kind):
    sc, refs = _case(B, H, W)
    gd, gf = ops.dense_reproj_vjp(*_dev_args(sc, sc['start']), _dev(sc['w']), rgb2imu=_dev(MOUNT), kernel=KERNELS[kind])
    assert gd.dtype == gf.dtype == torch.float32 and tuple(gd.shape) == (B, H, W) and tuple(gf.shape) == (B, 2, H, W)
    gd, gf = gd.cpu().numpy(), gf.cpu().numpy()
    for b, r in enumerate(refs[kind]):
        _check('%dx%d %s link %d' % (H, W, kind, b), gd[b], gf[b], r)
        assert np.abs(r['grad_depth']).max() > 0 and np.abs(r['grad_flow']).max() > 0
    if kind == 'huber' and H >= 24:          # both branches of the kernel are in use (the 43 pixels of 7 x 9 all lie below delta)
        s = np.concatenate([r['s'][r['valid']] for r in refs[kind]])
        assert (s > 1.0).any() and (s <= 1.0).any()


def test_identity_mount_and_missing_mask(cuda):
    sc, _ = _case(1, 24, 40)
    d = _dev_args(sc, sc['start'])
    gd, gf = ops.dense_reproj_vjp(d[0], d[1], None, d[3], d[4], _dev(sc['w']), kernel=robust.Cauchy(1.0))
    ref = vjp_reference_link(sc['depth'][0], sc['flow'][0], None, sc['start'][0], None, sc['intr'][0], sc['w'][0], robust.Cauchy(1.0))
    _check('identity mount, no mask', gd[0].cpu().numpy(), gf[0].cpu().numpy(), ref)


def test_two_calls_give_the_same_bits(cuda):
    sc, _ = _case(3, 136, 168)
    a = ops.dense_reproj_vjp(*_dev_args(sc, sc['start']), _dev(sc['w']), rgb2imu=_dev(MOUNT), kernel=robust.Huber(1.0))
    b = ops.dense_reproj_vjp(*_dev_args(sc, sc['start']), _dev(sc['w']), rgb2imu=_dev(MOUNT), kernel=robust.Huber(1.0))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_a_link_with_a_status_gets_zeros(cuda):
    """status != 0 on the middle link: its gradients are all zero, its neighbours' bits are those of a call without a status."""
    sc, _ = _case(3, 136, 168)
    args = _dev_args(sc, sc['start'])
    plain = ops.dense_reproj_vjp(*args, _dev(sc['w']), rgb2imu=_dev(MOUNT))
    zeros = ops.dense_reproj_vjp(*args, _dev(sc['w']), rgb2imu=_dev(MOUNT), status=torch.zeros(3, dtype=torch.int32))
    marked = ops.dense_reproj_vjp(*args, _dev(sc['w']), rgb2imu=_dev(MOUNT), status=torch.tensor([OK, FEW, OK], dtype=torch.int32))
    for p, z, m in zip(plain, zeros, marked):
        assert torch.equal(p, z)
        assert not m[1].any() and p[1].any()
        assert torch.equal(m[0], p[0]) and torch.equal(m[2], p[2])


def test_ift_weights_match_numpy_on_the_device_H(cuda):
    """w = -H^-1 v against numpy on the H the device returned: a Cholesky solve is backward stable, so the two solutions differ by a
    few eps cond(H) |w|; held to 64 eps cond(H) |w| with cond(H) from numpy, asserted below 1e10."""
    sc, _ = _case(3, 24, 40)
    ne = ops.dense_reproj_normal(*_dev_args(sc, sc['start']), rgb2imu=_dev(MOUNT))
    grad = np.random.default_rng(8).standard_normal((3, 7))
    w, status = ops.dense_reproj_ift_weights(ne.H, _dev(sc['start']), _dev(grad))
    assert w.dtype == torch.float64 and status.dtype == torch.int32 and status.tolist() == [OK, OK, OK]
    Hd = ne.H.cpu().numpy()
    for b in range(3):
        want = ift_weights_reference(Hd[b], sc['start'][b], grad[b])
        cond = np.linalg.cond(Hd[b])
        err = np.linalg.norm(w[b].cpu().numpy() - want)
        print('link %d: cond(H) %.3e, |w| %.3e, error %.3e = %.3f of the bound' % (b, cond, np.linalg.norm(want), err, err / (64 * EPS * cond * np.linalg.norm(want))))
        assert cond < 1e10
        assert err <= 64 * EPS * cond * np.linalg.norm(want)
    # an indefinite H on the middle link, and (separately) an incoming status: that link alone is marked and gets w = 0
    bad = ne.H.clone()
    bad[1, 2, 2] = -bad[1, 2, 2]
    w2, st2 = ops.dense_reproj_ift_weights(bad, _dev(sc['start']), _dev(grad))
    w3, st3 = ops.dense_reproj_ift_weights(ne.H, _dev(sc['start']), _dev(grad), status=torch.tensor([OK, FEW, OK], dtype=torch.int32))
    assert st2.tolist() == [OK, NOTPD, OK] and st3.tolist() == [OK, FEW, OK]
    for wx in (w2, w3):
        assert not wx[1].any() and torch.equal(wx[0], w[0]) and torch.equal(wx[2], w[2])


@functools.lru_cache(maxsize=None)
def _loss_scene():
    sc = make_scene(3, 24, 40, seed=124, noise=0.3, vary=False)          # DenseReprojectionLoss holds one set of intrinsics
    sc['start'] = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    sc['coeff'] = np.random.default_rng(6).standard_normal((3, 7))
    return sc


def _loss(sc, mask=None, leaf=True):
    fx, fy, cx, cy = sc['intr'][0]
    depth, flow = _dev(sc['depth']).requires_grad_(leaf), _dev(sc['flow']).requires_grad_(leaf)
    return depth, flow, DenseReprojectionLoss(depth, flow, fx, fy, cx, cy, _dev(sc['mask']) if mask is None else mask, pp.SE3(_dev(MOUNT)), device='cuda')


@pytest.mark.parametrize('kind', ['none', 'huber'])
def test_backward_through_the_refinement(cuda, kind):
    """refine(differentiable=True) on leaf depth and flow, L = sum coeff . motion, backward(): .grad against the restatement
    evaluated at the device's refined pose with w computed in numpy from the device's H.  On top of the store's bound the device's w
    may differ from numpy's by 64 eps cond(H) |w| (the test above), and the gradient is linear in w: the restatement's sum|term| at
    w = that difference in every component is added."""
    sc = _loss_scene()
    depth, flow, loss = _loss(sc)
    out = loss.refine(pp.SE3(_dev(sc['start'])), iters=10, kernel=KERNELS[kind], differentiable=True)
    assert isinstance(out, ops.DenseReprojRefined) and out.motion.grad_fn is not None and out.status.tolist() == [OK, OK, OK]
    assert not out.H.requires_grad and not out.cost.requires_grad
    (out.motion * _dev(sc['coeff'])).sum().backward()
    assert depth.grad is not None and flow.grad is not None and depth.grad.dtype == torch.float32
    pose, Hd = out.motion.detach().cpu().numpy(), out.H.cpu().numpy()
    gd, gf = depth.grad.cpu().numpy(), flow.grad.cpu().numpy()
    for b in range(3):
        w = ift_weights_reference(Hd[b], pose[b], sc['coeff'][b])
        cond = np.linalg.cond(Hd[b])
        assert cond < 1e10
        ref = vjp_reference_link(sc['depth'][b], sc['flow'][b], sc['mask'][b], pose[b], MOUNT, sc['intr'][b], w, KERNELS[kind])
        dw = vjp_reference_link(sc['depth'][b], sc['flow'][b], sc['mask'][b], pose[b], MOUNT, sc['intr'][b],
                                np.full(6, 64 * EPS * cond * np.linalg.norm(w)), KERNELS[kind])
        _check('backward %s link %d' % (kind, b), gd[b], gf[b], ref, dw['abs_depth'], dw['abs_flow'])
        assert np.abs(ref['grad_depth']).max() > 0 and np.abs(ref['grad_flow']).max() > 0
    # the default path: no grad_fn, the bits of ops.dense_reproj_refine and of the differentiable run
    plain = loss.refine(pp.SE3(_dev(sc['start'])), iters=10, kernel=KERNELS[kind])
    direct = ops.dense_reproj_refine(*_dev_args(sc, sc['start'])[:4], torch.tensor(loss.K4, dtype=torch.float64), rgb2imu=_dev(MOUNT),
                                     kernel=KERNELS[kind], iters=10)
    assert plain.motion.grad_fn is None and not plain.motion.requires_grad
    for k in ('motion', 'H', 'g', 'cost', 'l1', 'count', 'sums', 'damping', 'accepted', 'rejected', 'status'):
        assert torch.equal(getattr(plain, k), getattr(direct, k)) and torch.equal(getattr(plain, k), getattr(out, k).detach()), k


def test_backward_with_a_link_that_could_not_be_refined(cuda):
    """A link with fewer valid pixels than min_count (status FEW): its gradient is zero, the others' bits are those of a batch without
    it, and nothing raises."""
    sc = _loss_scene()
    mask = _dev(sc['mask']).clone()
    mask[1] = 0
    mask[1, 10:12, 17:22] = 1
    depth, flow, loss = _loss(sc, mask)
    out = loss.refine(pp.SE3(_dev(sc['start'])), iters=6, min_count=40, differentiable=True)
    assert out.status.tolist() == [OK, FEW, OK]
    (out.motion * _dev(sc['coeff'])).sum().backward()
    assert not depth.grad[1].any() and not flow.grad[1].any()
    depth2, flow2, loss2 = _loss(sc)
    out2 = loss2.refine(pp.SE3(_dev(sc['start'])), iters=6, min_count=40, differentiable=True)
    (out2.motion * _dev(sc['coeff'])).sum().backward()
    for b in (0, 2):
        assert depth.grad[b].any() and torch.equal(depth.grad[b], depth2.grad[b]) and torch.equal(flow.grad[b], flow2.grad[b])
