"""The gradient of the posterior depth variance (include/islam_hip.h, islam_dense_ba_depth_var_vjp): everything
that can be checked without a GPU -- the closed forms of tests/dense_ba_var_grad_f64.py against torch.autograd on the float64
restatement (S_cam recomputed inside it) and against central differences of the existing variance_reference, the share of the S_cam
path, the case table -- and the host-side argument errors, the Python plumbing and the register metadata of the three new kernels."""
import inspect
import os

import numpy as np
import pytest
import torch

from islam_amd import robust
from tests import dense_ba_var_grad_f64 as vg
from tests.dense_ba_var_f64 import scam_from_sums, variance_reference
from tests.dense_reproj_f64 import FEW, MOUNT, U, make_scene, noisy_prior, right_perturb

MODES = [True, False]


def _schur_link(kind, mapped):
    """Section 3.25's 7 x 9 Schur scene (tests/test_dense_ba_uncertainty_cpu.py): seed 107, the mount, a user mask, every clause dropping
    pixels, a perturbed rho, w = 1 -- with m = 1 or a map between 0.25 and 4.  Huber at 0.3 px, where the scene has both branches."""
    sc = noisy_prior(make_scene(1, 7, 9, seed=107, noise=0.3), seed=1)
    start = right_perturb(sc['motion'][0], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    rho = (1.0 / sc['depth'][0].astype(np.float64)) * (1.0 + 0.03 * np.random.default_rng(4).standard_normal((7, 9)))
    m = np.exp2(np.random.default_rng(5).uniform(-2.0, 2.0, (7, 9))).astype(np.float32) if mapped else None
    kernel = {'none': None, 'huber': robust.Huber(0.3), 'cauchy': robust.Cauchy(1.0)}[kind]
    return dict(depth=sc['depth'][0], flow=sc['flow'][0].astype(np.float64), mask=sc['mask'][0], motion=start, rgb2imu=MOUNT, intr=sc['intr'][0], wb=1.0,
                m=m, rho=rho, kernel=kernel)


def _case_link(kind, mapped, b=0):
    """A link of the (3,24,40) case of the uncertainty tests (tests/test_dense_ba_uncertainty_gpu.py: per-link intrinsics and weights,
    three pixels without a depth, three whose map entry is 0, NaN and -1) at its perturbed rho."""
    from tests.test_dense_ba_uncertainty_gpu import _case
    sc, _ = _case(3, 24, 40)
    kernel = {'none': None, 'huber': robust.Huber(1.0), 'cauchy': robust.Cauchy(1.0)}[kind]
    return dict(depth=sc['depth'][b], flow=sc['flow'][b].astype(np.float64), mask=sc['mask'][b], motion=sc['start'][b], rgb2imu=MOUNT, intr=sc['intr'][b],
                wb=float(sc['w'][b]), m=sc['m'][b] if mapped else None, rho=sc['rho'][b], kernel=kernel)


def _links(kinds=('none', 'huber', 'cauchy'), maps=(False, True)):
    for kind in kinds:
        for mapped in maps:
            yield '7x9 %s %s' % (kind, 'map' if mapped else 'w'), _schur_link(kind, mapped)
            yield '24x40 %s %s' % (kind, 'map' if mapped else 'w'), _case_link(kind, mapped, b=1 if mapped else 0)


def _terms(ln, **over):
    a = dict(ln, **over)
    return vg.link_terms(a['depth'], a['flow'], a['mask'], a['motion'], a['rgb2imu'], a['intr'], a['wb'], a['m'], a['rho'], a['kernel'])


def _closed(ln, r, marginal, g, **kw):
    return vg.variance_vjp_reference_link(r, scam_from_sums(r['sums']), marginal, g, ln['motion'], ln['rgb2imu'], **kw)


# ------------------------------------------------------------------------------------------------ 1. closed forms against autograd
def test_closed_forms_match_autograd_of_the_restatement():
    """Every output of variance_vjp_reference_link against torch.autograd.grad of the float64 restatement of v(rho, motion, flow), which
    recomputes S_cam from the same tensors on the same fixed valid set and Huber branch, with random cotangents: none, Huber and Cauchy,
    both modes, with and without a map, on the 7 x 9 Schur scene and the (3,24,40) case.  Within 2^-52 (K + 64 cond(S_cam)) of the sum
    of the magnitudes of the element's terms, K = K_GRAD (K_MOTION for grad_motion; counted in tests/dense_ba_var_grad_f64.py).  Huber
    has pixels on both branches."""
    worst = dict.fromkeys(vg.NAMES, 0.0)
    for k, (label, ln) in enumerate(_links()):
        r = _terms(ln)
        if isinstance(ln['kernel'], robust.Huber):
            assert r['out'].sum() >= 3 and (r['valid'] & ~r['out']).sum() >= 3, label
        else:
            assert not r['out'].any()
        Scam = scam_from_sums(r['sums'])
        cond = np.linalg.cond(Scam)
        assert cond < 1e9
        g = np.random.default_rng(40 + k).standard_normal(r['valid'].shape)
        for marginal in MODES:
            ref = _closed(ln, r, marginal, g)
            leaf = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
            rho, flow, motion = leaf(ln['rho']), leaf(ln['flow']), leaf(ln['motion'])
            v, S = vg.restatement_link(rho, motion, flow, r, ln['rgb2imu'], ln['intr'], ln['kernel'], marginal)
            want_v = variance_reference(r, Scam, marginal)[r['valid']]
            assert np.allclose(v.detach().numpy(), want_v, rtol=1e-9, atol=0.0) and np.allclose(S.detach().numpy(), Scam, rtol=1e-9, atol=1e-9 * np.abs(Scam).max())
            loss = (torch.from_numpy(g[r['valid']]) * v).sum()
            grads = torch.autograd.grad(loss, [rho, flow, motion], allow_unused=True)
            for name, got in zip(vg.NAMES, grads):
                got = np.zeros_like(ref[name]) if got is None else got.numpy()          # without a robust kernel v does not see the flow
                assert np.isfinite(got).all() and np.isfinite(ref[name]).all(), (label, name)
                used = vg.used(got, ref[name], ref['scale'][name], vg.K_MOTION if name == 'grad_motion' else vg.K_GRAD, cond)
                worst[name] = max(worst[name], used)
                assert used <= 1.0, (label, marginal, name, used)
            assert (ref['grad_inv_depth'][r['valid']] != 0).all() and np.abs(ref['grad_motion']).min() > 0, label
            assert (ref['grad_flow'] != 0).any() == (ln['kernel'] is not None), label
    print('worst share of the bound:', {k: '%.2e' % v for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ 2. closed forms against central differences
def test_closed_forms_match_central_differences_of_the_forward_restatement():
    """Directional derivatives of f = sum g v over the valid pixels by central differences of the existing variance_reference, S_cam
    recomputed at +h and -h from the restatement's own sums, in one random direction per input (rho, motion, flow) and one through all
    three, against the closed forms.  The steps: 2^-18 relative in rho, 2^-20 on the components of motion, 2^-12 px in the flow, and
    half of each.  The valid set and the Huber branch are identical at +h and -h, which is asserted and not skipped on.  The bound is
    the truncation term of the quotient at the smaller step, estimated from the two steps as |D(h) - D(h/2)| / 3 and taken twice, plus
    the rounding of the difference f(+) - f(-), 64 x 2^-52 (1 + cond(S_cam)) sum |g v| (cond: the solve against S_cam, marginal mode only; both sides are compared
    multiplied by the smaller step); it stays below 1e-2 of the derivative, so the comparison is not vacuous (asserted)."""
    for k, (label, ln) in enumerate(_links(maps=(True,))):
        r0 = _terms(ln)
        cond = np.linalg.cond(scam_from_sums(r0['sums']))
        g = np.random.default_rng(60 + k).standard_normal(r0['valid'].shape)
        rng = np.random.default_rng(80 + k)
        x0 = dict(rho=np.asarray(ln['rho'], np.float64), motion=np.asarray(ln['motion'], np.float64), flow=np.asarray(ln['flow'], np.float64))
        unit = dict(rho=2.0 ** -18 * x0['rho'] * rng.standard_normal(x0['rho'].shape), motion=2.0 ** -20 * rng.standard_normal(7),
                    flow=2.0 ** -12 * rng.standard_normal(x0['flow'].shape))
        keys = dict(rho='grad_inv_depth', motion='grad_motion', flow='grad_flow')
        for marginal in MODES:
            ref = _closed(ln, r0, marginal, g)
            v0 = variance_reference(r0, scam_from_sums(r0['sums']), marginal)
            S = float(np.abs(g * v0)[r0['valid']].sum())

            def f(x):
                r = _terms(ln, **x)
                assert np.array_equal(r['valid'], r0['valid']) and np.array_equal(r['out'], r0['out']) and np.array_equal(r['prior'], r0['prior']), label
                return float((g * variance_reference(r, scam_from_sums(r['sums']), marginal))[r0['valid']].sum())

            for which in list(unit) + ['all']:
                if which == 'flow' and ln['kernel'] is None:
                    continue          # v does not see the flow: both sides are exact zeros (test 3)
                quot = []
                for half in (1.0, 0.5):
                    xs = [{name: (x0[name] + sgn * half * unit[name] if which in (name, 'all') else x0[name]) for name in x0} for sgn in (1.0, -1.0)]
                    step = {name: 0.5 * (xs[0][name] - xs[1][name]) for name in x0}          # the direction as the two points hold it
                    want = sum(float(np.sum(ref[keys[name]] * step[name])) for name in x0)
                    quot.append((0.5 * (f(xs[0]) - f(xs[1])), want))
                d_big, d_small, want = 0.5 * quot[0][0], quot[1][0], quot[1][1]
                bound = 2.0 * abs(d_big - d_small) / 3.0 + 64.0 * U * (1.0 + (cond if marginal else 0.0)) * S
                print('%s, %s, %s: closed form %.9e, quotient %.9e, difference %.2e, bound %.2e' % (
                    label, 'marginal' if marginal else 'conditional', which, want, d_small, abs(want - d_small), bound))
                assert want != 0.0 and abs(want - d_small) <= bound, (label, marginal, which)
                assert bound <= 1e-2 * abs(want), (label, marginal, which)


# ------------------------------------------------------------------------------------------------ 3. the S_cam path, the flow without a kernel
def test_the_s_cam_path_is_real_and_the_flow_needs_a_robust_kernel():
    """The marginal-mode gradient with the cotangent of S_cam forced to zero differs from the full one in all three outputs on the
    7 x 9 scene (it is the gradient at a frozen S_cam, which autograd of the restatement does not give: test 1 would fail on it), and in
    conditional mode G is zero anyway.  Without a robust kernel grad_flow is exactly zero in both modes."""
    label, ln = '7x9', _schur_link('cauchy', True)
    r = _terms(ln)
    g = np.random.default_rng(7).standard_normal((7, 9))
    full, frozen = _closed(ln, r, True, g), _closed(ln, r, True, g, zero_G=True)
    assert np.abs(full['G']).max() > 0 and not frozen['G'].any()
    for name in vg.NAMES:
        d = np.abs(full[name] - frozen[name])
        print('%s: the S_cam path moves the gradient by up to %.3e of %.3e' % (name, d.max(), np.abs(full[name]).max()))
        assert d.max() > 1e-6 * np.abs(full[name]).max(), name
    cond_full, cond_frozen = _closed(ln, r, False, g), _closed(ln, r, False, g, zero_G=True)
    assert not cond_full['G'].any() and all(np.array_equal(cond_full[n], cond_frozen[n]) for n in vg.NAMES)
    for mapped in (False, True):
        ln = _schur_link('none', mapped)
        r = _terms(ln)
        for marginal in MODES:
            out = _closed(ln, r, marginal, g)
            assert not out['grad_flow'].any() and not out['scale']['grad_flow'].any() and out['grad_inv_depth'].any()


# ------------------------------------------------------------------------------------------------ 4. the case table
def test_case_table():
    """Exact zeros at the pixels whose v is 1 / w_i (a prior, invalid at the state) and at those whose v is NaN; cotangents that are
    NaN exactly where v is NaN give finite outputs, bit-equal to the ones with zeros there; a link with a status gets zeros."""
    ln = _case_link('cauchy', True, b=1)
    r = _terms(ln)
    Scam = scam_from_sums(r['sums'])
    g = np.random.default_rng(11).standard_normal(r['valid'].shape)
    for marginal in MODES:
        v = variance_reference(r, Scam, marginal)
        nan, const = np.isnan(v), r['prior'] & ~r['valid'] & ~np.isnan(v)
        assert nan.sum() == 6 and const.sum() > 100 and np.array_equal(v[const], 1.0 / r['w'][const])
        good = _closed(ln, r, marginal, np.where(nan, 0.0, g))
        bad = _closed(ln, r, marginal, np.where(nan, np.nan, g))
        for name in vg.NAMES:
            assert np.isfinite(bad[name]).all() and np.array_equal(bad[name], good[name]), (marginal, name)
        for sel in (nan, const):
            assert (good['grad_inv_depth'][sel] == 0).all() and (good['grad_flow'][:, sel] == 0).all()
        assert (good['grad_inv_depth'][r['valid']] != 0).all()
        dead = _closed(ln, r, marginal, g, status=FEW)
        assert not dead['grad_inv_depth'].any() and not dead['grad_flow'].any() and not dead['grad_motion'].any()


# ------------------------------------------------------------------------------------------------ 5. error paths and plumbing
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_exported_and_bound(lib):
    from islam_amd import _lib, dense_ba, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'islam_hip.h')).read()
    for name in ('islam_dense_ba_depth_var_vjp_scratch_bytes', 'islam_dense_ba_depth_var_vjp'):
        assert name in _lib.SIGNATURES and hasattr(lib._cdll, name), name
        assert name + '(' in header
    assert callable(ops.dense_ba_depth_variance_vjp) and issubclass(ops._DenseBADepthVariance, torch.autograd.Function)
    assert ops.DenseBADepthVarGrad._fields == ('grad_inv_depth', 'grad_flow', 'grad_motion', 'status')
    assert inspect.signature(dense_ba.DenseReprojectionLoss.depth_uncertainty).parameters['differentiable'].default is False
    f = lib.islam_dense_ba_depth_var_vjp_scratch_bytes
    need = 3 * (21 + 64 * 21 + 64 * 12) * 8
    assert f(0) == 0 and f(-1) == 0 and need <= f(3) < need + 3 * 256


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point: the rules of
    islam_dense_ba_depth_var, and a NULL inv_depth, grad_var or output."""
    one = 1        # any non-NULL address: a refused call never reads it

    def call(B=1, H=2, W=2, kind=0, delta=1.0, mode=0, depth=one, flow=one, motion=one, intr=one, prior=one, rho=one, sums=one, gvar=one, o1=one,
             o2=one, o3=one, st=one, scratch=one):
        return lib.islam_dense_ba_depth_var_vjp(depth, flow, None, motion, None, intr, prior, None, rho, sums, None, kind, delta, mode, gvar, o1, o2, o3,
                                                st, scratch, B, H, W, None)

    cases = [(dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
             (dict(kind=3), b'robust kind'), (dict(kind=-1), b'robust kind'), (dict(kind=1, delta=0.0), b'delta'), (dict(delta=-2.0), b'delta'),
             (dict(delta=float('nan')), b'delta'), (dict(mode=2), b'mode'), (dict(mode=-1), b'mode'), (dict(prior=None), b'prior_weight')]
    cases += [({k: None}, b'NULL') for k in ('depth', 'flow', 'motion', 'intr', 'rho', 'sums', 'gvar', 'o1', 'o2', 'o3', 'st', 'scratch')]
    for kw, what in cases:
        assert call(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_dense_ba_depth_var_vjp' in msg and what in msg, (kw, msg)


def _cpu_scene():
    sc = make_scene(2, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return sc, (t(sc['depth']), t(sc['flow']), t(sc['mask']), t(sc['motion']), t(sc['intr']))


def test_op_refuses_cpu_tensors():
    """Off the GPU the op raises RuntimeError: there is no CPU path."""
    from islam_amd import ops
    sc, args = _cpu_scene()
    rho, sums, g = 1.0 / args[0].double(), torch.ones(2, 30, dtype=torch.float64), torch.zeros(2, 7, 9, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_variance_vjp(*args, 2500.0, rho, sums, g)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_variance_vjp(*args, 2500.0, rho, sums, g, status=torch.zeros(2, dtype=torch.int32), prior_scale=torch.ones(2, 7, 9),
                                        rgb2imu=torch.from_numpy(MOUNT), kernel=robust.Cauchy(1.0), marginal=False)


def _cpu_joint(sc, args):
    from islam_amd.dense_ba import DenseBAJoint
    rho = (1.0 / args[0].double()).requires_grad_()
    motion = args[3].clone().requires_grad_()
    return DenseBAJoint(*([None] * 14))._replace(motion=motion, inv_depth=rho, sums=torch.ones(2, 30, dtype=torch.float64),
                                                 status=torch.zeros(2, dtype=torch.int32))


def test_depth_uncertainty_differentiable_argument_rules(monkeypatch):
    """depth_uncertainty(differentiable=True) keeps the argument rules of the default path, raises RuntimeError off the GPU, and hands
    ops._DenseBADepthVariance the stored depth, flow (NOT detached), mask, intrinsics and mount, the refinement's motion, inverse depths
    (both with their graph), sums and status, the prior weight and map of _prior_weight, the kernel and the mode; var_inv_depth,
    sigma_inv_depth and sigma_depth are formed in torch from what it returns."""
    from islam_amd import ops
    from tests.test_dense_ba_uncertainty_cpu import _cpu_loss
    sc, args = _cpu_scene()
    loss = _cpu_loss(sc)
    loss.flow.requires_grad_()
    joint = _cpu_joint(sc, args)
    with pytest.raises(RuntimeError, match='device tensors'):
        loss.depth_uncertainty(joint, 0.02, differentiable=True)
    calls = []

    class Fake:
        @staticmethod
        def apply(*a):
            calls.append(a)
            var = torch.full((2, 7, 9), 4.0, dtype=torch.float64)
            var[0, 0, 0] = float('nan')
            return var, torch.zeros(2, dtype=torch.int32)

    monkeypatch.setattr(ops, '_DenseBADepthVariance', Fake)
    monkeypatch.setattr(ops, 'dense_ba_depth_variance', lambda *a, **k: pytest.fail('the default path was taken'))
    kern = robust.Huber(0.5)
    sig = torch.full((2, 7, 9), 0.02, dtype=torch.float64)
    sig[1, 2, 3] = float('nan')
    out = loss.depth_uncertainty(joint, sig, sigma_px=0.5, kernel=kern, marginal=False, differentiable=True)
    depth, flow, mask, motion, intr, w, rho, sums, status, m, mount, kernel, marginal = calls[-1]
    assert depth is loss.z and flow is loss.flow and flow.requires_grad and mask is loss.mask and motion is joint.motion and rho is joint.inv_depth
    assert sums is joint.sums and status is joint.status and intr.tolist() == list(loss.K4) and torch.equal(mount, torch.from_numpy(MOUNT))
    assert w == 0.25 and m.dtype == torch.float32 and m[1, 2, 3] == 0 and m[0, 0, 0] == np.float32(2500.0) and kernel is kern and marginal is False
    assert torch.equal(out.var_inv_depth[1], torch.full((7, 9), 1.0, dtype=torch.float64)) and torch.isnan(out.var_inv_depth[0, 0, 0])
    assert out.sigma_inv_depth[1, 1, 1] == 1.0 and torch.equal(out.sigma_depth[1], 1.0 / (joint.inv_depth[1] * joint.inv_depth[1]))
    assert out.sigma_depth.grad_fn is not None          # through rho itself
    loss.depth_uncertainty(joint, 0.02, differentiable=True)
    assert calls[-1][5] == (1.0 / 0.02) ** 2 and calls[-1][9] is None and calls[-1][12] is True and calls[-1][11] is None
    n = len(calls)
    for bad, what in ((torch.ones(2, 2), 'sigma_inv_depth'), (-1.0, 'sigma_inv_depth'), (float('nan'), 'sigma_inv_depth')):
        with pytest.raises(ValueError, match=what):
            loss.depth_uncertainty(joint, bad, differentiable=True)
    with pytest.raises(ValueError, match='sigma_px'):
        loss.depth_uncertainty(joint, 0.02, sigma_px=0.0, differentiable=True)
    assert len(calls) == n


def test_default_path_does_not_use_the_function(monkeypatch):
    from islam_amd import ops
    from tests.test_dense_ba_uncertainty_cpu import _cpu_loss
    sc, args = _cpu_scene()
    loss = _cpu_loss(sc)
    joint = _cpu_joint(sc, args)
    seen = []

    def fake(depth, flow, mask, motion, intr, w, **kw):
        seen.append(kw)
        return ops.DenseBADepthVar(torch.ones(2, 7, 9, dtype=torch.float64), torch.zeros(2, dtype=torch.int32))

    monkeypatch.setattr(ops, 'dense_ba_depth_variance', fake)
    monkeypatch.setattr(ops._DenseBADepthVariance, 'apply', staticmethod(lambda *a: pytest.fail('the Function was used')))
    a = loss.depth_uncertainty(joint, 0.02)
    b = loss.depth_uncertainty(joint, 0.02, differentiable=False)
    assert len(seen) == 2 and sorted(seen[0]) == ['inv_depth', 'kernel', 'marginal', 'prior_scale', 'rgb2imu', 'status', 'sums']
    assert a.var_inv_depth.grad_fn is None and b.var_inv_depth.grad_fn is None


# ------------------------------------------------------------------------------------------------ 6. the kernels' metadata
def test_new_kernels_have_no_private_segment_and_no_spill(lib):
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = _kernels()
    for want in ('depth_var_adj_partial_kernel', 'depth_var_vjp_kernel', 'depth_var_pose_kernel'):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert not any(part in found[0] for part in ('dense_reproj', 'dense_ba', 'reproj_vjp', 'reproj_ift', 'joint_adj')), found[0]
        blk = ks[found[0]]
        print(want, 'vgpr', _field(blk, 'vgpr_count'), 'sgpr', _field(blk, 'sgpr_count'), 'lds', _field(blk, 'group_segment_fixed_size'))
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0 and _field(blk, 'sgpr_spill_count') == 0, want
