"""The gradient of depth propagation (include/islam_hip.h, islam_depth_propagate_vjp): everything that can be
checked without a GPU -- the closed forms of tests/dense_ba_prop_grad_f64.py against torch.autograd on the float64 restatement of the
smooth pieces and against central differences of the forward restatement (tests/dense_ba_prop_f64.py), the rows of the fusion table,
NaN cotangents and losers -- and the host-side argument errors, the Python plumbing and the register metadata of the two new kernels."""
import os

import numpy as np
import pytest
import torch

from tests import dense_ba_prop_grad_f64 as pg
from tests.dense_ba_prop_f64 import (FLAG_GATED, FLAG_MEAS, FLAG_PROP, gate_margin, prop_case, propagate_reference_link, scene_margins)
from tests.dense_reproj_f64 import FEW, MOUNT, OK, U, make_scene

CASES = [(1, 7, 9), (3, 24, 40)]          # the 7 x 9 large-motion scene and the (3,24,40) scene of prop_case
NAMES = ('grad_inv_depth', 'grad_var_inv_depth', 'grad_motion', 'grad_depth_next', 'grad_var_next')


def _links():
    """(label, the scene's arrays of one link, its forward restatement with the measurement at gate 3) for every link of CASES."""
    for shape in CASES:
        sc, refs = prop_case(*shape)
        for b in range(shape[0]):
            yield '%dx%d link %d' % (shape[1], shape[2], b), {k: sc[k][b] for k in ('rho', 'var', 'motion', 'intr', 'mask', 'depth_next', 'var_next')}, refs['gate3'][b]


def _cotangents(shape, seed):
    """Random cotangents of rho_f and s_f; a variance is some 1e3 times smaller than an inverse depth, its cotangent that much larger."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), 1e3 * rng.standard_normal(shape)


def _closed(ln, fw, gr, gs, **kw):
    args = dict(rho=ln['rho'], var=ln['var'], motion=ln['motion'], rgb2imu=MOUNT, intr=ln['intr'], process_var=0.0, depth_next=ln['depth_next'],
                var_next=ln['var_next'], source=fw['source'], flags=fw['flags'], status=fw['status'], g_rho=gr, g_var=gs)
    args.update(kw)
    return pg.propagate_vjp_reference_link(**args)


def _used(got, want, scale):
    """The largest |got - want| / (2^-52 scale) over the elements; an element without terms must agree exactly."""
    d = np.abs(np.asarray(got, np.float64) - want)
    assert (d[scale == 0] == 0).all()
    return float((d[scale > 0] / (U * scale[scale > 0])).max()) if (scale > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. closed forms against autograd
def test_closed_forms_match_autograd_of_the_restatement():
    """Every output of propagate_vjp_reference against torch.autograd.grad of the float64 restatement on the same winners and rows,
    the mount included, with random cotangents: within 2^-52 K_AD of the sum of the magnitudes of the element's terms (K_AD_MOTION for
    grad_motion; the counts are derived in tests/dense_ba_prop_grad_f64.py).  Both sides form the same T^-1 and the same forward values
    bit for bit, which the counts rely on and this test asserts."""
    worst = dict.fromkeys(NAMES, 0.0)
    for k, (label, ln, fw) in enumerate(_links()):
        gr, gs = _cotangents(ln['rho'].shape, 50 + k)
        ref = _closed(ln, fw, gr, gs)
        leaf = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
        ins = [leaf(ln[name]) for name in ('rho', 'var', 'motion', 'depth_next', 'var_next')]
        R2, tz = pg.torch_camera_inverse(ins[2], MOUNT)
        R, t = pg.camera_inverse(ln['motion'], MOUNT)
        assert np.array_equal(R2.detach().numpy(), R[2]) and tz.item() == t[2]
        rf, sf = pg.restatement_link(ins[0], ins[1], ins[2], MOUNT, ln['intr'], 0.0, ins[3], ins[4], fw['source'], fw['flags'], fw['status'])
        known = fw['flags'].ravel() != 0
        assert np.array_equal(rf.detach().numpy(), fw['inv_depth'].ravel()) and np.array_equal(sf.detach().numpy()[known], fw['var_inv_depth'].ravel()[known])
        sel = torch.from_numpy(known)
        loss = (torch.from_numpy(gr.ravel()) * rf)[sel].sum() + (torch.from_numpy(gs.ravel()) * sf)[sel].sum()
        grads = torch.autograd.grad(loss, ins)
        for name, g in zip(NAMES, grads):
            assert np.isfinite(g.numpy()).all() and np.isfinite(ref[name]).all() and (ref[name] != 0).sum() >= 7
            used = _used(g.numpy(), ref[name], ref['scale'][name]) / (pg.K_AD_MOTION if name == 'grad_motion' else pg.K_AD)
            worst[name] = max(worst[name], used)
            assert used <= 1.0, (label, name, used)
    print('worst share of the bound:', {k: round(v, 4) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ 2. closed forms against central differences
def _forward(ln, x):
    return propagate_reference_link(x['rho'], x['var'], ln['mask'], x['motion'], MOUNT, ln['intr'], OK, 0.0, x['depth_next'], x['var_next'], 3.0)


def _binade_step(x, shift):
    """2^(floor(log2 x) - shift) where x is finite and > 0, else 0: a step that keeps a float32 value exactly representable."""
    ok = np.isfinite(x) & (x > 0)
    return np.where(ok, np.exp2(np.floor(np.log2(np.where(ok, x, 1.0).astype(np.float64))) - shift), 0.0)


def test_closed_forms_match_central_differences_of_the_forward_restatement():
    """Directional derivatives of f = sum cr rho_f + cs s_f (over the targets where something is known) by central differences of the
    existing propagate_reference, in one random direction per input (rho, s, motion, depth_next, var_next) and one through all five,
    against the closed forms.  The steps: 2^-22 relative in rho, 2^-12 relative in s, 2^-25 on the components of motion, 2^-16 and 2^-12
    of a value's binade in depth_next and var_next (so that the float32 maps stay exact, asserted), and half of each.  The scenes'
    margins make them safe: the rounding distance of a link is above 5e-5 px, its z-gap above 1e-3 and its gate margin above 5e-3 (asserted), and
    u2 and v2 move by less than the rounding distance and rho' by less than half the z-gap under every step (asserted); source and flags
    are then identical at +h and -h, which is asserted and not skipped on.  The bound is the truncation term of the quotient at the
    smaller step, estimated from the two steps as |D(h) - D(h/2)| / 3 and taken twice, plus the rounding of the difference f(+) - f(-),
    64 x 2^-52 sum |c out| (both sides are compared multiplied by the smaller step, so nothing is divided by it); the bound stays below
    1e-2 of the derivative, so the comparison is not vacuous (asserted)."""
    for k, (label, ln, fw) in enumerate(_links()):
        m = scene_margins(propagate_reference_link(ln['rho'], ln['var'], ln['mask'], ln['motion'], MOUNT, ln['intr']))
        gm = gate_margin(fw, ln['depth_next'], ln['var_next'], 3.0)
        assert m.rounding > 5e-5 and m.zgap > 1e-3 and gm > 5e-3, (label, m, gm)
        gr, gs = _cotangents(ln['rho'].shape, 70 + k)
        ref = _closed(ln, fw, gr, gs)
        known = fw['flags'] != 0
        f = lambda r: float((gr * r['inv_depth'])[known].sum() + (gs * r['var_inv_depth'])[known].sum())
        S = float(np.abs(gr * fw['inv_depth'])[known].sum() + np.abs(gs * fw['var_inv_depth'])[known].sum())
        rng = np.random.default_rng(90 + k)
        shape = ln['rho'].shape
        sign = lambda: rng.choice([-1.0, 1.0], shape)
        x0 = {name: np.asarray(ln[name], np.float64) for name in ('rho', 'var', 'motion', 'depth_next', 'var_next')}
        unit = dict(rho=2.0 ** -22 * x0['rho'] * rng.standard_normal(shape), var=2.0 ** -12 * np.where(x0['var'] > 0, x0['var'], 0.0) * rng.standard_normal(shape),
                    motion=2.0 ** -25 * rng.standard_normal(7), depth_next=sign() * _binade_step(ln['depth_next'], 16),
                    var_next=sign() * _binade_step(ln['var_next'], 12))
        keys = dict(rho='grad_inv_depth', var='grad_var_inv_depth', motion='grad_motion', depth_next='grad_depth_next', var_next='grad_var_next')
        for which in list(unit) + ['all']:
            quot = []
            for half in (1.0, 0.5):
                at = []
                for sgn in (1.0, -1.0):
                    x = {name: (x0[name] + sgn * half * unit[name] if which in (name, 'all') else x0[name]) for name in x0}
                    for name in ('depth_next', 'var_next'):          # the float32 maps hold the perturbed values exactly
                        as32 = x[name].astype(np.float32)
                        assert np.array_equal(as32.astype(np.float64), x[name], equal_nan=True), (label, name)
                        x[name] = as32
                    r = _forward(ln, x)
                    assert np.array_equal(r['source'], fw['source']) and np.array_equal(r['flags'], fw['flags']), (label, which, half, sgn)
                    w, w0 = r['warp'], fw['warp']
                    pre = w0['pre']
                    assert max(np.abs(w['u2'] - w0['u2'])[pre].max(), np.abs(w['v2'] - w0['v2'])[pre].max()) < m.rounding
                    assert (np.abs(w['rp'] - w0['rp'])[pre] / w0['rp'][pre]).max() < 0.5 * m.zgap
                    at.append((f(r), x))
                # the direction as the two points hold it (a float64 sum rounds): the quotient is exact about their midpoint
                step = {name: np.nan_to_num(0.5 * (np.asarray(at[0][1][name], np.float64) - np.asarray(at[1][1][name], np.float64)), nan=0.0)
                        for name in x0}          # an absent entry (NaN) does not move
                want = sum(float(np.sum(ref[keys[name]] * step[name])) for name in x0)
                quot.append((0.5 * (at[0][0] - at[1][0]), want))
            # per unit of the smaller step: D(h) = quot[0] / 2, D(h/2) = quot[1], the closed form's value want = quot[1][1]
            d_big, d_small, want = 0.5 * quot[0][0], quot[1][0], quot[1][1]
            bound = 2.0 * abs(d_big - d_small) / 3.0 + 64.0 * U * S
            print('%s, %s: closed form %.9e, quotient %.9e, difference %.2e, bound %.2e' % (label, which, want, d_small, abs(want - d_small), bound))
            assert want != 0.0 and abs(want - d_small) <= bound, (label, which)
            assert bound <= 1e-2 * abs(want), (label, which)          # the quotient resolves the derivative: the check is not vacuous


# ------------------------------------------------------------------------------------------------ 3. rows, NaN cotangents, losers
def test_every_row_occurs_nan_cotangents_and_losers():
    """Every row of the fusion table occurs in the scenes (nothing, propagated only, measured only, both, gated).  With cotangents that
    are NaN exactly where nothing is known every gradient is finite and equals the one with zeros there; a candidate that lost its
    target gets exact zeros; the closed forms' rows: a gated or measured-only target passes its cotangents to the measurement alone."""
    seen = np.zeros(8, int)
    losers = 0
    for k, (label, ln, fw) in enumerate(_links()):
        seen += np.bincount(fw['flags'].ravel(), minlength=8)
        gr, gs = _cotangents(ln['rho'].shape, 110 + k)
        nothing = fw['flags'] == 0
        assert nothing.any()
        ref = _closed(ln, fw, np.where(nothing, 0.0, gr), np.where(nothing, 0.0, gs))
        got = _closed(ln, fw, np.where(nothing, np.nan, gr), np.where(nothing, np.nan, gs))
        for name in NAMES:
            assert np.isfinite(got[name]).all() and np.array_equal(got[name], ref[name]), (label, name)
        won = np.zeros(nothing.size, bool)
        won[fw['source'][fw['source'] >= 0]] = True
        lost = fw['warp']['cand'].ravel() & ~won
        losers += int(lost.sum())
        assert (got['grad_inv_depth'].ravel()[~won] == 0).all() and (got['grad_var_inv_depth'].ravel()[~won] == 0).all()
        alone = (fw['flags'] == FLAG_MEAS) | ((fw['flags'] & FLAG_GATED) != 0)
        rm = 1.0 / ln['depth_next'].astype(np.float64)[alone]
        assert np.array_equal(got['grad_depth_next'][alone], -(rm * rm) * gr[alone]) and np.array_equal(got['grad_var_next'][alone], gs[alone])
        gated_src = fw['source'][(fw['flags'] & FLAG_GATED) != 0]
        assert (got['grad_inv_depth'].ravel()[gated_src] == 0).all()          # the gate chose the measurement: the winner gets nothing
        only_p = fw['flags'] == FLAG_PROP
        assert (got['grad_depth_next'][only_p | nothing] == 0).all() and (got['grad_var_next'][only_p | nothing] == 0).all()
    assert (seen[[0, FLAG_PROP, FLAG_MEAS, FLAG_PROP | FLAG_MEAS, 7]] > 0).all() and seen[[4, 5, 6]].sum() == 0
    assert losers >= 50
    # a link with a status: zeros on the state and the pose, the measured-only row on the measurement
    label, ln, fw = next(x for x in _links() if x[0].startswith('24x40'))
    st = propagate_reference_link(ln['rho'], ln['var'], ln['mask'], ln['motion'], MOUNT, ln['intr'], FEW, 0.0, ln['depth_next'], ln['var_next'], 3.0)
    gr, gs = _cotangents(ln['rho'].shape, 130)
    got = _closed(ln, st, gr, gs)
    assert not got['grad_inv_depth'].any() and not got['grad_var_inv_depth'].any() and not got['grad_motion'].any()
    present = st['flags'] == FLAG_MEAS
    rm = 1.0 / ln['depth_next'].astype(np.float64)[present]
    assert np.array_equal(got['grad_depth_next'][present], -(rm * rm) * gr[present]) and (got['grad_depth_next'][~present] == 0).all()
    assert np.array_equal(got['grad_var_next'][present], gs[present]) and (got['grad_var_next'][~present] == 0).all()


# ------------------------------------------------------------------------------------------------ 4. error paths and plumbing
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_exported_and_bound(lib):
    from islam_amd import _lib, dense_ba, ops
    import inspect
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'islam_hip.h')).read()
    for name in ('islam_depth_propagate_vjp_scratch_bytes', 'islam_depth_propagate_vjp'):
        assert name in _lib.SIGNATURES and hasattr(lib._cdll, name), name
        assert name + '(' in header
    assert callable(ops.dense_ba_depth_propagate_vjp) and issubclass(ops._DenseBAPropagate, torch.autograd.Function)
    assert ops.DenseBAPropagateGrad._fields == ('grad_inv_depth', 'grad_var_inv_depth', 'grad_motion', 'grad_depth_next', 'grad_var_next')
    assert inspect.signature(dense_ba.DenseReprojectionLoss.propagate).parameters['differentiable'].default is False
    f = lib.islam_depth_propagate_vjp_scratch_bytes
    assert f(0) == 0 and f(-1) == 0 and 3 * 64 * 4 * 8 <= f(3) < 3 * 64 * 4 * 8 + 256


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    one = 1        # any non-NULL address: a refused call never reads it

    def call(B=1, H=2, W=2, rho=one, var=one, motion=one, intr=one, pv=one, dn=None, vn=None, src=one, fl=one, st=one, g1=None, g2=None, o1=one,
             o2=one, o3=one, o4=None, o5=None, scratch=one):
        return lib.islam_depth_propagate_vjp(rho, var, motion, None, intr, pv, dn, vn, src, fl, st, g1, g2, o1, o2, o3, o4, o5, scratch, B, H, W, None)

    cases = [(dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
             (dict(H=1 << 15, W=(1 << 15) + 1), b'bad shape'), (dict(dn=one), b'depth_next and var_next'), (dict(vn=one), b'depth_next and var_next'),
             (dict(dn=one, vn=one, o4=one), b'grad_depth_next and grad_var_next'), (dict(dn=one, vn=one, o5=one), b'grad_depth_next and grad_var_next'),
             (dict(o4=one, o5=one), b'without a measurement')]
    cases += [({k: None}, b'NULL') for k in ('rho', 'var', 'motion', 'intr', 'pv', 'src', 'fl', 'st', 'o1', 'o2', 'o3', 'scratch')]
    for kw, what in cases:
        assert call(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_depth_propagate_vjp' in msg and what in msg, (kw, msg)


def _op_args():
    sc = make_scene(2, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rho, var = 1.0 / t(sc['depth']).double(), torch.full((2, 7, 9), 1e-4, dtype=torch.float64)
    good = dict(inv_depth=rho, var_inv_depth=var, motion=t(sc['motion']), intr=t(sc['intr']), source=torch.full((2, 7, 9), -1, dtype=torch.int32),
                flags=torch.zeros(2, 7, 9, dtype=torch.uint8), status=torch.zeros(2, dtype=torch.int32))
    return sc, good, t(sc['depth']), torch.full((2, 7, 9), 4e-4)


def test_op_refuses_cpu_tensors_and_bad_arguments():
    """Off the GPU the op raises RuntimeError (there is no CPU path), after its argument rules, which raise ValueError."""
    from islam_amd import ops
    sc, good, dn, vn = _op_args()
    g = torch.zeros(2, 7, 9, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_propagate_vjp(**good)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_propagate_vjp(**good, grad_inv_depth=g, grad_var_inv_depth=g, rgb2imu=torch.from_numpy(MOUNT), process_var=1e-6, depth_next=dn,
                                         var_next=vn)
    for kw, what in ((dict(var_inv_depth=good['var_inv_depth'][:, :6]), 'var_inv_depth'), (dict(inv_depth=good['inv_depth'][0], var_inv_depth=good['var_inv_depth'][0]), 'inv_depth'),
                     (dict(motion=good['motion'][:1]), 'motion'), (dict(intr=torch.ones(3, 4)), 'intr'), (dict(rgb2imu=torch.ones(6)), 'rgb2imu'),
                     (dict(status=torch.zeros(3)), 'status'), (dict(status=None), 'status'), (dict(source=good['source'][:, :6]), 'source'),
                     (dict(flags=good['flags'][:1]), 'flags'), (dict(process_var=-1.0), 'process_var'), (dict(process_var=torch.ones(3)), 'process_var'),
                     (dict(depth_next=dn), 'depth_next'), (dict(var_next=vn), 'depth_next'), (dict(depth_next=dn[:, :6], var_next=vn), 'depth_next'),
                     (dict(grad_inv_depth=g[:1]), 'grad_inv_depth'), (dict(grad_var_inv_depth=g[:, :, :8]), 'grad_var_inv_depth')):
        with pytest.raises(ValueError, match=what):
            ops.dense_ba_depth_propagate_vjp(**dict(good, **kw))


def test_propagate_differentiable_argument_rules(monkeypatch):
    """propagate(differentiable=True) keeps the argument rules of the default path, refuses ``regularize`` with NotImplementedError
    before any launch, raises RuntimeError off the GPU, and hands ops._DenseBAPropagate the refinement's state, the uncertainty's
    variance and status, the stored mask, intrinsics and mount, process_var, the measurement with depth_next NOT detached and var_next
    detached, and the gate; depth and sigma_inv_depth are formed in torch from what it returns.  The default path calls
    ops.dense_ba_depth_propagate as before and never the Function."""
    from islam_amd import ops
    from islam_amd.dense_ba import DepthRegularizer
    from tests.test_depth_propagate_cpu import _cpu_loss, _cpu_state
    sc = make_scene(2, 7, 9, seed=1)
    loss = _cpu_loss(sc)
    joint, unc = _cpu_state(sc)
    dn = torch.from_numpy(sc['depth']).clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match='regularize'):
        loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, regularize=DepthRegularizer(), differentiable=True)
    with pytest.raises(RuntimeError, match='device tensors'):
        loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, differentiable=True)
    calls = []

    class Fake:
        @staticmethod
        def apply(*args):
            calls.append(args)
            rho = torch.full((2, 7, 9), 0.25, dtype=torch.float64)
            rho[0, 0, 0] = 0.0
            var = torch.full((2, 7, 9), 4e-4, dtype=torch.float64)
            var[0, 0, 0] = float('nan')
            return rho, var, torch.full((2, 7, 9), 7.0), None, None, None

    monkeypatch.setattr(ops, '_DenseBAPropagate', Fake)
    monkeypatch.setattr(ops, 'dense_ba_depth_propagate', lambda *a, **k: pytest.fail('the default path was taken'))
    out = loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, process_sigma=1e-3, gate=2.0, differentiable=True)
    rho, var, motion, intr, mask, status, mount, pv, dnext, vnext, gate = calls[-1]
    assert rho is joint.inv_depth and var is unc.var_inv_depth and motion is joint.motion and intr.tolist() == list(loss.K4)
    assert mask is loss.mask and status is unc.status and torch.equal(mount, torch.from_numpy(MOUNT)) and pv == 1e-3 * 1e-3 and gate == 2.0
    assert dnext.requires_grad and not vnext.requires_grad and vnext.dtype == torch.float32
    assert out.depth[0, 0, 0] == 7.0 and out.depth[1, 1, 1] == 4.0 and out.depth.dtype == torch.float32          # 1 / rho_f, else the kernel's bits
    assert torch.isnan(out.sigma_inv_depth[0, 0, 0]) and out.sigma_inv_depth[1, 1, 1] == 0.02
    n = len(calls)
    for kw, what in ((dict(depth_next=dn), 'come together'), (dict(sigma_inv_depth_next=0.02), 'come together'),
                     (dict(depth_next=dn[:, :6], sigma_inv_depth_next=0.02), 'depth_next'), (dict(depth_next=dn, sigma_inv_depth_next=0.0), 'sigma_inv_depth_next'),
                     (dict(process_sigma=-1.0), 'process_sigma')):
        with pytest.raises(ValueError, match=what):
            loss.propagate(joint, unc, differentiable=True, **kw)
    assert len(calls) == n


def test_default_path_does_not_use_the_function(monkeypatch):
    from islam_amd import ops
    from tests.test_depth_propagate_cpu import _cpu_loss, _cpu_state
    sc = make_scene(2, 7, 9, seed=1)
    loss = _cpu_loss(sc)
    joint, unc = _cpu_state(sc)
    dn = torch.from_numpy(sc['depth']).clone().requires_grad_(True)
    seen = []

    def fake(inv_depth, var_inv_depth, motion, intr, **kw):
        seen.append(kw)
        one = torch.ones(2, 7, 9, dtype=torch.float64)
        return ops.DenseBAPropagated(one, one, torch.ones(2, 7, 9), None, None, None)

    monkeypatch.setattr(ops, 'dense_ba_depth_propagate', fake)
    monkeypatch.setattr(ops._DenseBAPropagate, 'apply', staticmethod(lambda *a: pytest.fail('the Function was used')))
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02)
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, differentiable=False)
    assert len(seen) == 2 and not seen[0]['depth_next'].requires_grad and not seen[1]['depth_next'].requires_grad


# ------------------------------------------------------------------------------------------------ 5. the kernels' metadata
def test_new_kernels_have_no_private_segment_and_no_spill(lib):
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = _kernels()
    for want in ('depth_prop_vjp_kernel', 'depth_prop_pose_kernel'):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert not any(part in found[0] for part in ('dense_reproj', 'dense_ba', 'reproj_vjp', 'reproj_ift', 'joint_adj')), found[0]
        blk = ks[found[0]]
        print(want, 'vgpr', _field(blk, 'vgpr_count'), 'sgpr', _field(blk, 'sgpr_count'), 'lds', _field(blk, 'group_segment_fixed_size'))
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0 and _field(blk, 'sgpr_spill_count') == 0, want
