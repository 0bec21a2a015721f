"""The gradient of the depth regularisation (include/islam_hip.h, islam_depth_regularize_vjp): everything that
can be checked without a GPU -- the closed forms of tests/dense_ba_reg_grad_f64.py against torch.autograd on the float64 restatement
of the smooth pieces and against central differences of the forward restatement (tests/dense_ba_reg_f64.py), their structure (exact
zeros, the sum of the weights, NaN cotangents, links with a status, a hand-made table) -- and the host-side argument errors, the Python
plumbing and the register metadata of the three new kernels."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests import dense_ba_reg_grad_f64 as rg
from tests.dense_ba_prop_f64 import FLAG_GATED, FLAG_MEAS, FLAG_PROP, prop_case
from tests.dense_ba_reg_f64 import DEFAULTS, FLAG_FILLED, FLAG_REMOVED, compat, leak_scene, regularize_reference_link, shifted, window
from tests.dense_reproj_f64 import FEW, MOUNT, OK, U, make_scene

RADII2 = dict(DEFAULTS, occl_radius=2, fill_radius=2, smooth_radius=2, reg_gate=1.0, fill_min=2, fill_inflate=1.5)
NAMES = ('grad_inv_depth', 'grad_var_inv_depth', 'grad_depth_next', 'grad_var_next')


def _cotangents(shape, seed):
    """Random cotangents of rho_f and s_f; a variance is some 1e3 times smaller than an inverse depth, its cotangent that much larger."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), 1e3 * rng.standard_normal(shape)


def _leak_measurement():
    """A float32 measurement for the leak scene: the regularised map's own depth times (1 + 0.003 N(0,1)) with variance 1e-4, absent at
    every 7th pixel (NaN), at half the depth at every 11th (the gate at 3 refuses the map there), absent at every other hole that stays."""
    p = leak_scene()['pure']
    ref = regularize_reference_link(p['inv_depth'], p['var_inv_depth'], None, OK, 2.0 ** -12, **DEFAULTS)
    rng = np.random.default_rng(11)
    rho = np.where(ref['valid2'], ref['rho3'], 0.2) * (1.0 + 0.003 * rng.standard_normal(ref['rho3'].shape))
    idx = np.arange(rho.size).reshape(rho.shape)
    dn = (1.0 / rho).astype(np.float32)
    dn = np.where(idx % 11 == 5, np.float32(0.5) * dn, dn)
    dn = np.where((idx % 7 == 3) | (~ref['valid2'] & (idx % 2 == 0)), np.float32(np.nan), dn).astype(np.float32)
    return dn, np.full(rho.shape, 1e-4, np.float32)


def _scenes():
    """(label, pure maps of one link, dist_var, depth_next, var_next) of the leak scene, prop_case(1,7,9) and prop_case(3,24,40)."""
    dn, vn = _leak_measurement()
    yield 'leak', leak_scene()['pure'], 2.0 ** -12, dn, vn
    for shape, dv in (((1, 7, 9), (2.0 ** -12,)), ((3, 24, 40), (2.0 ** -14, 0.0, 3e-6))):
        sc, refs = prop_case(*shape)
        for b in range(shape[0]):
            yield '%dx%d link %d' % (shape[1], shape[2], b), refs['pure'][b], dv[b], sc['depth_next'][b], sc['var_next'][b]


def _reference(p, dv, dn, vn, gate, st, status=OK):
    return regularize_reference_link(p['inv_depth'], p['var_inv_depth'], None, status, dv, dn, vn, gate, **st)


# ------------------------------------------------------------------------------------------------ 1. closed forms against autograd
def test_closed_forms_match_autograd_of_the_restatement():
    """Every output of regularize_vjp_reference_link against torch.autograd.grad of the float64 restatement on the same fixed sets, at
    the defaults and at radii (2,2,2) with reg_gate 1, fill_min 2, fill_inflate 1.5, the measurement at gate 3, random cotangents:
    within 2^-52 K_AUTOGRAD of the element's scale (the float32 leaves add one float32 rounding of the value).  The restatement's
    forward values agree with regularize_reference_link's to 4 ulp.  Every row of the fusion table occurs and every stage removes,
    fills or moves something."""
    worst = dict.fromkeys(NAMES, 0.0)
    seen = np.zeros(8, int)
    for k, (label, p, dv, dn, vn) in enumerate(_scenes()):
        for cfg_name, st in (('defaults', DEFAULTS), ('radii 2', RADII2)):
            ref = _reference(p, dv, dn, vn, 3.0, st)
            H, W = ref['flags'].shape
            seen += np.bincount(ref['flags'].ravel() & 7, minlength=8)
            assert ref['removed'].any() and ref['filled'].any() and (ref['rho3'] != ref['rho2']).sum() > 10, (label, cfg_name)
            gr, gs = _cotangents((H, W), 50 + k)
            cf = rg.regularize_vjp_reference_link(ref, ref['flags'], dv, dn, vn, gr, gs, **st)
            v0 = ref['valid0']
            leaf = lambda a, dt: torch.tensor(np.ascontiguousarray(a, dt), requires_grad=True)
            ins = [leaf(np.where(v0, p['inv_depth'], 1.0), np.float64), leaf(np.where(v0, p['var_inv_depth'], 1.0), np.float64), leaf(dn, np.float32),
                   leaf(vn, np.float32)]
            rf, sf = rg.regularize_torch_link(ins[0], ins[1], ref, ref['flags'], dv, ins[2], ins[3], **st)
            known = (ref['flags'] & 3) != 0
            for got, want in ((rf, ref['inv_depth']), (sf, ref['var_inv_depth'])):
                assert (np.abs(got.detach().numpy() - want)[known] <= 4 * U * np.abs(want[known])).all(), (label, cfg_name)
            sel = torch.from_numpy(known)
            L = (torch.from_numpy(gr) * rf)[sel].sum() + (torch.from_numpy(gs) * sf)[sel].sum()
            grads = torch.autograd.grad(L, ins)
            for name, g in zip(NAMES, grads):
                g = g.numpy().astype(np.float64)
                assert np.isfinite(g).all() and np.isfinite(cf[name]).all() and (cf[name] != 0).sum() >= 7
                extra = rg.U24 * np.abs(cf[name]) + 2.0 ** -149 if name in NAMES[2:] else None
                s = rg.share('%s, %s, %s' % (label, cfg_name, name), cf[name], g, cf['scale' + name[4:]], rg.K_AUTOGRAD, extra)
                worst[name] = max(worst[name], s)
                assert s <= 1.0, (label, cfg_name, name, s)
            off = ~cf['valid1']
            assert (cf['grad_inv_depth'][off] == 0).all() and (cf['grad_var_inv_depth'][off] == 0).all()
            assert (grads[0].numpy()[off] == 0).all() and (grads[1].numpy()[off] == 0).all()
    print('worst share of the bound:', {k: round(v, 4) for k, v in worst.items()})
    assert (seen[[0, FLAG_PROP, FLAG_MEAS, FLAG_PROP | FLAG_MEAS, 7]] > 0).all() and seen[[4, 5, 6]].sum() == 0


# ------------------------------------------------------------------------------------------------ 2. closed forms against central differences
def compat_margin(ref, rho, var, st):
    """The smallest relative distance of a compat quotient (rho_k - rho_j)^2 / (reg_gate^2 (s_k + s_j)) to 1 over every pair a stage may
    test: valid0 pairs within max(occl_radius, 2 fill_radius) on the input, valid2 pairs within smooth_radius on stage-2 values."""
    g2 = st['reg_gate'] ** 2
    m = np.inf
    for r_, s_, valid, r in ((rho, var, ref['valid0'], max(st['occl_radius'], 2 * st['fill_radius'])), (ref['rho2'], ref['var2'], ref['valid2'], st['smooth_radius'])):
        r_, s_ = np.where(valid, r_, 1.0), np.where(valid, s_, 1.0)
        for dv, du in window(r):
            if (dv, du) == (0, 0):
                continue
            pair = valid & shifted(valid, dv, du, False)
            q = (shifted(r_, dv, du, 1.0) - r_) ** 2 / (g2 * (shifted(s_, dv, du, 1.0) + s_))
            if pair.any():
                m = min(m, float(np.abs(q[pair] - 1.0).min()))
    return m


def anchor_gap(ref, st):
    """The smallest relative gap between the two largest valid1 rho in the window of a filled pixel (inf where a window holds one)."""
    valid1 = ref['valid0'] & ~ref['removed']
    gap = np.inf
    for v, u in np.argwhere(ref['filled']):
        vals = sorted((ref['rho2'][v + dv, u + du] for dv, du in window(st['fill_radius'])
                       if 0 <= v + dv < valid1.shape[0] and 0 <= u + du < valid1.shape[1] and valid1[v + dv, u + du]), reverse=True)
        if len(vals) > 1:
            gap = min(gap, (vals[0] - vals[1]) / vals[0])
    return gap


def gate_margin(ref, dn, vn, gate):
    """The smallest relative distance of (rho3 - rho_m)^2 / (gate^2 (s2 + s_m)) to 1 where the map and the measurement meet."""
    both = ((ref['flags'] & 3) == 3)
    rm, sm = 1.0 / np.where(both, dn, 1.0).astype(np.float64), np.where(both, vn, 1.0).astype(np.float64)
    q = (ref['rho3'] - rm) ** 2 / (gate * gate * (ref['var2'] + sm))
    return float(np.abs(q[both] - 1.0).min())


def _binade_step(x, shift):
    """2^(floor(log2 x) - shift) where x is finite and > 0, else 0: a step that keeps a float32 value exactly representable."""
    ok = np.isfinite(x) & (x > 0)
    return np.where(ok, np.exp2(np.floor(np.log2(np.where(ok, x, 1.0).astype(np.float64))) - shift), 0.0)


def test_closed_forms_match_central_differences_of_the_forward_restatement():
    """Directional derivatives of f = sum cr rho_f + cs s_f (where something is known) by central differences of the existing
    regularize_reference_link on the leak scene with the measurement of _leak_measurement at gate 3, in one random direction per
    input (rho, s, depth_next, var_next) and one through all four, at two step sizes: at most 2^-23 relative in rho and 2^-13 in s,
    2^-16 and 2^-12 of a value's binade in depth_next and var_next (the float32 maps hold the perturbed values exactly, asserted), and
    half of each.  What makes the sets hold still (asserted): every compat quotient is further than 0.5 from 1 (relative; measured
    0.99), the two largest rho of a hole's window differ by more than 2^-21 (relative), the gate quotient is further than 1e-2 from
    1; flags and the removed and filled sets are identical at +h and -h, which is asserted and not skipped on.  The bound is section
    3.31's: twice the truncation estimate |D(h) - D(h/2)| / 3 plus the rounding of f(+) - f(-), 64 x 2^-52 sum |c out|."""
    label, p, dv, dn, vn = next(_scenes())
    st = DEFAULTS
    ref = _reference(p, dv, dn, vn, 3.0, st)
    v0 = ref['valid0']
    cm, ag, gm = compat_margin(ref, p['inv_depth'], p['var_inv_depth'], st), anchor_gap(ref, st), gate_margin(ref, dn, vn, 3.0)
    print('compat margin %.3f, anchor gap %.3e, gate margin %.3e' % (cm, ag, gm))
    assert cm > 0.5 and ag > 2.0 ** -21 and gm > 1e-2
    assert (np.bincount(ref['flags'].ravel() & 7, minlength=8)[[0, 1, 2, 3, 7]] > 0).all() and ref['removed'].any() and ref['filled'].any()
    gr, gs = _cotangents(v0.shape, 70)
    cf = rg.regularize_vjp_reference_link(ref, ref['flags'], dv, dn, vn, gr, gs, **st)
    known = (ref['flags'] & 3) != 0
    f = lambda r: float((gr * r['inv_depth'])[known].sum() + (gs * r['var_inv_depth'])[known].sum())
    S = float(np.abs(gr * ref['inv_depth'])[known].sum() + np.abs(gs * ref['var_inv_depth'])[known].sum())
    rng = np.random.default_rng(90)
    shape = v0.shape
    amp = lambda: rng.choice([-1.0, 1.0], shape) * rng.uniform(0.5, 1.0, shape)
    x0 = dict(rho=np.where(v0, p['inv_depth'], 0.0), var=np.where(v0, p['var_inv_depth'], np.nan), depth_next=dn.astype(np.float64), var_next=vn.astype(np.float64))
    unit = dict(rho=2.0 ** -23 * x0['rho'] * amp(), var=2.0 ** -13 * np.where(v0, p['var_inv_depth'], 0.0) * amp(),
                depth_next=rng.choice([-1.0, 1.0], shape) * _binade_step(dn, 16), var_next=rng.choice([-1.0, 1.0], shape) * _binade_step(vn, 12))
    keys = dict(rho='grad_inv_depth', var='grad_var_inv_depth', depth_next='grad_depth_next', var_next='grad_var_next')
    for which in list(unit) + ['all']:
        quot = []
        for half in (1.0, 0.5):
            at = []
            for sgn in (1.0, -1.0):
                x = {name: (x0[name] + sgn * half * unit[name] if which in (name, 'all') else x0[name]) for name in x0}
                for name in ('depth_next', 'var_next'):          # the float32 maps hold the perturbed values exactly
                    as32 = x[name].astype(np.float32)
                    assert np.array_equal(as32.astype(np.float64), x[name], equal_nan=True), name
                    x[name] = as32
                r = regularize_reference_link(x['rho'], x['var'], None, OK, dv, x['depth_next'], x['var_next'], 3.0, **st)
                assert np.array_equal(r['flags'], ref['flags']) and np.array_equal(r['removed'], ref['removed']) and np.array_equal(r['filled'], ref['filled'])
                at.append((f(r), x))
            step = {name: np.nan_to_num(0.5 * (np.asarray(at[0][1][name], np.float64) - np.asarray(at[1][1][name], np.float64)), nan=0.0) for name in x0}
            want = sum(float(np.sum(cf[keys[name]] * step[name])) for name in x0)
            quot.append((0.5 * (at[0][0] - at[1][0]), want))
        d_big, d_small, want = 0.5 * quot[0][0], quot[1][0], quot[1][1]
        bound = 2.0 * abs(d_big - d_small) / 3.0 + 64.0 * U * S
        print('%s, %s: closed form %.9e, quotient %.9e, difference %.2e, bound %.2e' % (label, which, want, d_small, abs(want - d_small), bound))
        assert want != 0.0 and abs(want - d_small) <= bound, which
        assert bound <= 1e-2 * abs(want), which          # the quotient resolves the derivative: the check is not vacuous


# ------------------------------------------------------------------------------------------------ 3. structure
def test_exact_zeros_weight_sums_and_identity():
    """Exact zeros at holes, removed, refilled and non-finite inputs; with a cotangent on rho_f alone and no measurement the sum of
    grad_inv_depth equals the sum of the cotangent over the present pixels (every stage is a mean with weights summing to 1) within
    2^-52 K_DEVICE of the summed scales; radii (0,0,0) without a measurement give the cotangents back bit for bit at present pixels."""
    refilled = 0
    for k, (label, p, dv, dn, vn) in enumerate(_scenes()):
        for st in (DEFAULTS, RADII2):
            ref = _reference(p, dv, None, None, 0.0, st)
            gr, gs = _cotangents(ref['flags'].shape, 150 + k)
            cf = rg.regularize_vjp_reference_link(ref, ref['flags'], dv, None, None, gr, gs, **st)
            assert cf['grad_depth_next'] is None and cf['grad_var_next'] is None
            valid1 = ref['valid0'] & ~ref['removed']
            for name in NAMES[:2]:
                assert (cf[name][~valid1] == 0).all() and (cf[name][ref['removed']] == 0).all() and (cf[name][ref['filled']] == 0).all(), (label, name)
                assert np.isfinite(cf[name]).all()
            refilled += int((ref['removed'] & ref['filled']).sum())
            only = rg.regularize_vjp_reference_link(ref, ref['flags'], dv, None, None, gr, None, **st)
            present = (ref['flags'] & FLAG_PROP) != 0
            total, want = float(only['grad_inv_depth'].sum()), float(gr[present].sum())
            bound = rg.U52 * rg.K_DEVICE * float(only['scale_inv_depth'].sum() + np.abs(gr[present]).sum())
            print('%s: sum of grad_inv_depth %.12f, of the cotangent %.12f, difference %.1e, bound %.1e' % (label, total, want, abs(total - want), bound))
            assert abs(total - want) <= bound, label
        st0 = dict(DEFAULTS, occl_radius=0, fill_radius=0, smooth_radius=0)
        ref = _reference(p, dv, None, None, 0.0, st0)
        cf = rg.regularize_vjp_reference_link(ref, ref['flags'], dv, None, None, gr, gs, **st0)
        present = (ref['flags'] & FLAG_PROP) != 0
        assert np.array_equal(present, ref['valid0']) and np.array_equal(cf['grad_inv_depth'][present], gr[present])
        assert np.array_equal(cf['grad_var_inv_depth'][present], gs[present]) and not cf['grad_inv_depth'][~present].any()
    assert refilled > 0


def test_nan_cotangents_and_links_with_a_status():
    """NaN cotangents where (flags & 3) == 0 give finite results equal to those with zeros there.  A link with a status, and one with
    dist_var -1 or NaN, gets zeros on the state and the measured-only row on the measurement."""
    for k, (label, p, dv, dn, vn) in enumerate(_scenes()):
        ref = _reference(p, dv, dn, vn, 3.0, DEFAULTS)
        gr, gs = _cotangents(ref['flags'].shape, 110 + k)
        nothing = (ref['flags'] & 3) == 0
        assert nothing.any(), label
        zero = rg.regularize_vjp_reference_link(ref, ref['flags'], dv, dn, vn, np.where(nothing, 0.0, gr), np.where(nothing, 0.0, gs), **DEFAULTS)
        nan = rg.regularize_vjp_reference_link(ref, ref['flags'], dv, dn, vn, np.where(nothing, np.nan, gr), np.where(nothing, np.nan, gs), **DEFAULTS)
        for name in NAMES:
            assert np.isfinite(nan[name]).all() and np.array_equal(nan[name], zero[name]), (label, name)
        alone = ((ref['flags'] & 7) == FLAG_MEAS) | ((ref['flags'] & FLAG_GATED) != 0)
        rm = 1.0 / dn.astype(np.float64)[alone]
        assert np.array_equal(nan['grad_depth_next'][alone], -(rm * rm) * gr[alone]) and np.array_equal(nan['grad_var_next'][alone], gs[alone])
        for status, dist in ((FEW, dv), (OK, -1.0), (OK, np.nan)):
            st = _reference(p, dist, dn, vn, 3.0, DEFAULTS, status=status)
            assert st['status'] != OK
            got = rg.regularize_vjp_reference_link(st, st['flags'], dist, dn, vn, gr, gs, **DEFAULTS)
            assert not got['grad_inv_depth'].any() and not got['grad_var_inv_depth'].any()
            present = st['flags'] == FLAG_MEAS
            rm = 1.0 / dn.astype(np.float64)[present]
            assert np.array_equal(got['grad_depth_next'][present], -(rm * rm) * gr[present]) and (got['grad_depth_next'][~present] == 0).all()
            assert np.array_equal(got['grad_var_next'][present], gs[present]) and (got['grad_var_next'][~present] == 0).all()


def test_hand_made_table_of_one_hole():
    """A 5 x 5 map: one hole in the middle, three neighbours of different variances, nothing else; fill_radius 1, fill_min 3,
    fill_inflate 2.5, no removal, no smoothing.  The four partial derivatives of the filled value from the header's formulas."""
    rho, var = np.full((5, 5), np.nan), np.full((5, 5), np.nan)
    cells = [((1, 1), 0.50, 1e-4), ((2, 3), 0.51, 4e-4), ((3, 2), 0.49, 2.5e-4)]
    for (v, u), r, s in cells:
        rho[v, u], var[v, u] = r, s
    st = dict(DEFAULTS, occl_radius=0, fill_radius=1, fill_min=3, fill_inflate=2.5, smooth_radius=0)
    ref = regularize_reference_link(rho, var, None, OK, 0.0, **st)
    assert ref['filled'].sum() >= 1 and ref['filled'][2, 2]
    w = np.array([1.0 / s for _, _, s in cells])
    r = np.array([r for _, r, _ in cells])
    S = w.sum()
    mean = (w * r).sum() / S
    e = r - mean
    s2 = 2.5 * (3 + (w * e * e).sum()) / S
    assert abs(ref['rho2'][2, 2] - mean) <= 4 * U * mean and abs(ref['var2'][2, 2] - s2) <= 8 * U * s2
    one = np.zeros((5, 5))
    one[2, 2] = 1.0
    on_rho = rg.regularize_vjp_reference_link(ref, ref['flags'], 0.0, None, None, one, None, **st)
    on_var = rg.regularize_vjp_reference_link(ref, ref['flags'], 0.0, None, None, None, one, **st)
    for i, ((v, u), _, _) in enumerate(cells):
        for got, want in ((on_rho['grad_inv_depth'][v, u], w[i] / S), (on_rho['grad_var_inv_depth'][v, u], -w[i] ** 2 * e[i] / S),
                          (on_var['grad_inv_depth'][v, u], 2 * 2.5 * w[i] * e[i] / S), (on_var['grad_var_inv_depth'][v, u], w[i] ** 2 * (s2 - 2.5 * e[i] ** 2) / S)):
            assert abs(got - want) <= 64 * U * abs(want) and want != 0, (i, got, want)
    assert on_rho['n_fill_terms'] >= 3 and on_rho['grad_inv_depth'][2, 2] == 0


# ------------------------------------------------------------------------------------------------ 4. error paths and plumbing
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_exported_and_bound(lib):
    from islam_amd import _lib, dense_ba, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'islam_hip.h')).read()
    for name in ('islam_depth_regularize_vjp_scratch_bytes', 'islam_depth_regularize_vjp'):
        assert name in _lib.SIGNATURES and hasattr(lib._cdll, name), name
        assert name + '(' in header
    assert callable(ops.dense_ba_depth_regularize_vjp) and issubclass(ops._DenseBARegularize, torch.autograd.Function)
    assert ops.DenseBARegularizeGrad._fields == NAMES
    assert inspect.signature(dense_ba.DenseReprojectionLoss.propagate).parameters['regularize_grad'].default is None
    assert dense_ba.DepthRegularizer()._asdict() == dict(DEFAULTS, dist_sigma=0.0)          # the record itself does not change
    f = lib.islam_depth_regularize_vjp_scratch_bytes
    n = 3 * 24 * 40
    assert f(0, 24, 40) == 0 and f(3, 0, 40) == 0 and f(3, 24, -1) == 0 and 89 * n <= f(3, 24, 40) < 89 * n + 12 * 256


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    one = 1        # any non-NULL address: a refused call never reads it

    def call(B=1, H=2, W=2, rho=one, var=one, dist=one, dn=None, vn=None, gate=0.0, r1=1, occl_min=2, r2=1, fill_min=3, inflate=1.0, r3=1, reg_gate=3.0,
             fl=one, g1=None, g2=None, o1=one, o2=one, o3=None, o4=None, scratch=one):
        return lib.islam_depth_regularize_vjp(rho, var, None, dist, dn, vn, gate, r1, occl_min, r2, fill_min, inflate, r3, reg_gate, fl, g1, g2, o1, o2, o3, o4,
                                              scratch, B, H, W, None)

    nan, inf = float('nan'), float('inf')
    cases = [(dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
             (dict(dn=one), b'depth_next and var_next'), (dict(vn=one), b'depth_next and var_next'),
             (dict(dn=one, vn=one, o3=one), b'grad_depth_next and grad_var_next'), (dict(dn=one, vn=one, o4=one), b'grad_depth_next and grad_var_next'),
             (dict(o3=one, o4=one), b'without a measurement'),
             (dict(gate=-1.0), b'gate'), (dict(gate=nan), b'gate'), (dict(gate=inf), b'gate'),
             (dict(r1=-1), b'radius'), (dict(r1=3), b'radius'), (dict(r2=3), b'radius'), (dict(r2=-1), b'radius'), (dict(r3=3), b'radius'),
             (dict(r3=-2), b'radius'), (dict(occl_min=0), b'occl_min'), (dict(fill_min=0), b'fill_min'), (dict(inflate=0.5), b'fill_inflate'),
             (dict(inflate=nan), b'fill_inflate'), (dict(inflate=inf), b'fill_inflate'), (dict(reg_gate=0.0), b'reg_gate'),
             (dict(reg_gate=-1.0), b'reg_gate'), (dict(reg_gate=nan), b'reg_gate'), (dict(reg_gate=inf), b'reg_gate')]
    cases += [({k: None}, b'NULL') for k in ('rho', 'var', 'dist', 'fl', 'o1', 'o2', 'scratch')]
    for kw, what in cases:
        assert call(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_depth_regularize_vjp' in msg and what in msg, (kw, msg)


def test_op_refuses_cpu_tensors_and_bad_arguments():
    """Off the GPU the op raises RuntimeError (there is no CPU path), after its argument rules, which raise ValueError."""
    from islam_amd import ops
    rho, var = torch.full((2, 7, 9), 0.25, dtype=torch.float64), torch.full((2, 7, 9), 1e-4, dtype=torch.float64)
    good = dict(inv_depth=rho, var_inv_depth=var, flags=torch.ones(2, 7, 9, dtype=torch.uint8))
    dn, vn, g = torch.full((2, 7, 9), 4.0), torch.full((2, 7, 9), 4e-4), torch.zeros(2, 7, 9, dtype=torch.float64)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_regularize_vjp(**good)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_regularize_vjp(**good, status=torch.zeros(2, dtype=torch.int32), grad_inv_depth=g, grad_var_inv_depth=g,
                                          dist_var=torch.tensor([1e-6, 2e-6]), depth_next=dn, var_next=vn, gate=3.0, occl_radius=2, occl_min=1,
                                          fill_radius=0, fill_min=2, fill_inflate=2.0, smooth_radius=2, reg_gate=2.0)
    for kw, what in ((dict(var_inv_depth=var[:, :6]), 'var_inv_depth'), (dict(inv_depth=rho[0], var_inv_depth=var[0]), 'inv_depth'),
                     (dict(flags=good['flags'][:1]), 'flags'), (dict(flags=None), 'flags'), (dict(status=torch.zeros(3)), 'status'),
                     (dict(grad_inv_depth=g[:1]), 'grad_inv_depth'), (dict(grad_var_inv_depth=g[:, :, :8]), 'grad_var_inv_depth'),
                     (dict(dist_var=-1.0), 'dist_var'), (dict(dist_var=float('nan')), 'dist_var'), (dict(dist_var=torch.tensor([1e-6, -1.0])), 'dist_var'),
                     (dict(dist_var=torch.ones(3)), 'dist_var'), (dict(depth_next=dn), 'depth_next'), (dict(var_next=vn), 'depth_next'),
                     (dict(depth_next=dn[:, :6], var_next=vn), 'depth_next'), (dict(depth_next=dn, var_next=vn, gate=-1.0), 'gate'),
                     (dict(gate=float('inf')), 'gate'), (dict(occl_radius=3), 'radius'), (dict(fill_radius=-1), 'radius'), (dict(smooth_radius=1.5), 'radius'),
                     (dict(occl_min=0), 'occl_min'), (dict(fill_min=0), 'fill_min'), (dict(fill_min=2.5), 'fill_min'), (dict(fill_inflate=0.9), 'fill_inflate'),
                     (dict(fill_inflate=float('nan')), 'fill_inflate'), (dict(reg_gate=0.0), 'reg_gate'), (dict(reg_gate=float('inf')), 'reg_gate')):
        with pytest.raises(ValueError, match=what):
            ops.dense_ba_depth_regularize_vjp(**dict(good, **kw))


def test_propagate_regularize_grad_rules(monkeypatch):
    """propagate(differentiable=True, regularize=DepthRegularizer(...), regularize_grad='piecewise') sends the pure propagation through
    ops._DenseBAPropagate without a measurement at gate 0, then its maps, source and status through ops._DenseBARegularize with
    dist_var = dist_sigma^2, the measurement (depth_next NOT detached, var_next detached), ``gate`` and the record's stages; depth and
    sigma_inv_depth are formed in torch from what that returns.  Without the keyword the call still raises NotImplementedError, now
    pointing to it; any other value, and 'piecewise' without both differentiable=True and a regulariser, is a ValueError; the default
    paths never touch the new Function."""
    from islam_amd import ops
    from islam_amd.dense_ba import DepthRegularizer
    from tests.test_depth_propagate_cpu import _cpu_loss, _cpu_state
    sc = make_scene(2, 7, 9, seed=1)
    loss = _cpu_loss(sc)
    joint, unc = _cpu_state(sc)
    dn = torch.from_numpy(sc['depth']).clone().requires_grad_(True)
    meas = dict(depth_next=dn, sigma_inv_depth_next=0.02)
    with pytest.raises(NotImplementedError, match='regularize') as info:
        loss.propagate(joint, unc, **meas, regularize=DepthRegularizer(), differentiable=True)
    assert "regularize_grad='piecewise'" in str(info.value)
    for kw in (dict(regularize_grad='soft', differentiable=True, regularize=DepthRegularizer()), dict(regularize_grad=True, differentiable=True, regularize=DepthRegularizer()),
               dict(regularize_grad='piecewise'), dict(regularize_grad='piecewise', differentiable=True), dict(regularize_grad='piecewise', regularize=DepthRegularizer())):
        with pytest.raises(ValueError, match='regularize_grad'):
            loss.propagate(joint, unc, **meas, **kw)
    with pytest.raises(ValueError, match='DepthRegularizer'):
        loss.propagate(joint, unc, **meas, regularize=dict(DEFAULTS), differentiable=True, regularize_grad='piecewise')
    with pytest.raises(RuntimeError, match='device tensors'):
        loss.propagate(joint, unc, **meas, regularize=DepthRegularizer(), differentiable=True, regularize_grad='piecewise')
    calls = []
    src, st = torch.zeros(2, 7, 9, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)

    def fake(tag, value):
        class Fake:
            @staticmethod
            def apply(*args):
                calls.append((tag, args))
                rho = torch.full((2, 7, 9), 0.25, dtype=torch.float64)
                rho[0, 0, 0] = 0.0
                var = torch.full((2, 7, 9), value, dtype=torch.float64)
                var[0, 0, 0] = float('nan')
                return rho, var, torch.full((2, 7, 9), 7.0), src, torch.ones(2, 7, 9, dtype=torch.uint8), st
        return Fake

    monkeypatch.setattr(ops, '_DenseBAPropagate', fake('propagate', 1e-4))
    monkeypatch.setattr(ops, '_DenseBARegularize', fake('regularize', 4e-4))
    monkeypatch.setattr(ops, 'dense_ba_depth_propagate', lambda *a, **k: pytest.fail('the default path was taken'))
    monkeypatch.setattr(ops, 'dense_ba_depth_regularize', lambda *a, **k: pytest.fail('the default path was taken'))
    cfg = DepthRegularizer(occl_radius=2, fill_min=2, fill_inflate=1.5, dist_sigma=2e-3)
    out = loss.propagate(joint, unc, **meas, process_sigma=1e-3, gate=2.0, regularize=cfg, differentiable=True, regularize_grad='piecewise')
    assert [c[0] for c in calls] == ['propagate', 'regularize']
    rho, var, motion, intr, mask, status, mount, pv, dnext, vnext, gate = calls[0][1]
    assert rho is joint.inv_depth and var is unc.var_inv_depth and motion is joint.motion and intr.tolist() == list(loss.K4)
    assert mask is loss.mask and status is unc.status and torch.equal(mount, torch.from_numpy(MOUNT)) and pv == 1e-3 * 1e-3
    assert dnext is None and vnext is None and gate == 0.0
    prho, pvar, psrc, pst, dist_var, dnext, vnext, gate, stages = calls[1][1]
    assert prho[1, 1, 1] == 0.25 and pvar[1, 1, 1] == 1e-4 and psrc is src and pst is st and dist_var == 2e-3 * 2e-3 and gate == 2.0
    assert dnext.requires_grad and not vnext.requires_grad and vnext.dtype == torch.float32
    assert stages == dict(DEFAULTS, occl_radius=2, fill_min=2, fill_inflate=1.5)
    assert type(out).__name__ == 'DenseBAPrior' and out.depth[0, 0, 0] == 7.0 and out.depth[1, 1, 1] == 4.0 and out.depth.dtype == torch.float32
    assert torch.isnan(out.sigma_inv_depth[0, 0, 0]) and out.sigma_inv_depth[1, 1, 1] == 0.02 and out.source is src and out.status is st
    # without a regulariser the differentiable path is the one of section 3.31: one Function, the measurement in it
    del calls[:]
    loss.propagate(joint, unc, **meas, differentiable=True)
    assert [c[0] for c in calls] == ['propagate'] and calls[0][1][8] is dn and calls[0][1][10] == 3.0


def test_default_paths_do_not_use_the_function(monkeypatch):
    from islam_amd import ops
    from islam_amd.dense_ba import DepthRegularizer
    from tests.test_depth_propagate_cpu import _cpu_loss, _cpu_state
    sc = make_scene(2, 7, 9, seed=1)
    loss = _cpu_loss(sc)
    joint, unc = _cpu_state(sc)
    dn = torch.from_numpy(sc['depth'])
    seen = []
    maps = lambda: (torch.ones(2, 7, 9, dtype=torch.float64), torch.ones(2, 7, 9, dtype=torch.float64), torch.ones(2, 7, 9), None, None, None)
    monkeypatch.setattr(ops, 'dense_ba_depth_propagate', lambda *a, **k: seen.append('propagate') or ops.DenseBAPropagated(*maps()))
    monkeypatch.setattr(ops, 'dense_ba_depth_regularize', lambda *a, **k: seen.append('regularize') or ops.DenseBARegularized(*maps()))
    monkeypatch.setattr(ops._DenseBARegularize, 'apply', staticmethod(lambda *a: pytest.fail('the Function was used')))
    monkeypatch.setattr(ops._DenseBAPropagate, 'apply', staticmethod(lambda *a: pytest.fail('the Function was used')))
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02)
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, regularize=DepthRegularizer())
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, regularize=DepthRegularizer(), differentiable=False, regularize_grad=None)
    assert seen == ['propagate', 'propagate', 'regularize', 'propagate', 'regularize']


# ------------------------------------------------------------------------------------------------ 5. the kernels' metadata
def test_new_kernels_have_no_private_segment_and_no_spill(lib):
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = _kernels()
    counted = ('dense_reproj', 'dense_ba', 'reproj_vjp', 'reproj_ift', 'joint_adj', 'depth_regularize_kernel', 'depth_splat_kernel', 'depth_fuse_kernel',
               'depth_prop_vjp_kernel', 'depth_prop_pose_kernel')
    for want in ('depth_reg_front_kernel', 'depth_reg_smooth_adj_kernel', 'depth_reg_fill_adj_kernel'):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert not any(part in found[0] for part in counted), found[0]
        blk = ks[found[0]]
        print(want, 'vgpr', _field(blk, 'vgpr_count'), 'sgpr', _field(blk, 'sgpr_count'), 'lds', _field(blk, 'group_segment_fixed_size'))
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0 and _field(blk, 'sgpr_spill_count') == 0, want
        assert _field(blk, 'group_segment_fixed_size') <= 32 * 1024
    assert len([n for n in ks if 'depth_regularize_kernel' in n]) == 1          # the forward is still one kernel under that name
