"""Regularisation of a propagated inverse-depth map (include/islam_hip.h, islam_depth_regularize): everything
about the float64 numpy restatement (tests/dense_ba_reg_f64.py) that can be checked without a GPU -- the three stencil stages against a
scalar brute force, hand-made 5 x 5 tables for every rule of the definition, the symmetry of the smoothing weights, the planted scene in
which background leaks through a magnified patch, the recursive filter on a plane with and without the stages -- and the host-side
argument errors, the Python plumbing and the register metadata of the new kernel."""
import math
import os

import numpy as np
import pytest
import torch

from tests import dense_ba_prop_f64 as prop
from tests import dense_ba_reg_f64 as reg
from tests.dense_ba_prop_f64 import FLAG_GATED, FLAG_MEAS, FLAG_PROP, filter_reference, fuse_pixel, prop_case, scene_margins
from tests.dense_ba_reg_f64 import DEFAULTS, FLAG_FILLED, FLAG_REMOVED, filter_reference_reg, leak_counts, leak_scene, regularize_reference_link
from tests.dense_reproj_f64 import BADPRIOR, FEW, MOUNT, OK, make_scene


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ 1. a scalar brute force
def _brute_force(rho, var, dist_var, r1, occl_min, r2, fill_min, inflate, r3, g):
    """The three stages pixel by pixel in Python floats, with the window's bounds clipped by hand and lists of neighbours instead of
    shifted maps: (removed, filled, rho2, var2, rho3) as nested lists; a pixel without a value holds None."""
    H, W = rho.shape
    g2 = g * g
    val = [[(float(rho[v, u]), float(var[v, u])) if math.isfinite(rho[v, u]) and rho[v, u] > 0 and math.isfinite(var[v, u]) and var[v, u] > 0
            else None for u in range(W)] for v in range(H)]

    def nbrs(state, v, u, r):          # row-major, clipped
        return [(vv, uu, state[vv][uu]) for vv in range(max(0, v - r), min(H, v + r + 1)) for uu in range(max(0, u - r), min(W, u + r + 1))
                if state[vv][uu] is not None]

    ok = lambda a, b: (a[0] - b[0]) * (a[0] - b[0]) <= g2 * (a[1] + b[1])
    removed = [[False] * W for _ in range(H)]
    for v in range(H):
        for u in range(W):
            if val[v][u] is None or r1 == 0:
                continue
            others = [x for vv, uu, x in nbrs(val, v, u, r1) if (vv, uu) != (v, u)]
            n_sup = len([x for x in others if ok(x, val[v][u])])
            n_occ = len([x for x in others if not ok(x, val[v][u]) and x[0] > val[v][u][0]])
            removed[v][u] = n_occ >= occl_min and n_occ > n_sup
    one = [[None if removed[v][u] else val[v][u] for u in range(W)] for v in range(H)]
    two = [row[:] for row in one]
    filled = [[False] * W for _ in range(H)]
    for v in range(H):
        for u in range(W):
            if one[v][u] is not None or r2 == 0:
                continue
            C = [x for _, _, x in nbrs(one, v, u, r2)]
            if not C:
                continue
            a = C[0]
            for x in C[1:]:
                if x[0] > a[0]:
                    a = x
            cluster = [x for x in C if ok(x, a)]
            if len(cluster) < fill_min:
                continue
            Sw = Swr = 0.0
            for x in cluster:
                Sw, Swr = Sw + 1.0 / x[1], Swr + (1.0 / x[1]) * x[0]
            mean, Se = Swr / Sw, 0.0
            for x in cluster:
                Se = Se + (1.0 / x[1]) * ((x[0] - mean) * (x[0] - mean))
            two[v][u], filled[v][u] = (mean, inflate * (len(cluster) / Sw + Se / Sw)), True
    three = [[None if x is None else x[0] for x in row] for row in two]
    for v in range(H):
        for u in range(W):
            if two[v][u] is None or r3 == 0:
                continue
            Sw = Swr = 0.0
            for vv, uu, x in nbrs(two, v, u, r3):
                if ok(x, two[v][u]):
                    w = 1.0 / (x[1] + dist_var * float((uu - u) ** 2 + (vv - v) ** 2))
                    Sw, Swr = Sw + w, Swr + w * x[0]
            three[v][u] = Swr / Sw
    return removed, filled, two, three


@pytest.mark.parametrize('cfg', [dict(DEFAULTS), dict(DEFAULTS, occl_radius=2, fill_radius=2, smooth_radius=2, fill_min=2, reg_gate=1.0, fill_inflate=1.5),
                                 dict(DEFAULTS, occl_radius=1, occl_min=1, fill_radius=2, fill_min=1, smooth_radius=1, reg_gate=0.5)])
def test_restatement_matches_a_scalar_brute_force(cfg):
    """The 7 x 9 scene's pure propagation (large motion: holes and several surfaces side by side): every stage of the restatement equals a
    pixel-by-pixel loop in Python floats that clips its windows by hand -- which pixels are removed and filled, and the bits of rho and s
    after stages 2 and 3 (both sides run the definition's operations in the definition's order)."""
    p = prop_case(1, 7, 9)[1]['pure'][0]
    dist_var = 2.0 ** -12
    r = regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], dist_var=dist_var, **cfg)
    removed, filled, two, three = _brute_force(p['inv_depth'], p['var_inv_depth'], dist_var, cfg['occl_radius'], cfg['occl_min'], cfg['fill_radius'],
                                               cfg['fill_min'], cfg['fill_inflate'], cfg['smooth_radius'], cfg['reg_gate'])
    assert np.array_equal(r['removed'], np.array(removed)) and np.array_equal(r['filled'], np.array(filled))
    have = np.array([[x is not None for x in row] for row in two])
    assert np.array_equal(r['valid2'], have) and np.array_equal(r['valid0'], p['source'] >= 0)
    pick = lambda rows, k: np.array([[1.0 if x is None else (x if k is None else x[k]) for x in row] for row in rows])
    assert np.array_equal(_bits(r['rho2']), _bits(pick(two, 0))) and np.array_equal(_bits(r['var2']), _bits(pick(two, 1)))
    assert np.array_equal(_bits(r['rho3']), _bits(pick(three, None)))
    print('removed %d, filled %d of %d holes, %d values' % (r['removed'].sum(), r['filled'].sum(), (~r['valid0']).sum(), have.sum()))
    assert r['filled'].sum() >= 5 and (cfg['reg_gate'] == 3.0 or r['removed'].sum() >= 1)
    # without a measurement the outputs are the stages' values, 0 and NaN where nothing is known, and the flags say what happened
    assert np.array_equal(_bits(r['inv_depth']), _bits(np.where(have, r['rho3'], 0.0)))
    assert np.array_equal(_bits(r['var_inv_depth']), _bits(np.where(have, r['var2'], np.nan)))
    assert np.array_equal(r['flags'], have * FLAG_PROP + r['filled'] * FLAG_FILLED + r['removed'] * FLAG_REMOVED)
    assert np.array_equal(r['source'], np.where(r['valid0'] & ~r['removed'], p['source'], -1))


def test_fusion_of_the_map_is_the_fusion_table_pixel_by_pixel():
    """fuse_map (the table over a whole map at once) against dense_ba_prop_f64.fuse_pixel at every pixel of the 24 x 40 scene, gate 3 and
    gate 0, with the scene's three absent measurements and its holes: the same bits, flags and float32 depths."""
    sc, refs = prop_case(3, 24, 40)
    p = refs['pure'][1]
    have = p['source'] >= 0
    for gate in (3.0, 0.0):
        rf, sf, fl, dep = reg.fuse_map(p['inv_depth'], p['var_inv_depth'], have, sc['depth_next'][1], sc['var_next'][1], gate)
        want = refs['gate3' if gate else 'gate0'][1]
        assert np.array_equal(_bits(rf), _bits(want['inv_depth'])) and np.array_equal(_bits(sf), _bits(want['var_inv_depth']))
        assert np.array_equal(fl, want['flags']) and np.array_equal(dep.view(np.int32), want['depth'].view(np.int32))
        for v, u in ((0, 7), (0, 20), (0, 33), (5, 5), (23, 39)):
            one = fuse_pixel(p['inv_depth'][v, u], p['var_inv_depth'][v, u], have[v, u], sc['depth_next'][1][v, u], sc['var_next'][1][v, u], gate)
            assert (rf[v, u], fl[v, u]) == (one[0], one[2]) and (sf[v, u] == one[1] or (np.isnan(sf[v, u]) and np.isnan(one[1])))
    rf, sf, fl, dep = reg.fuse_map(p['inv_depth'], p['var_inv_depth'], have, None, None, 3.0)
    assert np.array_equal(_bits(rf), _bits(p['inv_depth'])) and np.array_equal(_bits(sf), _bits(p['var_inv_depth']))
    assert np.array_equal(fl, p['flags']) and np.array_equal(dep.view(np.int32), p['depth'].view(np.int32))


# ------------------------------------------------------------------------------------------------ 2. hand-made tables
S = 1e-4          # one variance for the tables: at reg_gate 3 two values are compatible up to 3 sqrt(2e-4) = 0.0424 apart
NEAR, FAR = 0.5, 0.125


def _table(fill=0.0):
    return np.full((5, 5), fill), np.full((5, 5), S)


def _run(rho, var, **kw):
    rho = np.where(rho > 0, rho, 0.0)
    return regularize_reference_link(rho, np.where(rho > 0, var, np.nan), np.arange(25, dtype=np.int32).reshape(5, 5), **dict(DEFAULTS, **kw))


def test_table_far_pixel_among_nearer_neighbours_is_removed_and_a_nearest_never():
    rho, var = _table()
    rho[2, 2] = FAR
    rho[1, 1], rho[1, 3] = NEAR, NEAR          # occl_min = 2 nearer incompatible neighbours, no support
    r = _run(rho, var, fill_radius=0, smooth_radius=0)
    assert r['removed'].sum() == 1 and r['removed'][2, 2] and r['flags'][2, 2] == FLAG_REMOVED and r['source'][2, 2] == -1
    assert r['inv_depth'][2, 2] == 0 and np.isnan(r['var_inv_depth'][2, 2]) and r['flags'][1, 1] == FLAG_PROP and r['source'][1, 1] == 6
    rho[1, 3] = 0.0          # one nearer neighbour is below occl_min
    assert not _run(rho, var, fill_radius=0, smooth_radius=0)['removed'].any()
    assert _run(rho, var, fill_radius=0, smooth_radius=0, occl_min=1)['removed'][2, 2]
    # a near pixel among many far ones: nothing nearer around it, never removed; nor are the far ones (their one nearer neighbour is
    # outvoted by seven compatible ones)
    rho, var = _table(FAR)
    rho[2, 2] = NEAR
    assert not _run(rho, var, fill_radius=0, smooth_radius=0, occl_min=1)['removed'][2, 2]
    assert _run(rho, var, fill_radius=0, smooth_radius=0, occl_min=1)['removed'].sum() == 0
    # farther neighbours that are incompatible count for nothing
    rho, var = _table()
    rho[2, 2], rho[1, 1], rho[1, 3], rho[3, 3] = NEAR, FAR, FAR, FAR
    assert not _run(rho, var, fill_radius=0, smooth_radius=0, occl_min=1)['removed'][2, 2]


def test_table_equal_counts_keep_the_pixel():
    rho, var = _table()
    rho[2, 2], rho[1, 1], rho[1, 3] = FAR, NEAR, NEAR
    rho[3, 1], rho[3, 3] = FAR + 0.01, FAR - 0.01          # two compatible neighbours: n_occ = n_sup = 2
    assert not _run(rho, var, fill_radius=0, smooth_radius=0)['removed'].any()
    rho[3, 3] = 0.0          # n_occ = 2 > n_sup = 1
    r = _run(rho, var, fill_radius=0, smooth_radius=0)
    assert r['removed'][2, 2] and r['removed'].sum() == 1


def test_table_windows_are_clipped_at_corners():
    rho, var = _table()
    rho[0, 0], rho[0, 1], rho[1, 0] = FAR, NEAR, NEAR          # a corner's window holds three neighbours
    r = _run(rho, var, fill_radius=0, smooth_radius=0)
    assert r['removed'][0, 0] and r['removed'].sum() == 1
    rho, var = _table()
    rho[4, 4] = FAR
    rho[2, 2], rho[2, 3], rho[2, 4], rho[3, 2], rho[4, 2] = (NEAR,) * 5          # radius 2 reaches them, radius 1 does not
    assert not _run(rho, var, fill_radius=0, smooth_radius=0)['removed'].any()
    assert _run(rho, var, occl_radius=2, fill_radius=0, smooth_radius=0)['removed'][4, 4]
    # a hole in a corner is filled from its three neighbours, and smoothing a corner averages four values
    rho, var = _table(NEAR)
    rho[0, 4] = 0.0
    r = _run(rho, var, occl_radius=0, smooth_radius=0)
    assert r['filled'][0, 4] and r['filled'].sum() == 1 and r['inv_depth'][0, 4] == NEAR and r['var_inv_depth'][0, 4] == 3 / (3 / S)
    rho, var = _table(NEAR)
    rho[4, 0] = NEAR + 0.02
    r = _run(rho, var, occl_radius=0, fill_radius=0)
    w = 1.0 / S
    assert r['inv_depth'][4, 0] == (w * NEAR + w * NEAR + w * (NEAR + 0.02) + w * NEAR) / (w + w + w + w)          # rows 3, 4; columns 0, 1


def test_table_fill_min_neighbours():
    for n, want in ((DEFAULTS['fill_min'] - 1, False), (DEFAULTS['fill_min'], True)):
        rho, var = _table()
        for k in range(n):
            rho[1, 1 + k] = NEAR + 0.001 * k
        r = _run(rho, var, occl_radius=0, smooth_radius=0)
        assert bool(r['filled'][2, 2]) == want and r['flags'][2, 2] == (FLAG_PROP | FLAG_FILLED if want else 0)
    # the filled value: the weighted mean; the variance: one neighbour's (the harmonic mean) plus the scatter, times fill_inflate
    var[1, 1], var[1, 2], var[1, 3] = S, 2 * S, 4 * S
    for inflate in (1.0, 2.5):
        r = _run(rho, var, occl_radius=0, smooth_radius=0, fill_inflate=inflate)
        w = [1.0 / var[1, 1 + k] for k in range(3)]
        Sw = (0.0 + w[0]) + w[1] + w[2]
        mean = (((0.0 + w[0] * rho[1, 1]) + w[1] * rho[1, 2]) + w[2] * rho[1, 3]) / Sw
        Se = 0.0
        for k in range(3):
            Se = Se + w[k] * ((rho[1, 1 + k] - mean) * (rho[1, 1 + k] - mean))
        assert r['inv_depth'][2, 2] == mean and r['var_inv_depth'][2, 2] == inflate * (3.0 / Sw + Se / Sw) and r['source'][2, 2] == -1
        assert abs(3.0 / Sw - 3.0 / (1 / S + 1 / (2 * S) + 1 / (4 * S))) < 1e-18 and r['var_inv_depth'][2, 2] > inflate * 3.0 / Sw
    # a removed pixel is refilled from what is left around it: both bits
    rho, var = _table()
    rho[2, 2], rho[1, 1], rho[1, 2], rho[1, 3] = FAR, NEAR, NEAR, NEAR
    r = _run(rho, var, smooth_radius=0)
    assert r['flags'][2, 2] == FLAG_PROP | FLAG_FILLED | FLAG_REMOVED and r['inv_depth'][2, 2] == NEAR and r['source'][2, 2] == -1


def test_table_cluster_follows_the_nearest_neighbour():
    rho, var = _table()
    rho[1, 1], rho[1, 2], rho[1, 3], rho[2, 1] = FAR, FAR, FAR, FAR          # four of the far surface
    rho[3, 1], rho[3, 2], rho[3, 3] = NEAR, NEAR + 0.002, NEAR - 0.002          # three of the near one
    r = _run(rho, var, occl_radius=0, smooth_radius=0)
    assert r['filled'][2, 2] and abs(r['inv_depth'][2, 2] - NEAR) < 1e-3
    rho[3, 3] = 0.0          # the near cluster is below fill_min: the hole stays, the far majority does not take it
    r = _run(rho, var, occl_radius=0, smooth_radius=0)
    assert not r['filled'][2, 2]
    # the anchor is the largest rho even when it is alone: with fill_min = 1 the hole takes that one value and its variance
    r = _run(rho, var, occl_radius=0, smooth_radius=0, fill_min=1)
    assert r['filled'][2, 2] and abs(r['inv_depth'][2, 2] - (NEAR + 0.001)) < 2e-3


def test_table_equal_rho_goes_to_the_first_neighbour():
    """Two neighbours with the same largest rho and different variances: compat(k, a) uses s_a, so which one anchors decides the cluster."""
    rho, var = _table()
    rho[1, 1], rho[3, 3] = NEAR, NEAR
    var[1, 1], var[3, 3] = S, 100 * S
    rho[1, 3] = NEAR - 0.06          # (0.06)^2 = 3.6e-3: within 9 (s_k + 100 S) = 9.09e-2 of (3,3), outside 9 (2 S) = 1.8e-3 of (1,1)
    r = _run(rho, var, occl_radius=0, smooth_radius=0, fill_min=1)
    w = [1.0 / S, 1.0 / (100 * S)]
    assert r['filled'][2, 2] and r['inv_depth'][2, 2] == ((0.0 + w[0] * NEAR) + w[1] * NEAR) / ((0.0 + w[0]) + w[1])          # (1,3) is out
    rho, var = rho[::-1, ::-1].copy(), var[::-1, ::-1].copy()          # now the wide one comes first and anchors: (3,1) joins
    r = _run(rho, var, occl_radius=0, smooth_radius=0, fill_min=1)
    assert r['filled'][2, 2] and r['inv_depth'][2, 2] < NEAR - 1e-4


def test_table_radius_zero_leaves_its_stage_out_and_all_zero_is_the_identity():
    rho, var = _table()
    rho[2, 2], rho[1, 1], rho[1, 2], rho[1, 3] = FAR, NEAR, NEAR + 0.004, NEAR - 0.004
    full = _run(rho, var)
    assert full['removed'][2, 2] and full['filled'].sum() >= 1 and full['inv_depth'][1, 2] != rho[1, 2]
    r = _run(rho, var, occl_radius=0)
    assert not r['removed'].any() and not (r['flags'] & FLAG_REMOVED).any() and r['filled'].sum() >= 1 and r['inv_depth'][2, 2] == FAR
    r = _run(rho, var, fill_radius=0)
    assert not r['filled'].any() and r['removed'][2, 2] and r['inv_depth'][1, 2] != rho[1, 2]
    r = _run(rho, var, smooth_radius=0)
    assert r['inv_depth'][1, 2] == rho[1, 2] and r['removed'][2, 2] and r['filled'].any()
    # all radii 0, no measurement: the identity on the bits of a propagated map (0 and NaN at its holes)
    p = prop_case(3, 24, 40)[1]['pure'][0]
    r = regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], **dict(DEFAULTS, occl_radius=0, fill_radius=0, smooth_radius=0))
    for k in ('inv_depth', 'var_inv_depth'):
        assert np.array_equal(_bits(r[k]), _bits(p[k])), k
    assert np.array_equal(r['depth'].view(np.int32), p['depth'].view(np.int32)) and np.array_equal(r['source'], p['source'])
    assert np.array_equal(r['flags'], p['flags']) and r['status'] == OK


# ------------------------------------------------------------------------------------------------ 3. the smoothing weights
def test_smoothing_keeps_an_affine_map_and_never_touches_the_variance():
    """Equal variances and dist_var = 0 make the weights of a window symmetric about its centre, so the mean of an exactly affine rho is
    the centre's value: interior pixels move by rounding only (nine or twenty-five terms: below 1e-14 relative).  The variance map after
    smoothing has the bits it had before, for any input."""
    v, u = np.meshgrid(np.arange(12.0), np.arange(15.0), indexing='ij')
    rho = 0.3 + 0.002 * u - 0.001 * v
    var = np.full(rho.shape, 1e-4)
    for r3 in (1, 2):
        r = regularize_reference_link(rho, var, None, **dict(DEFAULTS, occl_radius=0, fill_radius=0, smooth_radius=r3))
        inner = (slice(r3, 12 - r3), slice(r3, 15 - r3))
        rel = np.abs(r['inv_depth'] - rho)[inner] / rho[inner]
        print('radius %d: largest relative change of an interior pixel %.1e' % (r3, rel.max()))
        assert rel.max() <= 1e-14 and np.abs(r['inv_depth'] - rho).max() > 1e-4          # the border's windows are one-sided
    for B, H, W in ((1, 7, 9), (3, 24, 40)):
        for p in prop_case(B, H, W)[1]['pure']:
            off = regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], dist_var=1e-5, **dict(DEFAULTS, smooth_radius=0))
            on = regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], dist_var=1e-5, **dict(DEFAULTS, smooth_radius=2))
            assert np.array_equal(_bits(on['var_inv_depth']), _bits(off['var_inv_depth'])) and np.array_equal(on['flags'], off['flags'])
            assert (on['inv_depth'] != off['inv_depth']).sum() > 10


# ------------------------------------------------------------------------------------------------ 4. the planted leak scene
def test_leaks_through_a_magnified_patch_are_removed_and_refilled():
    """leak_scene: the strict interior of the patch's footprint holds 315 targets -- 140 hit by the patch, 54 won by background pixels
    through its holes, 121 holes (rounding margin 6.2e-3 px, z-gap 0.81: the source indices are unambiguous).  The default regulariser
    removes 42 pixels, all of them leaks and none anywhere else in the image, and leaves 303 of the 315 within 5 % of the patch's inverse
    depth 1/1.4; with occl_radius = 0 the 54 leaks stay and 261 are there (the holes alone)."""
    sc = leak_scene()
    m = scene_margins(sc['pure'])
    n = {k: int(sc[k].sum()) for k in ('interior', 'hit_fg', 'leak', 'hole')}
    print('margins: rounding %.1e, z-gap %.2f; interior %s' % (m.rounding, m.zgap, n))
    assert m.rounding > 1e-3 and m.zgap > 0.5
    assert n['interior'] == n['hit_fg'] + n['leak'] + n['hole'] and n['interior'] >= 300 and n['leak'] >= 40 and n['hole'] >= 100
    p = sc['pure']
    run = lambda **kw: regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], **dict(DEFAULTS, **kw))
    full, no_occl = run(), run(occl_radius=0)
    c, c0 = leak_counts(sc, full), leak_counts(sc, no_occl)
    print('default: %s; occl_radius = 0: %s' % (c, c0))
    assert c['removed'] == c['removed_leaks']                      # removed is a subset of the leaks, over the whole image
    assert 3 * c['removed_leaks'] >= 2 * n['leak']
    assert c['at_fg'] >= 0.9 * n['interior']
    assert c['at_fg'] > c0['at_fg'] and c0['removed'] == 0
    # what was measured, exactly
    assert (n['interior'], n['hit_fg'], n['leak'], n['hole']) == (315, 140, 54, 121) and (c['removed'], c['at_fg'], c0['at_fg']) == (42, 303, 261)


# ------------------------------------------------------------------------------------------------ 5. the filter on a plane
@pytest.mark.parametrize('H,W', [(24, 40), (48, 64)])
def test_regularised_filter_on_a_plane(H, W):
    """plane_sequence, K = 3, seed 0, every 37th stereo pixel missing, the restatements alone: the committed filter_reference (no stages)
    against the same loop with removal + filling and with all three stages (dist_var = the squared gradient of the target frame's inverse
    depth).  Over each run's own "both, not gated" pixels of the last frame: the stages cover more of the image, filling lowers the RMS
    error, smoothing lowers it again, chi^2/n never exceeds 1 + 4 sqrt(2/n) (smoothing leaves the variance alone: conservative, 0.31 -
    0.32), and no more pixels are left without a prior.  Measured:
      24 x 40  none 0.909 / 1.0452e-2 / 1.045;  fill 0.961 / 9.788e-3 / 0.977;  all 0.966 / 5.599e-3 / 0.318
      48 x 64  none 0.895 / 9.8770e-3 / 0.977;  fill 0.959 / 9.395e-3 / 0.920;  all 0.961 / 5.572e-3 / 0.311   (share / rho RMS / chi^2/n)"""
    base = filter_reference(H, W)[3]
    fill, full = filter_reference_reg(H, W, 'fill'), filter_reference_reg(H, W, 'all')
    for name, st in (('none', base), ('fill', fill[3]), ('all', full[3])):
        print('%dx%d %-4s share %.3f  n %d  rho RMS %.4e  chi^2/n %.3f (<= %.3f)  without a prior %d' % (
            H, W, name, st['share'], st['n'], st['rms'], st['chi2'], 1 + 4 * math.sqrt(2.0 / st['n']), st['none']))
    for _, priors, runs, st in (fill, full):
        assert all(r['status'] == OK and pr['status'] == OK for r, pr in zip(runs, priors))
        assert st['share'] > base['share']
        assert st['chi2'] <= 1 + 4 * math.sqrt(2.0 / st['n'])
        assert st['none'] <= base['none']
        assert any(pr['filled'].sum() > 0 for pr in priors)
    assert fill[3]['rms'] < base['rms']
    assert full[3]['rms'] < fill[3]['rms']


def test_status_words_of_the_restatement():
    sc, refs = prop_case(3, 24, 40)
    p = refs['pure'][1]
    meas = dict(depth_next=sc['depth_next'][1], var_next=sc['var_next'][1], gate=3.0)
    for kw, want in ((dict(status=FEW), FEW), (dict(dist_var=-1.0), BADPRIOR), (dict(dist_var=np.nan), BADPRIOR), (dict(dist_var=np.inf), BADPRIOR),
                     (dict(status=FEW, dist_var=-1.0), FEW)):
        r = regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], **kw, **meas)
        assert r['status'] == want and (r['source'] == -1).all() and not (r['flags'] & ~np.uint8(FLAG_MEAS)).any()
        present = r['flags'] == FLAG_MEAS
        assert present.sum() == 24 * 40 - 3 and np.array_equal(r['depth'].view(np.int32), sc['depth_next'][1].view(np.int32))
        assert np.array_equal(r['var_inv_depth'][present], sc['var_next'][1][present].astype(np.float64)) and np.isnan(r['var_inv_depth'][~present]).all()
    # a healthy link with the measurement: gated pixels exist, and a filled pixel can be fused or gated like any other
    r = regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], **meas)
    assert r['status'] == OK and (r['flags'] & FLAG_GATED).any() and ((r['flags'] & (FLAG_FILLED | FLAG_MEAS)) == (FLAG_FILLED | FLAG_MEAS)).any()


# ------------------------------------------------------------------------------------------------ 6. error paths and plumbing
@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from islam_amd import _lib
    return _lib.lib()


def test_symbols_are_declared_exported_and_bound(lib):
    from islam_amd import _lib, dense_ba, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'islam_hip.h')).read()
    for name in ('islam_depth_regularize_scratch_bytes', 'islam_depth_regularize'):
        assert name in _lib.SIGNATURES and hasattr(lib._cdll, name), name
        assert name + '(' in header
    assert callable(ops.dense_ba_depth_regularize)
    assert ops.DenseBARegularized._fields == ('inv_depth', 'var_inv_depth', 'depth', 'source', 'flags', 'status')
    d = dense_ba.DepthRegularizer()
    assert d._asdict() == dict(DEFAULTS, dist_sigma=0.0) and d._replace(smooth_radius=0).smooth_radius == 0
    with pytest.raises(AttributeError):
        d.occl_radius = 2
    assert lib.islam_depth_regularize_scratch_bytes(3, 24, 40) == 0          # one fused launch: nothing in between


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    one = 1        # any non-NULL address: a refused call never reads it

    def call(B=1, H=2, W=2, rho=one, var=one, dist=one, dn=None, vn=None, gate=0.0, r1=1, occl_min=2, r2=1, fill_min=3, inflate=1.0, r3=1, reg_gate=3.0,
             o1=one, o2=one, o3=one, o4=one, o5=one, o6=one):
        return lib.islam_depth_regularize(rho, var, None, None, dist, dn, vn, gate, r1, occl_min, r2, fill_min, inflate, r3, reg_gate, o1, o2, o3, o4, o5,
                                          o6, None, B, H, W, None)

    nan, inf = float('nan'), float('inf')
    cases = [(dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
             (dict(dn=one), b'depth_next and var_next'), (dict(vn=one), b'depth_next and var_next'),
             (dict(gate=-1.0), b'gate'), (dict(gate=nan), b'gate'), (dict(gate=inf), b'gate'),
             (dict(r1=-1), b'radius'), (dict(r1=3), b'radius'), (dict(r2=3), b'radius'), (dict(r2=-1), b'radius'), (dict(r3=3), b'radius'),
             (dict(r3=-2), b'radius'), (dict(occl_min=0), b'occl_min'), (dict(fill_min=0), b'fill_min'), (dict(inflate=0.5), b'fill_inflate'),
             (dict(inflate=nan), b'fill_inflate'), (dict(inflate=inf), b'fill_inflate'), (dict(reg_gate=0.0), b'reg_gate'),
             (dict(reg_gate=-1.0), b'reg_gate'), (dict(reg_gate=nan), b'reg_gate'), (dict(reg_gate=inf), b'reg_gate')]
    cases += [({k: None}, b'NULL') for k in ('rho', 'var', 'dist', 'o1', 'o2', 'o3', 'o4', 'o5', 'o6')]
    for kw, what in cases:
        assert call(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_depth_regularize' in msg and what in msg, (kw, msg)


def test_op_refuses_cpu_tensors_and_bad_arguments():
    """Off the GPU the op raises RuntimeError (there is no CPU path), after its argument rules, which raise ValueError."""
    from islam_amd import ops
    rho, var = torch.full((2, 7, 9), 0.25, dtype=torch.float64), torch.full((2, 7, 9), 1e-4, dtype=torch.float64)
    good = dict(inv_depth=rho, var_inv_depth=var)
    dn, vn = torch.full((2, 7, 9), 4.0), torch.full((2, 7, 9), 4e-4)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_regularize(**good)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_regularize(**good, source=torch.zeros(2, 7, 9, dtype=torch.int32), status=torch.zeros(2, dtype=torch.int32),
                                      dist_var=torch.tensor([1e-6, 2e-6]), depth_next=dn, var_next=vn, gate=3.0, occl_radius=2, occl_min=1, fill_radius=0,
                                      fill_min=2, fill_inflate=2.0, smooth_radius=2, reg_gate=2.0)
    for kw, what in ((dict(var_inv_depth=var[:, :6]), 'var_inv_depth'), (dict(inv_depth=rho[0], var_inv_depth=var[0]), 'inv_depth'),
                     (dict(source=torch.zeros(2, 7, 8, dtype=torch.int32)), 'source'), (dict(status=torch.zeros(3)), 'status'),
                     (dict(dist_var=-1.0), 'dist_var'), (dict(dist_var=float('nan')), 'dist_var'), (dict(dist_var=torch.tensor([1e-6, -1.0])), 'dist_var'),
                     (dict(dist_var=torch.ones(3)), 'dist_var'), (dict(depth_next=dn), 'depth_next'), (dict(var_next=vn), 'depth_next'),
                     (dict(depth_next=dn[:, :6], var_next=vn), 'depth_next'), (dict(depth_next=dn, var_next=vn, gate=-1.0), 'gate'),
                     (dict(gate=float('inf')), 'gate'), (dict(occl_radius=3), 'radius'), (dict(fill_radius=-1), 'radius'), (dict(smooth_radius=1.5), 'radius'),
                     (dict(occl_min=0), 'occl_min'), (dict(fill_min=0), 'fill_min'), (dict(fill_min=2.5), 'fill_min'), (dict(fill_inflate=0.9), 'fill_inflate'),
                     (dict(fill_inflate=float('nan')), 'fill_inflate'), (dict(reg_gate=0.0), 'reg_gate'), (dict(reg_gate=float('inf')), 'reg_gate')):
        with pytest.raises(ValueError, match=what):
            ops.dense_ba_depth_regularize(**dict(good, **kw))


def test_propagate_argument_rules(monkeypatch):
    """DenseReprojectionLoss.propagate(regularize=None) makes today's single call to ops.dense_ba_depth_propagate, measurement included;
    with a DepthRegularizer it propagates without a measurement (gate 0) and hands the pure maps, their source and status, dist_var =
    dist_sigma^2, the measurement, ``gate`` and the record's stages to ops.dense_ba_depth_regularize, whose result it returns as the
    same DenseBAPrior; its ValueError cases."""
    from islam_amd import ops
    from islam_amd.dense_ba import DepthRegularizer
    from tests.test_depth_propagate_cpu import _cpu_loss, _cpu_state
    sc = make_scene(2, 7, 9, seed=1)
    loss = _cpu_loss(sc)
    joint, unc = _cpu_state(sc)
    dn = torch.from_numpy(sc['depth'])
    calls = []
    maps = lambda v: (torch.full((2, 7, 9), 0.25, dtype=torch.float64), torch.full((2, 7, 9), v, dtype=torch.float64), torch.ones(2, 7, 9),
                      torch.zeros(2, 7, 9, dtype=torch.int32), torch.ones(2, 7, 9, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32))

    def fake_prop(inv_depth, var_inv_depth, motion, intr, **kw):
        calls.append(('propagate', (inv_depth, var_inv_depth, motion, intr), kw))
        return ops.DenseBAPropagated(*maps(4e-4))

    def fake_reg(inv_depth, var_inv_depth, **kw):
        calls.append(('regularize', (inv_depth, var_inv_depth), kw))
        return ops.DenseBARegularized(*maps(9e-4))

    monkeypatch.setattr(ops, 'dense_ba_depth_propagate', fake_prop)
    monkeypatch.setattr(ops, 'dense_ba_depth_regularize', fake_reg)
    out = loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, process_sigma=1e-3, regularize=None)
    assert [c[0] for c in calls] == ['propagate']
    kw = calls[0][2]
    assert sorted(kw) == ['depth_next', 'gate', 'mask', 'process_var', 'rgb2imu', 'status', 'var_next'] and kw['gate'] == 3.0
    assert torch.equal(kw['depth_next'], dn) and kw['var_next'].dtype == torch.float32 and kw['process_var'] == 1e-3 * 1e-3
    assert torch.equal(out.sigma_inv_depth, torch.full((2, 7, 9), 0.02, dtype=torch.float64))
    del calls[:]
    cfg = DepthRegularizer(occl_radius=2, fill_min=2, fill_inflate=1.5, dist_sigma=2e-3)
    out = loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, process_sigma=1e-3, gate=2.0, regularize=cfg)
    assert [c[0] for c in calls] == ['propagate', 'regularize']
    (_, link, kw), (_, pure, rkw) = calls
    assert link[0] is joint.inv_depth and link[1] is unc.var_inv_depth and link[2] is joint.motion and link[3].tolist() == list(loss.K4)
    assert kw['mask'] is loss.mask and kw['status'] is unc.status and kw['rgb2imu'] is loss.rgb2imu_pose and kw['process_var'] == 1e-3 * 1e-3
    assert kw['depth_next'] is None and kw['var_next'] is None and kw['gate'] == 0.0
    assert torch.equal(pure[1], torch.full((2, 7, 9), 4e-4, dtype=torch.float64)) and rkw['source'].dtype == torch.int32 and rkw['status'].shape == (2,)
    assert rkw['dist_var'] == 2e-3 * 2e-3 and rkw['gate'] == 2.0 and torch.equal(rkw['depth_next'], dn)
    assert torch.equal(rkw['var_next'], torch.full((2, 7, 9), 0.02, dtype=torch.float64).pow(2).to(torch.float32))
    stages = {k: rkw[k] for k in DEFAULTS}
    assert stages == dict(DEFAULTS, occl_radius=2, fill_min=2, fill_inflate=1.5) and 'dist_sigma' not in rkw
    assert type(out).__name__ == 'DenseBAPrior' and torch.equal(out.sigma_inv_depth, torch.full((2, 7, 9), 9e-4, dtype=torch.float64).sqrt())
    assert torch.equal(out.var_inv_depth, torch.full((2, 7, 9), 9e-4, dtype=torch.float64))
    # a (B,) dist_sigma: squared, with NaN for an entry the device has to refuse (a host tensor is refused here)
    loss.propagate(joint, unc, regularize=DepthRegularizer(dist_sigma=torch.tensor([1e-3, 2e-3], dtype=torch.float64)))
    assert torch.equal(calls[-1][2]['dist_var'], torch.tensor([1e-3 * 1e-3, 2e-3 * 2e-3], dtype=torch.float64))
    assert calls[-1][2]['depth_next'] is None and calls[-1][2]['gate'] == 3.0
    n = len(calls)
    for kw, what in ((dict(regularize=DepthRegularizer(dist_sigma=-1.0)), 'dist_sigma'), (dict(regularize=DepthRegularizer(dist_sigma=float('nan'))), 'dist_sigma'),
                     (dict(regularize=DepthRegularizer(dist_sigma=torch.tensor([0.0, -1.0]))), 'dist_sigma'), (dict(regularize=dict(DEFAULTS)), 'DepthRegularizer'),
                     (dict(regularize=True), 'DepthRegularizer'), (dict(regularize=DepthRegularizer(), depth_next=dn), 'come together')):
        with pytest.raises(ValueError, match=what):
            loss.propagate(joint, unc, **kw)
    assert len(calls) == n


# ------------------------------------------------------------------------------------------------ 7. the kernel's metadata
def test_new_kernel_has_no_private_segment_and_no_spill(lib):
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = _kernels()
    found = [n for n in ks if 'depth_regularize_kernel' in n]
    assert len(found) == 1, found
    assert not any(part in found[0] for part in ('dense_reproj', 'dense_ba', 'reproj_vjp', 'reproj_ift', 'joint_adj')), found[0]
    blk = ks[found[0]]
    print('depth_regularize_kernel vgpr', _field(blk, 'vgpr_count'), 'sgpr', _field(blk, 'sgpr_count'), 'lds', _field(blk, 'group_segment_fixed_size'))
    assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0
    assert _field(blk, 'group_segment_fixed_size') <= 20 * 1024          # 44 x 20 cells of (rho, s) and three bytes: 16.7 KB
