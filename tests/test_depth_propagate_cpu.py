"""Depth propagation (include/islam_hip.h, islam_depth_propagate): everything about the float64 numpy restatement
(tests/dense_ba_prop_f64.py) that can be checked without a GPU -- the warp and the z-buffer against a brute-force loop over targets, J
against a finite difference, the fusion table case by case, the fp32 tie rule, the scene conditions the GPU tests rely on, the per-link
refinements run as a recursive depth filter on a sequence of frames looking at one plane -- and the host-side argument errors, the Python
plumbing and the register metadata of the two new kernels."""
import math
import os

import numpy as np
import pytest
import torch

from tests import dense_ba_prop_f64 as prop
from tests.dense_ba_prop_f64 import (FLAG_GATED, FLAG_MEAS, FLAG_PROP, KAPPA_MAX, SHAPES, filter_reference, fuse_pixel, gate_margin, multi_targets,
                                     prop_args, prop_case, propagate_reference_link, scene_margins)
from tests.dense_ba_var_f64 import chi2_band
from tests.dense_reproj_f64 import BADPRIOR, FEW, MOUNT, OK, make_scene


# ------------------------------------------------------------------------------------------------ 1. the warp and the z-buffer
def _pose_matrix(p):
    """[t, q xyzw] as a 4 x 4 homogeneous matrix, from the textbook formula."""
    x, y, z, w = (float(c) for c in p[3:])
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = p[:3]
    return T


def _brute_force(rho, var, mask, motion, rgb2imu, intr, process_var):
    """The winner of every target by a loop over targets and, inside it, over all sources, in Python scalars: (source, rho', s').  T^-1
    comes from 4 x 4 matrices, (C^-1 M C)^-1 by numpy's inverse, not from the helper's quaternion algebra."""
    H, W = rho.shape
    fx, fy, cx, cy = (float(x) for x in intr)
    C, M = _pose_matrix(rgb2imu), _pose_matrix(motion)
    Ti = np.linalg.inv(np.linalg.inv(C) @ M @ C)
    R, t = Ti[:3, :3].tolist(), Ti[:3, 3].tolist()
    out = []
    for j in range(H * W):
        best = None
        for i in range(H * W):
            v, u = divmod(i, W)
            r, s = float(rho[v, u]), float(var[v, u])
            if not (mask[v, u] and math.isfinite(r) and r > 0 and math.isfinite(s) and s > 0):
                continue
            xh, yh = (u - cx) / fx, (v - cy) / fy
            a = R[2][0] * xh + R[2][1] * yh + R[2][2]
            Qx = (R[0][0] * xh + R[0][1] * yh + R[0][2]) / r + t[0]
            Qy = (R[1][0] * xh + R[1][1] * yh + R[1][2]) / r + t[1]
            Qz = a / r + t[2]
            if not Qz > 0.1:
                continue
            rp = 1.0 / Qz
            Jd = a * (rp * rp) / (r * r)
            sp = Jd * Jd * s + process_var
            iu, iv = math.floor(fx * Qx / Qz + cx + 0.5), math.floor(fy * Qy / Qz + cy + 0.5)
            if not (0 <= iu < W and 0 <= iv < H and math.isfinite(sp)) or iv * W + iu != j:
                continue
            rank = (int(np.float32(rp).view(np.uint32)), -i)
            if best is None or rank > best[0]:
                best = (rank, i, rp, sp)
        out.append((-1, 0.0, math.nan) if best is None else best[1:])
    return out


def test_reference_matches_a_brute_force_loop_over_targets():
    """The 7 x 9 scene with the large motion: propagate_reference_link (a scatter with a running maximum of 64-bit keys) names the same
    source at every target as a loop over targets that ranks all sources by (float32 bits of rho', -i), with the same rho' and s' to
    1e-12 relative (the loop forms T^-1 from 4 x 4 matrices, the helper from quaternions: a few roundings apart, against the scene's
    margins of 2e-3 px and 0.18 in rho').  At least five targets receive two or more candidates (a condition on the scene)."""
    sc, refs = prop_case(1, 7, 9)
    r = refs['pure'][0]
    assert multi_targets(r) >= 5
    want = _brute_force(sc['rho'][0], sc['var'][0], sc['mask'][0], sc['motion'][0], MOUNT, sc['intr'][0], 0.0)
    assert [w[0] for w in want] == r['source'].ravel().tolist()
    hit = r['source'].ravel() >= 0
    assert 20 <= hit.sum() < 63
    np.testing.assert_allclose(np.array([w[1] for w in want]), r['inv_depth'].ravel(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.array([w[2] for w in want])[hit], r['var_inv_depth'].ravel()[hit], rtol=1e-12, atol=0)
    assert np.isnan(r['var_inv_depth'].ravel()[~hit]).all() and (r['inv_depth'].ravel()[~hit] == 0).all()
    assert np.array_equal(r['flags'].ravel(), np.where(hit, FLAG_PROP, 0))
    with np.errstate(divide='ignore'):
        assert np.array_equal(r['depth'].ravel(), np.where(hit, 1.0 / r['inv_depth'].ravel(), 0.0).astype(np.float32))
    # a nearer surface wins: at a target with several candidates the winner's rho' is the largest
    w = r['warp']
    for j in np.flatnonzero(np.bincount(w['j'][w['cand']], minlength=63) > 1):
        assert r['inv_depth'].ravel()[j] == w['rp'][w['cand'] & (w['j'] == j)].max()


# ------------------------------------------------------------------------------------------------ 2. the Jacobian
def test_jacobian_is_the_derivative_of_the_warped_inverse_depth():
    """J = a rho'^2 / rho^2 against the central difference of rho'(rho) at h = 1e-6 rho: the quotient's truncation error is
    h^2 |rho'''| / 6, below 1e-10 relative here, and its rounding error 2^-52 / 1e-6 = 2e-10: agreement to 1e-8 relative."""
    sc, refs = prop_case(3, 24, 40)
    worst = 0.0
    for b in range(3):
        args = [a[b] if k in (0, 1, 2, 3, 5) else a for k, a in enumerate(prop_args(sc))]
        w = refs['pure'][b]['warp']
        h = 1e-6 * sc['rho'][b]
        up = prop.warp_link(sc['rho'][b] + h, *args[1:], 0.0)['rp']
        dn = prop.warp_link(sc['rho'][b] - h, *args[1:], 0.0)['rp']
        c = w['cand']
        err = np.abs((up - dn)[c] / (2 * h[c]) - w['J'][c]) / np.abs(w['J'][c])
        worst = max(worst, float(err.max()))
        assert c.sum() > 500 and (w['J'][c] > 0).all()
    print('worst relative gap between J and the difference quotient: %.2e' % worst)
    assert worst < 1e-8


# ------------------------------------------------------------------------------------------------ 3. the fusion table
def test_fusion_table_case_by_case():
    rp, sp = 0.25, 4e-4
    f32 = np.float32
    # both, not gated: the information-weighted mean, a variance below both
    dn, vn = f32(1.0 / 0.27), f32(9e-4)
    rm, sm = 1.0 / np.float64(dn), np.float64(vn)
    rf, sf, fl = fuse_pixel(rp, sp, True, dn, vn, 3.0)
    assert fl == FLAG_PROP | FLAG_MEAS and rf == (rp * sm + rm * sp) / (sp + sm) and sf == sp * sm / (sp + sm)
    assert min(rp, rm) < rf < max(rp, rm) and sf <= min(sp, sm)
    assert abs(rf - (rp / sp + rm / sm) / (1 / sp + 1 / sm)) < 1e-15 and abs(1 / sf - (1 / sp + 1 / sm)) < 1e-9 / sf
    # gated: |d| > 3 sqrt(s' + s_m); the measurement alone, its bits
    dn = f32(1.0 / 0.5)
    assert (rp - 0.5) ** 2 > 9 * (sp + sm)
    assert fuse_pixel(rp, sp, True, dn, vn, 3.0) == (1.0 / np.float64(dn), sm, FLAG_PROP | FLAG_MEAS | FLAG_GATED)
    # gate = 0 never gates, whatever the distance
    rf, sf, fl = fuse_pixel(rp, sp, True, dn, vn, 0.0)
    assert fl == FLAG_PROP | FLAG_MEAS and sf <= min(sp, sm)
    # only the propagated value; a measurement that is not finite or not positive in depth or in variance counts as absent
    assert fuse_pixel(rp, sp, True, None, None, 3.0) == (rp, sp, FLAG_PROP)
    for bad in ((f32(0.0), vn), (f32(-1.0), vn), (f32(np.nan), vn), (f32(np.inf), vn), (dn, f32(0.0)), (dn, f32(np.nan)), (dn, f32(-1.0)), (dn, f32(np.inf))):
        assert fuse_pixel(rp, sp, True, *bad, 3.0) == (rp, sp, FLAG_PROP), bad
        rf, sf, fl = fuse_pixel(0.0, np.nan, False, *bad, 3.0)
        assert rf == 0.0 and np.isnan(sf) and fl == 0, bad
    # only the measurement; none
    assert fuse_pixel(0.0, np.nan, False, dn, vn, 3.0) == (1.0 / np.float64(dn), sm, FLAG_MEAS)
    rf, sf, fl = fuse_pixel(0.0, np.nan, False, None, None, 3.0)
    assert rf == 0.0 and np.isnan(sf) and fl == 0
    # over a scene: s_f <= min(s', s_m) wherever both are fused, and gate = 0 sets bit 2 nowhere while gate = 3 does
    sc, refs = prop_case(3, 24, 40)
    for b in range(3):
        g3, g0 = refs['gate3'][b], refs['gate0'][b]
        assert not (g0['flags'] & FLAG_GATED).any() and (g3['flags'] & FLAG_GATED).sum() > 50
        assert np.array_equal(g3['flags'] & 3, g0['flags']) and np.array_equal(g3['source'], g0['source'])
        for r in (g3, g0):
            both = r['flags'] == (FLAG_PROP | FLAG_MEAS)
            sp_ = r['warp']['sp'].ravel()[r['source'][both]]
            assert both.sum() > 100 and (r['var_inv_depth'][both] <= np.minimum(sp_, sc['var_next'][b][both].astype(np.float64))).all()
        gated = (g3['flags'] & FLAG_GATED) != 0
        assert np.array_equal(g3['inv_depth'][gated], 1.0 / sc['depth_next'][b][gated].astype(np.float64))
        assert np.array_equal(g3['depth'][gated].view(np.int32), sc['depth_next'][b][gated].view(np.int32))


# ------------------------------------------------------------------------------------------------ 4. the fp32 tie rule
def tie_scene(rel):
    """One row of seven pixels, identity mount and rotation, T^-1 = (I, (0, 0, 1.5)), fx = 1, cx = 3: a pixel at u - cx = x and rho = 1
    lands at x / 2.5, so sources 5 (x = 2) and 6 (x = 3) both land on target 4 with rho' = 0.4.  Source 6 carries rho (1 + rel)."""
    rho = np.zeros((1, 7))
    rho[0, 5], rho[0, 6] = 1.0, 1.0 + rel
    var = np.full((1, 7), 1e-4)
    motion = np.array([0, 0, -1.5, 0, 0, 0, 1.0])
    return rho, var, None, motion, None, np.array([1.0, 1.0, 3.0, 0.0])


def test_equal_fp32_keys_go_to_the_smaller_source_index():
    for rel, want in ((1e-12, 5), (0.0, 5), (-1e-12, 5), (1e-3, 6), (-1e-3, 5)):
        r = propagate_reference_link(*tie_scene(rel))
        rp = r['warp']['rp'][0]
        assert r['warp']['j'][0, 5] == r['warp']['j'][0, 6] == 4 and r['warp']['cand'].sum() == 2
        assert (np.float32(rp[5]) == np.float32(rp[6])) == (abs(rel) < 1e-6)
        assert r['source'][0].tolist() == [-1, -1, -1, -1, want, -1, -1], rel
        assert r['inv_depth'][0, 4] == rp[want]
    r = propagate_reference_link(*tie_scene(1e-12))
    assert r['warp']['rp'][0, 6] > r['warp']['rp'][0, 5]          # the loser is nearer in float64: the rule is the fp32 one


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
    for name in ('islam_depth_propagate_scratch_bytes', 'islam_depth_propagate'):
        assert name in _lib.SIGNATURES and hasattr(lib._cdll, name), name
        assert name + '(' in header
    assert callable(ops.dense_ba_depth_propagate) and callable(dense_ba.DenseReprojectionLoss.propagate)
    assert ops.DenseBAPropagated._fields == ('inv_depth', 'var_inv_depth', 'depth', 'source', 'flags', 'status')
    assert dense_ba.DenseBAPrior._fields == ('depth', 'sigma_inv_depth', 'inv_depth', 'var_inv_depth', 'source', 'flags', 'status')
    f = lib.islam_depth_propagate_scratch_bytes
    assert f(0, 4, 4) == 0 and f(2, 0, 4) == 0 and f(2, 4, -1) == 0 and 3 * 24 * 40 * 8 <= f(3, 24, 40) < 3 * 24 * 40 * 8 + 256


def test_host_side_argument_errors(lib):
    """Arguments are refused on the host, before any device work, with a message naming the entry point."""
    one = 1        # any non-NULL address: a refused call never reads it

    def call(B=1, H=2, W=2, rho=one, var=one, motion=one, intr=one, pv=one, dn=None, vn=None, gate=0.0, o1=one, o2=one, o3=one, o4=one, o5=one,
             o6=one, scratch=one):
        return lib.islam_depth_propagate(rho, var, None, motion, None, intr, None, pv, dn, vn, gate, o1, o2, o3, o4, o5, o6, scratch, B, H, W, None)

    cases = [(dict(B=0), b'bad shape'), (dict(H=0), b'bad shape'), (dict(W=-1), b'bad shape'), (dict(H=1 << 16, W=1 << 16), b'bad shape'),
             (dict(H=1 << 15, W=(1 << 15) + 1), b'bad shape'), (dict(dn=one), b'depth_next and var_next'), (dict(vn=one), b'depth_next and var_next'),
             (dict(gate=-1.0), b'gate'), (dict(gate=float('nan')), b'gate'), (dict(gate=float('inf')), b'gate')]
    cases += [({k: None}, b'NULL') for k in ('rho', 'var', 'motion', 'intr', 'pv', 'o1', 'o2', 'o3', 'o4', 'o5', 'o6', 'scratch')]
    for kw, what in cases:
        assert call(**kw) == -1, kw
        msg = lib.islam_last_error()
        assert b'islam_depth_propagate' in msg and what in msg, (kw, msg)


def _cpu_loss(sc):
    from islam_amd import lietensor as pp
    from islam_amd.dense_ba import DenseReprojectionLoss
    fx, fy, cx, cy = sc['intr'][0]
    return DenseReprojectionLoss(torch.from_numpy(sc['depth']), torch.from_numpy(sc['flow']), fx, fy, cx, cy, torch.from_numpy(sc['mask']),
                                 pp.SE3(torch.from_numpy(MOUNT)), device='cpu')


def _cpu_state(sc):
    from islam_amd.dense_ba import DenseBADepthUncertainty, DenseBAJoint
    rho = 1.0 / torch.from_numpy(sc['depth']).double()
    joint = DenseBAJoint(*([None] * 14))._replace(motion=torch.from_numpy(sc['motion']), inv_depth=rho, status=torch.zeros(2, dtype=torch.int32))
    unc = DenseBADepthUncertainty(torch.full_like(rho, 1e-4), None, None, torch.tensor([0, 1], dtype=torch.int32))
    return joint, unc


def test_op_refuses_cpu_tensors_and_bad_arguments():
    """Off the GPU the op raises RuntimeError (there is no CPU path), after its argument rules, which raise ValueError."""
    from islam_amd import ops
    sc = make_scene(2, 7, 9, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rho, var = 1.0 / t(sc['depth']).double(), torch.full((2, 7, 9), 1e-4, dtype=torch.float64)
    good = dict(inv_depth=rho, var_inv_depth=var, motion=t(sc['motion']), intr=t(sc['intr']))
    dn, vn = t(sc['depth']), torch.full((2, 7, 9), 4e-4)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_propagate(**good)
    with pytest.raises(RuntimeError, match='device tensors'):
        ops.dense_ba_depth_propagate(**good, mask=t(sc['mask']), status=torch.zeros(2, dtype=torch.int32), rgb2imu=t(MOUNT), process_var=1e-6, depth_next=dn,
                                     var_next=vn, gate=3.0)
    for kw, what in ((dict(var_inv_depth=var[:, :6]), 'var_inv_depth'), (dict(inv_depth=rho[0], var_inv_depth=var[0]), 'inv_depth'),
                     (dict(motion=t(sc['motion'])[:1]), 'motion'), (dict(intr=torch.ones(3, 4)), 'intr'), (dict(mask=torch.ones(2, 7, 8)), 'mask'),
                     (dict(rgb2imu=torch.ones(6)), 'rgb2imu'), (dict(status=torch.zeros(3)), 'status'), (dict(process_var=-1.0), 'process_var'),
                     (dict(process_var=float('nan')), 'process_var'), (dict(process_var=torch.tensor([1e-6, -1.0])), 'process_var'),
                     (dict(process_var=torch.ones(3)), 'process_var'), (dict(depth_next=dn), 'depth_next'), (dict(var_next=vn), 'depth_next'),
                     (dict(depth_next=dn[:, :6], var_next=vn), 'depth_next'), (dict(depth_next=dn, var_next=vn, gate=-1.0), 'gate'),
                     (dict(gate=float('inf')), 'gate')):
        with pytest.raises(ValueError, match=what):
            ops.dense_ba_depth_propagate(**dict(good, **kw))
    loss = _cpu_loss(sc)
    with pytest.raises(RuntimeError, match='device tensors'):
        loss.propagate(*_cpu_state(sc), depth_next=dn, sigma_inv_depth_next=0.02)


def test_python_argument_rules(monkeypatch):
    """DenseReprojectionLoss.propagate hands ops the refinement's state, the uncertainty's variance and status, the stored mask,
    intrinsics and mount, process_var = process_sigma^2 and var_next = float32(sigma^2) (NaN where a map's sigma is not finite or not
    positive), and returns sigma_inv_depth = sqrt(var); its ValueError cases."""
    from islam_amd import ops
    sc = make_scene(2, 7, 9, seed=1)
    loss = _cpu_loss(sc)
    joint, unc = _cpu_state(sc)
    dn = torch.from_numpy(sc['depth'])
    calls = []

    def fake(inv_depth, var_inv_depth, motion, intr, **kw):
        calls.append((inv_depth, var_inv_depth, motion, intr, kw))
        var = torch.full((2, 7, 9), 4e-4, dtype=torch.float64)
        var[0, 0, 0] = float('nan')
        return ops.DenseBAPropagated(torch.ones(2, 7, 9, dtype=torch.float64), var, torch.ones(2, 7, 9), None, None, None)

    monkeypatch.setattr(ops, 'dense_ba_depth_propagate', fake)
    out = loss.propagate(joint, unc)
    rho, var, motion, intr, kw = calls[-1]
    assert rho is joint.inv_depth and var is unc.var_inv_depth and motion is joint.motion and intr.tolist() == list(loss.K4)
    assert kw['mask'] is loss.mask and kw['status'] is unc.status and kw['rgb2imu'] is loss.rgb2imu_pose
    assert kw['process_var'] == 0.0 and kw['depth_next'] is None and kw['var_next'] is None and kw['gate'] == 3.0
    assert torch.equal(out.sigma_inv_depth[1], torch.full((7, 9), 0.02, dtype=torch.float64)) and torch.isnan(out.sigma_inv_depth[0, 0, 0])
    assert out._fields[:2] == ('depth', 'sigma_inv_depth') and out.var_inv_depth is not None
    sig = torch.from_numpy(np.random.default_rng(3).uniform(0.01, 0.05, (2, 7, 9)))
    sig[0, 2, 5], sig[1, 3, 1], sig[0, 1, 7], sig[1, 0, 0] = 0.0, float('nan'), -1.0, float('inf')
    bad = ~(torch.isfinite(sig) & (sig > 0))
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=sig, process_sigma=1e-3, gate=0.0)
    kw = calls[-1][4]
    assert kw['process_var'] == 1e-3 * 1e-3 and kw['gate'] == 0.0 and torch.equal(kw['depth_next'], dn)
    assert kw['var_next'].dtype == torch.float32 and torch.equal(torch.isnan(kw['var_next']), bad) and bad.sum() == 4
    assert torch.equal(kw['var_next'][~bad], (sig * sig).to(torch.float32)[~bad])
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=0.02, process_sigma=torch.tensor([1e-3, 2e-3], dtype=torch.float64))
    kw = calls[-1][4]
    assert torch.equal(kw['var_next'], torch.full((2, 7, 9), 0.02, dtype=torch.float64).pow(2).to(torch.float32))
    assert torch.equal(kw['process_var'], torch.tensor([1e-3 * 1e-3, 2e-3 * 2e-3], dtype=torch.float64))
    loss.propagate(joint, unc, depth_next=dn, sigma_inv_depth_next=torch.tensor([0.02, 0.04], dtype=torch.float64))
    assert torch.equal(calls[-1][4]['var_next'][:, 0, 0], torch.tensor([0.02, 0.04], dtype=torch.float64).pow(2).to(torch.float32))
    n = len(calls)
    for kw, what in ((dict(depth_next=dn), 'come together'), (dict(sigma_inv_depth_next=0.02), 'come together'),
                     (dict(depth_next=dn[:, :6], sigma_inv_depth_next=0.02), 'depth_next'), (dict(depth_next=dn, sigma_inv_depth_next=0.0), 'sigma_inv_depth_next'),
                     (dict(depth_next=dn, sigma_inv_depth_next=float('nan')), 'sigma_inv_depth_next'),
                     (dict(depth_next=dn, sigma_inv_depth_next=torch.tensor([0.02, -1.0])), 'sigma_inv_depth_next'),
                     (dict(depth_next=dn, sigma_inv_depth_next=torch.ones(2, 2)), 'sigma_inv_depth_next'),
                     (dict(depth_next=dn, sigma_inv_depth_next=torch.ones(2, 7, 8)), 'sigma_inv_depth_next'), (dict(process_sigma=-1.0), 'process_sigma'),
                     (dict(process_sigma=float('inf')), 'process_sigma'), (dict(process_sigma=torch.tensor([0.0, -1.0])), 'process_sigma')):
        with pytest.raises(ValueError, match=what):
            loss.propagate(joint, unc, **kw)
    assert len(calls) == n


# ------------------------------------------------------------------------------------------------ 6. the kernels' metadata
def test_new_kernels_have_no_private_segment_and_no_spill(lib):
    from tests.test_codeobj_cpu import LIB, READELF, _field, _kernels
    if not (os.path.exists(LIB) and os.path.exists(READELF)):
        pytest.skip('library or llvm-readelf missing')
    ks = _kernels()
    for want in ('depth_splat_kernel', 'depth_fuse_kernel'):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert not any(part in found[0] for part in ('dense_reproj', 'dense_ba', 'reproj_vjp', 'reproj_ift', 'joint_adj')), found[0]
        blk = ks[found[0]]
        print(want, 'vgpr', _field(blk, 'vgpr_count'), 'sgpr', _field(blk, 'sgpr_count'), 'lds', _field(blk, 'group_segment_fixed_size'))
        assert _field(blk, 'private_segment_fixed_size') == 0 and _field(blk, 'vgpr_spill_count') == 0, want


# ------------------------------------------------------------------------------------------------ 7. what the GPU tests rely on
@pytest.mark.parametrize('B,H,W', SHAPES)
def test_scene_conditions(B, H, W):
    """On the restatement alone: no candidate rounds within 1e-9 of a pixel border or lies within 1e-9 of the Q.z threshold, no two
    candidates of one target are closer than 1e-5 relative in rho' (fp32 resolves 6e-8), no d^2 / (s' + s_m) lies within 1e-9 of gate^2,
    the amplification kappa of K_RHO stays below its bound, the two larger shapes hit at least 40 % of their targets, every shape has
    targets with several candidates, and the fused run shows every row of the fusion table."""
    sc, refs = prop_case(B, H, W)
    seen = np.zeros(8, int)
    for b in range(B):
        m = scene_margins(refs['pure'][b])
        multi = multi_targets(refs['pure'][b])
        gm = gate_margin(refs['gate3'][b], sc['depth_next'][b], sc['var_next'][b], 3.0)
        print('%dx%d link %d: rounding %.1e, z-gap %.1e, hit %.0f %%, Q.z margin %.1e, kappa %.2f, %d multi-candidate targets, gate margin %.1e' % (
            H, W, b, m.rounding, m.zgap, 100 * m.hit, m.qz, m.kappa, multi, gm))
        assert m.rounding > 1e-9 and m.zgap > 1e-5 and m.qz > 1e-9 and gm > 1e-9 and m.kappa < KAPPA_MAX
        assert m.hit >= 0.4 or H == 7
        assert multi >= (5 if H == 7 else 50)
        seen += np.bincount(refs['gate3'][b]['flags'].ravel(), minlength=8)
        cand = refs['pure'][b]['warp']['cand']
        assert 0.4 < cand.mean() < 0.95 and not cand.ravel()[[5, 16, 27]].any()          # the three variances 0, NaN, -1
    assert (seen[[0, 1, 2, 3, 7]] > 0).all() and seen[[4, 5, 6]].sum() == 0
    assert (~sc['mask']).any() and (sc['depth'] == np.float32(0.05)).any()


def test_status_words_of_the_restatement():
    sc, refs = prop_case(3, 24, 40)
    args = [a[1] if k in (0, 1, 2, 3, 5) else a for k, a in enumerate(prop_args(sc))]
    meas = dict(depth_next=sc['depth_next'][1], var_next=sc['var_next'][1], gate=3.0)
    for kw, want in ((dict(status=FEW), FEW), (dict(process_var=-1.0), BADPRIOR), (dict(process_var=np.nan), BADPRIOR), (dict(status=FEW, process_var=-1.0), FEW)):
        r = propagate_reference_link(*args, **kw, **meas)
        assert r['status'] == want and (r['source'] == -1).all() and not (r['flags'] & ~np.uint8(FLAG_MEAS)).any()
        present = r['flags'] == FLAG_MEAS
        assert present.sum() == 24 * 40 - 3 and np.array_equal(r['depth'].view(np.int32), sc['depth_next'][1].view(np.int32))
        assert np.array_equal(r['var_inv_depth'][present], sc['var_next'][1][present].astype(np.float64)) and np.isnan(r['var_inv_depth'][~present]).all()


# ------------------------------------------------------------------------------------------------ 8. the recursive filter
@pytest.mark.parametrize('H,W', [(24, 40), (48, 64)])
def test_filter_on_a_plane_beats_the_stereo_map(H, W):
    """Three links over four frames looking at one plane (plane_sequence, seed 0), the restatements alone: refine_joint with the per-pixel
    sigma map, the marginal variance, the propagation with the discretisation variance (g_u^2 + g_v^2) / 12 of the next frame, the fusion
    with that frame's stereo map (sigma 0.02, every 37th pixel without a measurement) at gate 3.  At the last frame, over the pixels flagged "both, not gated" (at least half
    the image, a condition), the fused prior's inverse-depth RMS error is strictly below the stereo map's on the same pixels, and the
    mean of (rho_f - rho_true)^2 / s_f lies within 1 +- 4 sqrt(2 / n).  Measured: 24 x 40  RMS 1.9501e-2 (stereo) -> 1.0452e-2 on 90.9 %
    of the image, chi^2/n 1.045 (band 0.81 .. 1.19);  48 x 64  2.0155e-2 -> 9.8770e-3 on 89.5 %, chi^2/n 0.977 (0.89 .. 1.11)."""
    seq, priors, runs, st = filter_reference(H, W)
    for k, (run, pr) in enumerate(zip(runs, priors)):
        m = scene_margins(pr)
        print('link %d: accepted %d rejected %d last step %.1e; rounding %.1e z-gap %.1e hit %.0f %%; flags %s' % (
            k, run['accepted'], run['rejected'], run['last_step'], m.rounding, m.zgap, 100 * m.hit, np.bincount(pr['flags'].ravel(), minlength=8).tolist()))
        assert run['status'] == OK and pr['status'] == OK and run['last_step'] < 1e-6
        assert m.rounding > 1e-9 and m.zgap > 1e-5
        assert gate_margin(pr, seq['stereo'][k + 1], np.full((H, W), prop.SIGMA_STEREO ** 2, np.float32), 3.0) > 1e-6
    lo, hi = chi2_band(st['n'])
    print('%dx%d: %.1f %% of the last frame fused; rho RMS stereo %.4e -> fused %.4e; chi^2/n %.3f in %.2f .. %.2f' % (
        H, W, 100 * st['share'], st['rms_stereo'], st['rms'], st['chi2'], lo, hi))
    assert st['share'] >= 0.5
    # every prior has pixels with nothing at all (sigma NaN: "no prior" for the next link) and pixels with a propagated value only
    assert all(prop.filter_stats(pr, seq, k + 1)['none'] > 0 and (pr['flags'] == FLAG_PROP).sum() > 0 for k, pr in enumerate(priors))
    assert st['rms'] < st['rms_stereo']
    assert lo <= st['chi2'] <= hi
    # the filter learns: every link's fused error is below the one before it
    rms = [prop.filter_stats(pr, seq, k + 1)['rms'] for k, pr in enumerate(priors)]
    assert rms[0] > rms[1] > rms[2]
