"""The float64 numpy restatement of depth propagation (include/islam_hip.h, islam_depth_propagate), a helper
module beside dense_ba_var_f64.py and not a test file: the warp, the z-buffer and the fusion table pixel by pixel from the header's
definitions (propagate_reference), what a scene must satisfy for source indices and flags to be comparable exactly (scene_margins), the
scenes of the two test files, and the sequence of frames looking at one plane on which the per-link refinements run as a recursive depth
filter (plane_sequence, filter_reference).  The CPU test file checks this module against a brute-force loop, finite differences and
hand-placed cases; the GPU test file holds the kernels to it."""
import collections
import functools

import numpy as np

from oracle import lie
from tests.dense_ba_var_f64 import ba_map_reference_link, ba_refine_map_reference_link, scam_from_sums, variance_reference
from tests.dense_reproj_f64 import BADPRIOR, MOUNT, OK, SEEDS, make_scene, right_perturb

FLAG_PROP, FLAG_MEAS, FLAG_GATED = 1, 2, 4
# Roundings between the device's and this module's values, counted from the definition block.  The per-pixel arithmetic runs the same
# operations in the same order on both sides (the kernel contracts nothing), so what differs is T^-1 = (R, t): the mount conjugation,
# the inverse and the matrix of the quaternion, 32 roundings on an entry of R or t, as the family's other counts take it.  From there to
# rho' = 1 / (a / rho + t_z): xh, yh (2 each), the three products and two sums of a (5), a / rho (1), + t_z (1), 1 / Q.z (1) -- 44 on
# the terms of Q.z, whose sum of magnitudes is at most kappa Q.z with kappa = ((|R20 xh| + |R21 yh| + |R22|) / rho + |t_z|) / Q.z; the
# scenes of the tests have Q.z > 0.1 against |t_z| < 0.9 and depths of 0.05 or >= 2 m, kappa < 5.5 (asserted per scene): K_RHO = 44 x 5.5
# = 242, rounded up to 256.  s' = J^2 s + q with J = a rho'^2 / rho^2: a (12 kappa_a, below 16), rho'^2 (2 K_RHO + 1), rho^2 (1), the
# product and the quotient (2), so J carries 2 K_RHO + 20, J^2 twice that and 1, times s (1), plus q (1): K_VAR = 4 K_RHO + 43, rounded
# up to 4 K_RHO + 64.  The fused values are quotients of sums of positive products: rho_f carries K_RHO + K_VAR + 4 at most, s_f
# 2 K_VAR + 3; one bound for both, K_FUSE = 2 K_VAR + 4.
K_RHO = 256
K_VAR = 4 * K_RHO + 64
K_FUSE = 2 * K_VAR + 4
KAPPA_MAX = 5.5

Margins = collections.namedtuple('Margins', 'rounding zgap hit qz kappa')


def camera_inverse(motion, rgb2imu):
    """(R, t) = T^-1 of a link, T = C^-1 motion C (C = rgb2imu; None: the identity), as link_front forms it."""
    M = np.asarray(motion, np.float64)
    if rgb2imu is not None:
        C = np.asarray(rgb2imu, np.float64)
        M = lie.se3_mul(lie.se3_mul(lie.se3_inv(C), M), C)
    Ti = lie.se3_inv(M)
    return lie.quat_matrix(Ti[3:]), Ti[:3]


def warp_link(rho, var, mask, motion, rgb2imu, intr, process_var):
    """The definition block for every source pixel of one link, float64, one rounding per operation in the header's order.  Returns a
    dict of (H,W) arrays: a, Qz, rho' (rp), J, s' (sp), u2, v2, fu, fv (the floors, as floats), pre (every clause but the bounds: the
    mask, a usable rho and s, Q.z > 0.1, a finite s'), cand (pre and inside the image) and j (the target index, -1 where not cand)."""
    rho, var = np.asarray(rho, np.float64), np.asarray(var, np.float64)
    H, W = rho.shape
    fx, fy, cx, cy = (float(x) for x in intr)
    R, t = camera_inverse(motion, rgb2imu)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    xh, yh = (u - cx) / fx, (v - cy) / fy
    user = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    usable = user & np.isfinite(rho) & (rho > 0) & np.isfinite(var) & (var > 0)
    with np.errstate(all='ignore'):          # an unusable pixel may hold anything
        dx = R[0, 0] * xh + R[0, 1] * yh + R[0, 2]
        dy = R[1, 0] * xh + R[1, 1] * yh + R[1, 2]
        a = R[2, 0] * xh + R[2, 1] * yh + R[2, 2]
        Qx, Qy, Qz = dx / rho + t[0], dy / rho + t[1], a / rho + t[2]
        rp = 1.0 / Qz
        J = a * (rp * rp) / (rho * rho)
        sp = J * J * var + float(process_var)
        u2, v2 = fx * Qx / Qz + cx, fy * Qy / Qz + cy
        fu, fv = np.floor(u2 + 0.5), np.floor(v2 + 0.5)
        pre = usable & (Qz > 0.1) & np.isfinite(sp)
        cand = pre & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        kappa = ((np.abs(R[2, 0] * xh) + np.abs(R[2, 1] * yh) + abs(R[2, 2])) / rho + abs(t[2])) / Qz
    j = np.full((H, W), -1, np.int64)
    j[cand] = fv[cand].astype(np.int64) * W + fu[cand].astype(np.int64)
    return dict(a=a, Qz=Qz, rp=rp, J=J, sp=sp, u2=u2, v2=v2, fu=fu, fv=fv, pre=pre, cand=cand, j=j, kappa=kappa)


def key_of(rp, i):
    """The 64-bit z-buffer key of a candidate: the bits of (float)rho' above 0xFFFFFFFF - i."""
    return (np.uint64(np.float32(rp).view(np.uint32)) << np.uint64(32)) | np.uint64(0xFFFFFFFF - int(i))


def fuse_pixel(rp, sp, have_p, depth_next, var_next, gate):
    """The fusion table at one target: (rho_f, s_f, flags).  depth_next, var_next: float32 scalars or None."""
    meas = False
    if depth_next is not None:
        dn, sm = np.float32(depth_next), np.float64(np.float32(var_next))
        meas = bool(np.isfinite(dn) and dn > 0 and np.isfinite(sm) and sm > 0)
    flags = (FLAG_PROP if have_p else 0) | (FLAG_MEAS if meas else 0)
    rm = 1.0 / np.float64(dn) if meas else 0.0
    if have_p and meas:
        d, tot = rp - rm, sp + sm
        if gate > 0 and d * d > gate * gate * tot:
            return rm, sm, flags | FLAG_GATED
        return (rp * sm + rm * sp) / tot, sp * sm / tot, flags
    if have_p:
        return rp, sp, flags
    if meas:
        return rm, sm, flags
    return 0.0, np.nan, flags


def propagate_reference_link(rho, var, mask, motion, rgb2imu, intr, status=OK, process_var=0.0, depth_next=None, var_next=None, gate=0.0):
    """islam_depth_propagate for one link.  Returns a dict: inv_depth, var_inv_depth (H,W) float64, depth (H,W) float32, source (H,W)
    int32, flags (H,W) uint8, status, and the warp of every source pixel (warp_link's dict under 'warp': u2, v2, rp per candidate)."""
    H, W = np.asarray(rho).shape
    pv = float(process_var)
    st = int(status) if int(status) != OK else (OK if np.isfinite(pv) and pv >= 0 else BADPRIOR)
    w = warp_link(rho, var, mask, motion, rgb2imu, intr, pv)
    keys = np.zeros(H * W, np.uint64)
    if st == OK:
        for i in np.flatnonzero(w['cand'].ravel()):
            j = w['j'].ravel()[i]
            keys[j] = max(keys[j], key_of(w['rp'].ravel()[i], i))
    out = dict(inv_depth=np.zeros((H, W)), var_inv_depth=np.full((H, W), np.nan), depth=np.zeros((H, W), np.float32),
               source=np.full((H, W), -1, np.int32), flags=np.zeros((H, W), np.uint8), status=st, warp=w)
    for j in range(H * W):
        r, c = divmod(j, W)
        src = 0xFFFFFFFF - int(keys[j] & np.uint64(0xFFFFFFFF)) if keys[j] else -1
        rp, sp = (w['rp'].ravel()[src], w['sp'].ravel()[src]) if src >= 0 else (0.0, np.nan)
        dn = None if depth_next is None else depth_next[r, c]
        rf, sf, fl = fuse_pixel(rp, sp, src >= 0, dn, None if dn is None else var_next[r, c], gate)
        out['inv_depth'][r, c], out['var_inv_depth'][r, c], out['source'][r, c], out['flags'][r, c] = rf, sf, src, fl
        out['depth'][r, c] = np.float32(1.0 / rf) if rf > 0 else (np.float32(0.0) if dn is None else dn)
    return out


def propagate_reference(rho, var, mask, motion, rgb2imu, intr, status=None, process_var=0.0, depth_next=None, var_next=None, gate=0.0):
    """propagate_reference_link for every link of a batch: a list of dicts.  intr (4) or (B,4); process_var a number or (B,)."""
    B = rho.shape[0]
    intr = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (B, 4))
    pv = np.broadcast_to(np.asarray(process_var, np.float64).reshape(-1), (B,))
    return [propagate_reference_link(rho[b], var[b], None if mask is None else mask[b], motion[b], rgb2imu, intr[b],
                                     OK if status is None else status[b], pv[b], None if depth_next is None else depth_next[b],
                                     None if var_next is None else var_next[b], gate) for b in range(B)]


def scene_margins(r):
    """What makes a link's source indices and flags comparable exactly, from a propagate_reference_link dict: the smallest distance of
    u2 + 0.5 or v2 + 0.5 to an integer over the pixels that pass every clause but the bounds and land within a pixel of the image
    (rounding); the smallest relative gap between the two largest rho' at a target with two or more candidates (zgap; inf without
    one); the share of targets hit; the smallest relative margin of Q.z to 0.1 over the usable pixels (qz); the largest kappa of a
    candidate (the amplification in K_RHO)."""
    w = r['warp']
    H, W = w['cand'].shape
    near = w['pre'] & (w['fu'] >= -1) & (w['fu'] <= W) & (w['fv'] >= -1) & (w['fv'] <= H)
    frac = lambda x: np.abs(x - np.round(x))
    rounding = float(min(frac(w['u2'][near] + 0.5).min(), frac(w['v2'][near] + 0.5).min())) if near.any() else np.inf
    by_target = collections.defaultdict(list)
    for i in np.flatnonzero(w['cand'].ravel()):
        by_target[w['j'].ravel()[i]].append(w['rp'].ravel()[i])
    gaps = [(s[-1] - s[-2]) / s[-1] for s in (sorted(v) for v in by_target.values() if len(v) > 1)]
    fin = np.isfinite(w['Qz'])
    qz = float((np.abs(w['Qz'][fin] - 0.1) / 0.1).min())
    return Margins(rounding, float(min(gaps)) if gaps else np.inf, len(by_target) / float(H * W), qz,
                   float(w['kappa'][w['cand']].max()) if w['cand'].any() else 0.0)


def multi_targets(r):
    """How many targets of a link receive two or more candidates."""
    j = r['warp']['j'][r['warp']['cand']]
    return int((np.bincount(j) > 1).sum()) if j.size else 0


# ------------------------------------------------------------------------------------------------ the scenes of the kernel tests
SHAPES = [(1, 7, 9), (3, 24, 40), (3, 136, 168)]          # below one wavefront; most workgroups idle; a ragged tail above 64 x 256 threads
NO_VAR = (0.0, np.nan, -1.0)          # variances that take a pixel out
BIG_MOTION = np.array([0.7, -0.5, -0.6, 0.10, -0.14, 0.12])          # se3 of the 7 x 9 scene: several pixels land on one


@functools.lru_cache(maxsize=None)
def prop_scene(B, H, W):
    """The family's scene of a shape (make_scene at its committed seed: the mount, per-link intrinsics, the user mask, every 17th depth
    at 0.05; at 7 x 9 with the large motion BIG_MOTION) with a state rho = 1/depth (1 + 0.05 U(-1,1)), variances 2^U(-14,-8) of which
    three are 0, NaN and -1, and a measurement: the scene's own depth times (1 + 0.1 N(0,1)) as float32 with variances 2^U(-14,-8)
    float32, three entries (depth 0, variance NaN, depth -1) marked absent."""
    big = lie.se3_exp(BIG_MOTION[None]) if H == 7 else None
    sc = make_scene(B, H, W, seed=SEEDS[H], motion=big)
    rng = np.random.default_rng(1000 + H)
    sc['rho'] = (1.0 / sc['depth'].astype(np.float64)) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (B, H, W)))
    sc['var'] = np.exp2(rng.uniform(-14.0, -8.0, (B, H, W)))
    flat = sc['var'].reshape(B, -1)
    for k, val in enumerate(NO_VAR):
        flat[:, 5 + 11 * k] = val
    sc['depth_next'] = (sc['depth'].astype(np.float64) * (1.0 + 0.1 * rng.standard_normal((B, H, W)))).astype(np.float32)
    sc['var_next'] = np.exp2(rng.uniform(-14.0, -8.0, (B, H, W))).astype(np.float32)
    dn, vn = sc['depth_next'].reshape(B, -1), sc['var_next'].reshape(B, -1)
    dn[:, 7], vn[:, 20], dn[:, 33] = 0.0, np.nan, -1.0
    return sc


def prop_args(sc):
    """(rho, var, mask, motion, rgb2imu, intr) of a prop_scene for propagate_reference."""
    return sc['rho'], sc['var'], sc['mask'], sc['motion'], MOUNT, sc['intr']


@functools.lru_cache(maxsize=None)
def prop_case(B, H, W):
    """The scene of a shape and the restatement on it: pure propagation, and with the measurement at gate 3 and gate 0."""
    sc = prop_scene(B, H, W)
    meas = dict(depth_next=sc['depth_next'], var_next=sc['var_next'])
    return sc, dict(pure=propagate_reference(*prop_args(sc)), gate3=propagate_reference(*prop_args(sc), gate=3.0, **meas),
                    gate0=propagate_reference(*prop_args(sc), gate=0.0, **meas))


def gate_margin(r, depth_next, var_next, gate):
    """The smallest relative distance of d^2 / (s' + s_m) to gate^2 over the targets of a link where both hypotheses are present."""
    both = (r['flags'] & 3) == 3
    src = r['source'][both]
    rp, sp = r['warp']['rp'].ravel()[src], r['warp']['sp'].ravel()[src]
    rm, sm = 1.0 / depth_next[both].astype(np.float64), var_next[both].astype(np.float64)
    q = (rp - rm) ** 2 / (sp + sm)
    return float((np.abs(q - gate * gate) / (gate * gate)).min()) if q.size else np.inf


# ------------------------------------------------------------------------------------------------ the recursive filter on a plane
SIGMA_PX = 0.3          # px of flow noise
SIGMA_STEREO = 0.02     # 1/m of noise on every frame's stereo inverse depth
PLANE_SEED = 0
PLANE_HOLES = 37          # filter_reference: every 37th pixel of every later frame's stereo map is knocked out


def plane_sequence(H, W, K, seed, holes=0):
    """K + 1 frames looking at one world plane n.X = d, K links between them.  The inverse depth along a pixel's ray is exactly affine in
    (u, v) for a plane: with camera k at (Rw, tw) in the world, rho = n.(Rw ray) / (d - n.tw), so the true rho of every pixel of every
    frame follows from the ray-plane intersection and its gradient (g_u, g_v) is a constant per frame.  Identity mount, fx = fy = 0.6 W,
    the principal point at the centre; per link a camera motion of 0.1 - 0.2 m and up to 0.03 rad per axis, the exact flow of the true
    depths plus 0.3 px noise (float32) and a start pose 0.02 away from the true one; per frame a stereo map 1 / (rho_true + 0.02 N(0,1))
    as float32; holes > 0: in the frames after the first, every holes-th pixel of the stereo map carries no measurement (0 and NaN in
    turn), so that a target on which nothing lands has no prior at all.  Returns a dict: intr (4), motion (K,7) (the pose of frame k+1 in frame k), start (K,7), flow (K,2,H,W), rho_true
    (K+1,H,W), stereo (K+1,H,W) float32, grad (K+1,2) and process_var (K+1) = (g_u^2 + g_v^2) / 12, the discretisation variance of
    nearest-pixel splatting into that frame."""
    rng = np.random.default_rng(seed)
    intr = np.array([0.6 * W, 0.6 * W, (W - 1) / 2.0, (H - 1) / 2.0])
    n, d = np.array([0.35, -0.25, 1.0]), 5.0
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    ray = np.stack([(u - intr[2]) / intr[0], (v - intr[3]) / intr[1], np.ones_like(u)], -1)
    xi = []
    for _ in range(K):
        tr = rng.standard_normal(3)
        xi.append(np.concatenate([tr / np.linalg.norm(tr) * rng.uniform(0.1, 0.2), rng.uniform(-0.03, 0.03, 3)]))
    motion = lie.se3_exp(np.array(xi))
    world = [np.array([0, 0, 0, 0, 0, 0, 1.0])]
    for k in range(K):
        world.append(lie.se3_mul(world[-1], motion[k]))
    rho_true, grad = [], []
    for X in world:
        Rw, den = lie.quat_matrix(X[3:]), d - n @ X[:3]
        rho_true.append((ray @ Rw.T) @ n / den)
        grad.append([n @ Rw[:, 0] / intr[0] / den, n @ Rw[:, 1] / intr[1] / den])
    rho_true, grad = np.array(rho_true), np.array(grad)
    assert (rho_true > 0.05).all()
    flow = np.zeros((K, 2, H, W))
    for k in range(K):
        Ti = lie.se3_inv(motion[k])
        Q = (ray / rho_true[k][..., None]) @ lie.quat_matrix(Ti[3:]).T + Ti[:3]
        flow[k] = np.stack([intr[0] * Q[..., 0] / Q[..., 2] + intr[2] - u, intr[1] * Q[..., 1] / Q[..., 2] + intr[3] - v])
    flow = (flow + SIGMA_PX * rng.standard_normal(flow.shape)).astype(np.float32)
    noisy = rho_true + SIGMA_STEREO * rng.standard_normal(rho_true.shape)
    assert (noisy > 0).all()
    start = np.array([right_perturb(motion[k], 0.02 * np.array([0.4, -0.5, 0.4, 0.4, -0.3, 0.4])) for k in range(K)])
    stereo = (1.0 / noisy).astype(np.float32)
    if holes:
        later = stereo[1:].reshape(K, -1)
        later[:, 5::2 * holes] = 0.0
        later[:, 5 + holes::2 * holes] = np.nan
    return dict(intr=intr, motion=motion, start=start, flow=flow, rho_true=rho_true, stereo=stereo, grad=grad,
                process_var=(grad ** 2).sum(1) / 12.0)


def sigma_scale(sigma):
    """The weight map DenseReprojectionLoss._prior_weight forms from a per-pixel sigma: float32(1 / sigma^2), 0 where sigma is not finite
    or not positive."""
    ok = np.isfinite(sigma) & (sigma > 0)
    return np.where(ok, 1.0 / np.where(ok, sigma, 1.0) ** 2, 0.0).astype(np.float32)


def filter_stats(prior, seq, k):
    """Over the pixels of frame k flagged "both, not gated": their share of the image, the inverse-depth RMS error of the fused prior and
    of the frame's stereo map, and the mean of (rho_f - rho_true)^2 / s_f; also how many pixels of the frame are left without any prior."""
    sel = np.asarray(prior['flags']) == (FLAG_PROP | FLAG_MEAS)
    err = (np.asarray(prior['inv_depth']) - seq['rho_true'][k])[sel]
    stereo = (1.0 / seq['stereo'][k][sel].astype(np.float64) - seq['rho_true'][k][sel])
    s = np.asarray(prior['var_inv_depth'])[sel]
    return dict(share=float(sel.mean()), n=int(sel.sum()), rms=float(np.sqrt(np.mean(err ** 2))), rms_stereo=float(np.sqrt(np.mean(stereo ** 2))),
                chi2=float(np.mean(err ** 2 / s)), none=int((np.asarray(prior['flags']) == 0).sum()))


@functools.lru_cache(maxsize=None)
def filter_reference(H, W, K=3):
    """The recursive filter on plane_sequence(H, W, K, PLANE_SEED, PLANE_HOLES) with the restatements alone (computed once, shared between the CPU and
    the GPU tests).  Frame 0 starts from its stereo map at sigma = 0.02; link k: the joint refinement with the per-pixel sigma map (20
    evaluations, ba_refine_map_reference_link; a pixel whose sigma is NaN has no prior), the marginal variance at the returned state (variance_reference), the propagation into
    frame k+1 with that frame's discretisation variance, fused with its stereo map at gate 3.  Returns (seq, priors (the K fused priors,
    propagate_reference_link dicts), runs (the K refinements), stats (filter_stats of the last frame))."""
    seq = plane_sequence(H, W, K, PLANE_SEED, PLANE_HOLES)
    depth = seq['stereo'][0]
    sigma = np.full((H, W), SIGMA_STEREO)
    var_next = np.full((H, W), SIGMA_STEREO ** 2, np.float32)
    priors, runs = [], []
    for k in range(K):
        args = (depth, seq['flow'][k], None)
        m = sigma_scale(sigma)
        run = ba_refine_map_reference_link(*args, seq['start'][k], None, seq['intr'], SIGMA_PX ** 2, m, iters=20)
        at = ba_map_reference_link(*args, run['motion'], None, seq['intr'], SIGMA_PX ** 2, m, run['rho'])
        var = SIGMA_PX ** 2 * variance_reference(at, scam_from_sums(at['sums']), True)
        prior = propagate_reference_link(run['rho'], var, None, run['motion'], None, seq['intr'], run['status'], seq['process_var'][k + 1],
                                         seq['stereo'][k + 1], var_next, 3.0)
        priors.append(prior)
        runs.append(run)
        depth = prior['depth']
        with np.errstate(invalid='ignore'):
            sigma = np.sqrt(prior['var_inv_depth'])
    return seq, priors, runs, filter_stats(priors[-1], seq, K)
