"""The float64 numpy restatement of the regularisation of a propagated inverse-depth map (include/islam_hip.h, islam_depth_regularize;
DESIGN.md section 3.29), a helper module beside dense_ba_prop_f64.py and not a test file: occlusion removal, hole filling, smoothing and
the fusion table from the header's definitions (regularize_reference_link), the planted scene in which background leaks through the holes
of a magnified foreground patch (leak_scene), and the recursive filter of dense_ba_prop_f64.filter_reference with the regularisation
between the pure propagation and the fusion (filter_reference_reg).

Every stage loops explicitly over the offsets (dv, du) of its window, row by row, and adds one neighbour's term at a time to the running
sums of all pixels at once (np.where keeps a sum untouched where the neighbour does not count), so each pixel's sum is formed by the
IEEE operations of the definition in the definition's order; nothing here reduces with np.sum, whose pairwise order is another one.  The
CPU test file checks this module against a scalar brute force and hand-made tables; the GPU test file holds the kernel to it bit for bit."""
import functools

import numpy as np

from tests import dense_ba_prop_f64 as prop
from tests.dense_ba_prop_f64 import FLAG_GATED, FLAG_MEAS, FLAG_PROP, PLANE_HOLES, PLANE_SEED, SIGMA_PX, SIGMA_STEREO
from tests.dense_ba_var_f64 import ba_map_reference_link, ba_refine_map_reference_link, scam_from_sums, variance_reference
from tests.dense_reproj_f64 import BADPRIOR, OK

FLAG_FILLED, FLAG_REMOVED = 8, 16
DEFAULTS = dict(occl_radius=1, occl_min=2, fill_radius=1, fill_min=3, fill_inflate=1.0, smooth_radius=1, reg_gate=3.0)


def window(r):
    """The offsets (dv, du) of a (2r+1)^2 window in row-major order."""
    return [(dv, du) for dv in range(-r, r + 1) for du in range(-r, r + 1)]


def shifted(a, dv, du, fill):
    """out[v, u] = a[v + dv, u + du], ``fill`` where that lies outside the image: the neighbour at offset (dv, du) of every pixel."""
    H, W = a.shape
    out = np.full_like(a, fill)
    out[max(0, -dv):min(H, H - dv), max(0, -du):min(W, W - du)] = a[max(0, dv):min(H, H + dv), max(0, du):min(W, W + du)]
    return out


def compat(rk, sk, rj, sj, g2):
    """(rho_k - rho_j)^2 <= reg_gate^2 (s_k + s_j), one rounding per operation."""
    d = rk - rj
    return d * d <= g2 * (sk + sj)


def remove_occluded(rho, s, valid, r, occl_min, g2):
    """Stage 1: the removed pixels.  rho, s hold 1 where not valid."""
    nsup, nocc = np.zeros(rho.shape, int), np.zeros(rho.shape, int)
    for dv, du in window(r):
        if (dv, du) == (0, 0):
            continue
        vk, rk, sk = shifted(valid, dv, du, False), shifted(rho, dv, du, 1.0), shifted(s, dv, du, 1.0)
        c = compat(rk, sk, rho, s, g2)
        nsup += vk & c
        nocc += vk & ~c & (rk > rho)
    return valid & (nocc >= occl_min) & (nocc > nsup)


def fill_holes(rho, s, valid, r, fill_min, inflate, g2):
    """Stage 2: (rho, s, filled) with the holes filled that have a cluster of at least fill_min around their nearest neighbour."""
    has, ra, sa = np.zeros(rho.shape, bool), np.zeros(rho.shape), np.ones(rho.shape)
    for dv, du in window(r):          # the valid neighbour with the largest rho, the first one among equals
        vk, rk, sk = shifted(valid, dv, du, False), shifted(rho, dv, du, 1.0), shifted(s, dv, du, 1.0)
        take = vk & (~has | (rk > ra))
        ra, sa, has = np.where(take, rk, ra), np.where(take, sk, sa), has | vk
    n, Sw, Swr = np.zeros(rho.shape, int), np.zeros(rho.shape), np.zeros(rho.shape)
    for dv, du in window(r):
        vk, rk, sk = shifted(valid, dv, du, False), shifted(rho, dv, du, 1.0), shifted(s, dv, du, 1.0)
        member = has & vk & compat(rk, sk, ra, sa, g2)
        w = 1.0 / sk
        Sw, Swr, n = np.where(member, Sw + w, Sw), np.where(member, Swr + w * rk, Swr), n + member
    filled = ~valid & has & (n >= fill_min)
    mean = Swr / np.where(filled, Sw, 1.0)
    Se = np.zeros(rho.shape)
    for dv, du in window(r):          # the scatter about the mean: a pass of its own
        vk, rk, sk = shifted(valid, dv, du, False), shifted(rho, dv, du, 1.0), shifted(s, dv, du, 1.0)
        member = has & vk & compat(rk, sk, ra, sa, g2)
        e = rk - mean
        Se = np.where(member, Se + (1.0 / sk) * (e * e), Se)
    Swd = np.where(filled, Sw, 1.0)
    var = inflate * (n.astype(np.float64) / Swd + Se / Swd)
    return np.where(filled, mean, rho), np.where(filled, var, s), filled


def smooth(rho, s, valid, r, dist_var, g2):
    """Stage 3: every valid value as the weighted mean of its compatible valid neighbours, itself included."""
    Sw, Swr = np.zeros(rho.shape), np.zeros(rho.shape)
    for dv, du in window(r):
        vk, rk, sk = shifted(valid, dv, du, False), shifted(rho, dv, du, 1.0), shifted(s, dv, du, 1.0)
        member = valid & vk & compat(rk, sk, rho, s, g2)
        w = 1.0 / (sk + dist_var * float(du * du + dv * dv))
        Sw, Swr = np.where(member, Sw + w, Sw), np.where(member, Swr + w * rk, Swr)
    return np.where(valid, Swr / np.where(valid, Sw, 1.0), rho)


def fuse_map(rp, sp, have, depth_next, var_next, gate):
    """dense_ba_prop_f64.fuse_pixel at every pixel at once: (rho_f, s_f, flags, depth float32).  depth_next, var_next: float32 maps or
    None."""
    shape = rp.shape
    if depth_next is None:
        dn, meas, rm, sm = np.zeros(shape, np.float32), np.zeros(shape, bool), np.zeros(shape), np.ones(shape)
    else:
        dn, smf = np.asarray(depth_next, np.float32), np.asarray(var_next, np.float32).astype(np.float64)
        with np.errstate(invalid='ignore'):
            meas = np.isfinite(dn) & (dn > 0) & np.isfinite(smf) & (smf > 0)
        rm, sm = 1.0 / np.where(meas, dn, np.float32(1.0)).astype(np.float64), np.where(meas, smf, 1.0)
    rp, sp = np.where(have, rp, 1.0), np.where(have, sp, 1.0)
    d, tot = rp - rm, sp + sm
    both = have & meas
    gated = both & (gate > 0) & (d * d > gate * gate * tot)
    fused = both & ~gated
    only_m = gated | (meas & ~have)
    rf = np.where(fused, (rp * sm + rm * sp) / tot, np.where(only_m, rm, np.where(have, rp, 0.0)))
    sf = np.where(fused, sp * sm / tot, np.where(only_m, sm, np.where(have, sp, np.nan)))
    flags = (have * FLAG_PROP + meas * FLAG_MEAS + gated * FLAG_GATED).astype(np.uint8)
    depth = np.where(rf > 0, (1.0 / np.where(rf > 0, rf, 1.0)).astype(np.float32), dn)
    return rf, sf, flags, depth


def regularize_reference_link(rho, var, source=None, status=OK, dist_var=0.0, depth_next=None, var_next=None, gate=0.0, occl_radius=1,
                              occl_min=2, fill_radius=1, fill_min=3, fill_inflate=1.0, smooth_radius=1, reg_gate=3.0):
    """islam_depth_regularize for one link.  Returns a dict: inv_depth, var_inv_depth (H,W) float64, depth (H,W) float32, source (H,W)
    int32, flags (H,W) uint8, status, and the stages: valid0, removed, filled, valid2 (bool maps), rho2 and var2 (after stage 2) and
    rho3 (after stage 3), which hold 1 where nothing is valid."""
    rho, var = np.asarray(rho, np.float64), np.asarray(var, np.float64)
    dist_var = float(dist_var)
    st = int(status) if int(status) != OK else (OK if np.isfinite(dist_var) and dist_var >= 0 else BADPRIOR)
    g2 = float(reg_gate) * float(reg_gate)
    with np.errstate(invalid='ignore'):
        valid0 = np.isfinite(rho) & (rho > 0) & np.isfinite(var) & (var > 0)
    if st != OK:
        valid0 = np.zeros(rho.shape, bool)
    r0, s0 = np.where(valid0, rho, 1.0), np.where(valid0, var, 1.0)
    none = np.zeros(rho.shape, bool)
    with np.errstate(all='ignore'):          # where nothing is valid the stages compute on placeholders nobody reads
        removed = remove_occluded(r0, s0, valid0, occl_radius, occl_min, g2) if occl_radius else none
        valid1 = valid0 & ~removed
        r1, s1 = np.where(valid1, r0, 1.0), np.where(valid1, s0, 1.0)
        r2, s2, filled = fill_holes(r1, s1, valid1, fill_radius, fill_min, float(fill_inflate), g2) if fill_radius else (r1, s1, none)
        valid2 = valid1 | filled
        r3 = smooth(r2, s2, valid2, smooth_radius, dist_var, g2) if smooth_radius else r2
    rf, sf, flags, depth = fuse_map(r3, s2, valid2, depth_next, var_next, float(gate))
    flags = flags | (filled * FLAG_FILLED + removed * FLAG_REMOVED).astype(np.uint8)
    src = np.full(rho.shape, -1, np.int32) if source is None else np.where(valid1, np.asarray(source), -1).astype(np.int32)
    return dict(inv_depth=rf, var_inv_depth=sf, depth=depth, source=src, flags=flags, status=st, valid0=valid0, removed=removed, filled=filled,
                valid2=valid2, rho2=r2, var2=s2, rho3=r3)


def regularize_reference(pure, status=None, dist_var=0.0, depth_next=None, var_next=None, gate=0.0, **stages):
    """regularize_reference_link on every link of a pure propagation (a list of propagate_reference_link dicts): a list of dicts.
    dist_var a number or (B,); status (B) or None: the dicts' own."""
    B = len(pure)
    dv = np.broadcast_to(np.asarray(dist_var, np.float64).reshape(-1), (B,))
    return [regularize_reference_link(p['inv_depth'], p['var_inv_depth'], p['source'], p['status'] if status is None else status[b], dv[b],
                                      None if depth_next is None else depth_next[b], None if var_next is None else var_next[b], gate, **stages)
            for b, p in enumerate(pure)]


# ------------------------------------------------------------------------------------------------ the planted leak scene
LEAK_NEAR, LEAK_FAR, LEAK_ROWS, LEAK_COLS = 2.0, 8.0, (6, 18), (12, 28)
LEAK_MOTION = np.array([0.03, -0.02, 0.6, 0, 0, 0, 1.0])


@functools.lru_cache(maxsize=None)
def leak_scene():
    """24 x 40, plane_sequence's intrinsics; a background at 8 m and a patch (rows 6..17, columns 12..27) at 2 m, rho = 1 / depth times
    (1 + 0.002 N(0,1)) from default_rng(5), s = 1e-4; the camera moves (0.03, -0.02, 0.6) m without rotation, so the patch comes to 1.4 m
    and is magnified by 1.43: its splat has holes, and background pixels land in them.  Returns a dict: rho, var, intr, motion, fg (the
    patch among the sources), pure (the pure propagation, a propagate_reference_link dict), interior (the targets strictly inside the
    bounding box of the targets the patch hits), hit_fg, leak (interior targets won by a background source) and hole (interior targets
    on which nothing landed)."""
    H, W = 24, 40
    intr = np.array([0.6 * W, 0.6 * W, (W - 1) / 2.0, (H - 1) / 2.0])
    fg = np.zeros((H, W), bool)
    fg[LEAK_ROWS[0]:LEAK_ROWS[1], LEAK_COLS[0]:LEAK_COLS[1]] = True
    depth = np.where(fg, LEAK_NEAR, LEAK_FAR)
    rho = 1.0 / depth * (1.0 + 0.002 * np.random.default_rng(5).standard_normal((H, W)))
    var = np.full((H, W), 1e-4)
    pure = prop.propagate_reference_link(rho, var, None, LEAK_MOTION, None, intr)
    src = pure['source']
    from_fg = (src >= 0) & fg.ravel()[np.maximum(src, 0)]
    rows, cols = np.flatnonzero(from_fg.any(1)), np.flatnonzero(from_fg.any(0))
    interior = np.zeros((H, W), bool)
    interior[rows[0] + 1:rows[-1], cols[0] + 1:cols[-1]] = True
    return dict(rho=rho, var=var, intr=intr, motion=LEAK_MOTION, fg=fg, pure=pure, interior=interior, hit_fg=interior & from_fg,
                leak=interior & (src >= 0) & ~from_fg, hole=interior & (src < 0))


def leak_counts(sc, reg):
    """What the stages did to the leak scene (reg: a regularize_reference_link dict, or the device's maps under the same names): how
    many pixels were removed, how many of them were leaks, how many interior targets end within 5 % of the patch's inverse depth 1/1.4."""
    flags, rho = np.asarray(reg['flags']), np.asarray(reg['inv_depth'])
    removed = (flags & FLAG_REMOVED) != 0
    near = 1.0 / (LEAK_NEAR - LEAK_MOTION[2])
    at_fg = ((flags & FLAG_PROP) != 0) & (np.abs(rho - near) <= 0.05 * near)
    return dict(removed=int(removed.sum()), removed_leaks=int((removed & sc['leak']).sum()), at_fg=int((at_fg & sc['interior']).sum()))


# ------------------------------------------------------------------------------------------------ the recursive filter, regularised
MODES = dict(fill=dict(DEFAULTS, smooth_radius=0), all=dict(DEFAULTS))


def reg_filter_stats(prior, seq, k):
    """dense_ba_prop_f64.filter_stats with the bits 8 and 16 set aside: a filled pixel that was fused counts as "both, not gated"."""
    return prop.filter_stats(dict(prior, flags=np.asarray(prior['flags']) & 7), seq, k)


@functools.lru_cache(maxsize=None)
def filter_reference_reg(H, W, mode, K=3):
    """dense_ba_prop_f64.filter_reference with the regularisation between the pure propagation and the fusion: link k refines and takes
    the marginal variance as there, propagates into frame k+1 without a measurement, regularises with MODES[mode] and dist_var =
    g_u^2 + g_v^2 of frame k+1 (the squared change of the plane's inverse depth per pixel) and fuses with that frame's stereo map at
    gate 3.  Returns (seq, priors (regularize_reference_link dicts), runs, stats (reg_filter_stats of the last frame))."""
    seq = prop.plane_sequence(H, W, K, PLANE_SEED, PLANE_HOLES)
    depth = seq['stereo'][0]
    sigma = np.full((H, W), SIGMA_STEREO)
    var_next = np.full((H, W), SIGMA_STEREO ** 2, np.float32)
    priors, runs = [], []
    for k in range(K):
        args = (depth, seq['flow'][k], None)
        m = prop.sigma_scale(sigma)
        run = ba_refine_map_reference_link(*args, seq['start'][k], None, seq['intr'], SIGMA_PX ** 2, m, iters=20)
        at = ba_map_reference_link(*args, run['motion'], None, seq['intr'], SIGMA_PX ** 2, m, run['rho'])
        var = SIGMA_PX ** 2 * variance_reference(at, scam_from_sums(at['sums']), True)
        pure = prop.propagate_reference_link(run['rho'], var, None, run['motion'], None, seq['intr'], run['status'], seq['process_var'][k + 1])
        prior = regularize_reference_link(pure['inv_depth'], pure['var_inv_depth'], pure['source'], pure['status'],
                                          float((seq['grad'][k + 1] ** 2).sum()), seq['stereo'][k + 1], var_next, 3.0, **MODES[mode])
        priors.append(prior)
        runs.append(run)
        depth = prior['depth']
        with np.errstate(invalid='ignore'):
            sigma = np.sqrt(prior['var_inv_depth'])
    return seq, priors, runs, reg_filter_stats(priors[-1], seq, K)
