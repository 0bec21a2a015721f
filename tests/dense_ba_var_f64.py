"""The float64 numpy restatement of the joint problem with a per-pixel prior weight map and of the posterior variance of the inverse
depths (include/islam_hip.h, islam_dense_ba_normal_map / _refine_map / _depth_var), a helper module beside
dense_reproj_f64.py and not a test file: the sums with a map (ba_map_reference_link, built on link_front like ba_reference_link), the
joint Levenberg-Marquardt with a map (ba_refine_reference_link driven by it), the variance from the restatement's per-pixel terms
(variance_reference), the explicitly assembled dense system with per-pixel weights, and the two-level scenes.  The CPU test file checks
this module against the inverted dense matrix and on planted scenes; the GPU test file holds the kernels to it."""
import functools
import math

import numpy as np
import pytest

from tests import dense_reproj_f64 as f64
from tests.dense_reproj_f64 import K_ROUND, NSUM, S_COST, S_COUNT, S_G, S_L1, TRIU, _fsum_cols, _seq_cols, _user, body_from_sums, link_front, planted_scene

# Roundings in one term of a camera-frame sum with a map: the 112 of dense_reproj_f64.K_ROUND (rounded up to 128 there) and one more, the
# product w_i = w_b (double)m_i that stands in front of h_dd, g_d and the cost term.
K_MAP = K_ROUND + 1
# Roundings of the longest path through depth_var_pixel_kernel, counted as section 3.25 counted its 112: section 3.23's 64 up to c, r and
# the rows of J_cam, then 1/rho (1), R ray (10), -1/rho^2 (2), jd (8), e (2), w_i (1), h_dd (4), 1/h_dd (1), an entry of h_cam (3), a row
# of S_cam^-1 h with the doubled off-diagonal entries (11), the product with h and the sum over the rows (11), quad / h_dd^2 (2) and the
# final sum (1): 121, rounded up.
K_VAR = 128


def map_as_double(m):
    """The weight map as the kernels read it: float32, widened to float64."""
    return np.asarray(m, np.float32).astype(np.float64)


def ba_map_reference_link(depth, flow, mask, motion, rgb2imu, intr, wb, m, rho=None, kernel=None):
    """ba_reference_link with a weight map m (H,W): the pixel's w_i = wb * (double)(float)m_i takes the place of w, and a pixel has a
    usable prior iff its depth AND its m_i are finite and > 0.  Returns the dict of ba_reference_link and ``w`` (H,W): the pixels'
    weights (1 where the pixel has no prior: nothing reads it there)."""
    z = np.asarray(depth, np.float64)
    m64 = map_as_double(m)
    prior = np.isfinite(z) & (z > 0) & np.isfinite(m64) & (m64 > 0)
    w = np.where(prior, float(wb) * np.where(prior, m64, 1.0), 1.0)
    rho0 = np.where(prior, 1.0 / np.where(prior, z, 1.0), 0.0)
    rho = rho0.copy() if rho is None else np.asarray(rho, np.float64)
    usable = prior & np.isfinite(rho) & (rho > 0)
    rs = np.where(usable, rho, 1.0)
    f = link_front(1.0 / rs, flow, _user(mask, depth.shape) & usable, motion, rgb2imu, intr, kernel)
    A, valid, ru, rv, rob, ju, jv, dR = (f[k] for k in ('A', 'valid', 'ru', 'rv', 'rob', 'ju', 'jv', 'dQ'))
    c = np.where(valid, f['c'], 0.0)
    k = -1.0 / (rs * rs)
    jdu = (f['a'] * dR[..., 0] + f['bq'] * dR[..., 2]) * k
    jdv = (f['cq'] * dR[..., 1] + f['dq'] * dR[..., 2]) * k
    hpd = c[..., None] * (ju * jdu[..., None] + jv * jdv[..., None])
    dprior = rho - rho0
    hdd = c * (jdu * jdu + jdv * jdv) + w
    gd = c * (jdu * ru + jdv * rv) + w * dprior

    sel = valid
    cs, jus, jvs, hs, hds, gds = c[sel], ju[sel], jv[sel], hpd[sel], hdd[sel], gd[sel]
    n = int(sel.sum())
    first = np.zeros((n, NSUM))
    second = np.zeros((n, NSUM))
    first[:, :21] = (cs[:, None, None] * (jus[:, :, None] * jus[:, None, :] + jvs[:, :, None] * jvs[:, None, :]))[:, TRIU[0], TRIU[1]]
    second[:, :21] = (hs[:, :, None] * hs[:, None, :] / hds[:, None, None])[:, TRIU[0], TRIU[1]]
    first[:, S_G:S_G + 6] = cs[:, None] * (jus * ru[sel][:, None] + jvs * rv[sel][:, None])
    second[:, S_G:S_G + 6] = hs * (gds / hds)[:, None]
    first[:, S_COST] = rob[sel]
    second[:, S_COST] = -w[sel] * dprior[sel] ** 2
    first[:, S_L1] = np.abs(ru[sel]) + np.abs(rv[sel])
    first[:, S_COUNT] = 1.0
    terms = first - second
    sums, ab = _fsum_cols(terms), _fsum_cols(np.abs(first) + np.abs(second))
    S, g = body_from_sums(sums, A)
    Sabs, gabs = body_from_sums(ab, np.abs(A))
    Hpp, gp = body_from_sums(_fsum_cols(first), A)
    return dict(sums=sums, abs=ab, fwd=_seq_cols(terms), bwd=_seq_cols(terms[::-1]), S=S, g=g, Sabs=Sabs, gabs=gabs, cost=sums[S_COST],
                l1=sums[S_L1], count=n, A=A, valid=valid, prior=prior, rho0=rho0, rho=rho, hpd=hpd, hdd=hdd, gd=gd, Hpp=Hpp, gp=gp,
                margin=f['margin'], rejects=f['rejects'], c=c, ju=ju, jv=jv, jdu=jdu, jdv=jdv, ru=ru, rv=rv, w=w)


def ba_map_reference(depth, flow, mask, motion, rgb2imu, intr, wb, m, rho=None, kernel=None):
    """ba_map_reference_link for every link of a batch: a list of dicts.  wb: a number or (B,); m (B,H,W)."""
    B = depth.shape[0]
    intr = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (B, 4))
    wb = np.broadcast_to(np.asarray(wb, np.float64).reshape(-1), (B,))
    return [ba_map_reference_link(depth[b], flow[b], None if mask is None else mask[b], motion[b], rgb2imu, intr[b], float(wb[b]), m[b],
                                  None if rho is None else rho[b], kernel) for b in range(B)]


def ba_refine_map_reference_link(depth, flow, mask, motion, rgb2imu, intr, wb, m, **kw):
    """The joint LM of islam_dense_ba_refine_map for one link: ba_refine_reference_link, its evaluation replaced for the length of the
    call by the map restatement closed over m."""
    def with_map(depth, flow, mask, X, rgb2imu, intr, w, rho=None, kernel=None):
        return ba_map_reference_link(depth, flow, mask, X, rgb2imu, intr, w, m, rho, kernel)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(f64, 'ba_reference_link', with_map)
        return f64.ba_refine_reference_link(depth, flow, mask, motion, rgb2imu, intr, wb, **kw)


def scam_from_sums(sums):
    Sc = np.zeros((6, 6))
    Sc[TRIU] = np.asarray(sums)[:21]
    return Sc + np.triu(Sc, 1).T


def variance_reference(r, Scam, marginal, w=None):
    """v (H,W) of section 3.27 from a restatement's dict r (hpd, hdd, valid, prior, rho, and w unless given: a number or (H,W)) and the
    6x6 camera-frame Schur complement Scam:  1/h_dd + h^T Scam^-1 h / h_dd^2 (marginal) or 1/h_dd at a valid pixel, 1/w_i at a pixel
    with a prior that is invalid at the state, NaN without a usable prior or at a rho that is not finite or is <= 0."""
    w = np.broadcast_to(np.asarray(r['w'] if w is None else w, np.float64), r['hdd'].shape)
    usable = r['prior'] & np.isfinite(r['rho']) & (r['rho'] > 0)
    v = np.full(r['hdd'].shape, np.nan)
    v[usable] = 1.0 / w[usable]
    valid = r['valid']
    h, hdd = r['hpd'][valid], r['hdd'][valid]
    v[valid] = 1.0 / hdd
    if marginal:
        v[valid] = 1.0 / hdd + np.einsum('ni,ni->n', h, np.linalg.solve(Scam, h.T).T) / (hdd * hdd)
    return v


def dense_system_map(r):
    """The joint Gauss-Newton matrix assembled explicitly from stacked residual rows, per-pixel weights r['w']: unknowns [xi (6, body
    frame); rho_i of every pixel with a prior], rows sqrt(c) [J_cam A, jd e_i] per valid pixel and component, sqrt(w_i) [0, e_i] per
    prior.  Returns (matrix, the flat indices of the pixels with a prior in the order of its depth columns)."""
    idx = np.flatnonzero(r['prior'].ravel())
    n = idx.size
    flat = lambda a: a.reshape(-1, *a.shape[2:])
    c, ju, jv, jdu, jdv, w = (flat(r[k]) for k in ('c', 'ju', 'jv', 'jdu', 'jdv', 'w'))
    valid = r['valid'].ravel()
    rows = []
    for col, p in enumerate(idx):
        if valid[p]:
            for j, jd in ((ju[p], jdu[p]), (jv[p], jdv[p])):
                row = np.zeros(6 + n)
                row[:6] = math.sqrt(c[p]) * (j @ r['A'])
                row[6 + col] = math.sqrt(c[p]) * jd
                rows.append(row)
        row = np.zeros(6 + n)
        row[6 + col] = math.sqrt(w[p])
        rows.append(row)
    Jb = np.array(rows)
    return Jb.T @ Jb, idx


# ------------------------------------------------------------------------------------------------ the two-level scenes
SIGMA_PX = 0.3
SIGMA_LEVELS = (0.01, 0.03)          # 1/m: the inverse-depth noise on even and on odd columns


def two_level_scene(H, W, seed):
    """planted_scene(H, W, seed) with a prior whose noise has two levels: sigma_i = 0.01 on even columns and 0.03 on odd ones, the depth
    map 1 / (rho_true + sigma N(0,1)) from default_rng(seed + 1000), float32.  Adds sigma (1,H,W), scale = float32(1 / sigma^2) (the map
    beside prior_weight = SIGMA_PX^2, so that w_i = 0.3^2 / sigma_i^2) and w_uniform = 0.3^2 / mean(sigma^2)."""
    sc = planted_scene(H, W, seed)
    sigma = np.broadcast_to(np.where(np.arange(W) % 2 == 0, SIGMA_LEVELS[0], SIGMA_LEVELS[1]), (1, H, W)).copy()
    rho = sc['rho_true'] + sigma * np.random.default_rng(seed + 1000).standard_normal((H, W))
    assert (rho > 0).all()
    return dict(sc, depth=(1.0 / rho).astype(np.float32), sigma=sigma, scale=(1.0 / sigma ** 2).astype(np.float32),
                w_uniform=SIGMA_PX ** 2 / float(np.mean(sigma ** 2)))


TWO_LEVEL_SEED = 0


@functools.lru_cache(maxsize=None)
def two_level_case(H, W):
    """The two-level scene of a size and the restatement's joint refinement of it (20 evaluations from the scene's start): with the map
    in the three summation orders, and with the uniform weight (computed once, shared between the CPU and the GPU tests).  Returns
    (scene, {order: map run}, uniform run, the map restatement evaluated at the map run's final state)."""
    sc = two_level_scene(H, W, TWO_LEVEL_SEED)
    args = (sc['depth'][0], sc['flow'][0], sc['mask'][0], sc['start'][0], None, sc['intr'][0])
    runs = {o: ba_refine_map_reference_link(*args, SIGMA_PX ** 2, sc['scale'][0], iters=20, order=o) for o in ('sums', 'fwd', 'bwd')}
    uniform = f64.ba_refine_reference_link(*args, sc['w_uniform'], iters=20)
    fin = runs['sums']
    at = ba_map_reference_link(sc['depth'][0], sc['flow'][0], sc['mask'][0], fin['motion'], None, sc['intr'][0], SIGMA_PX ** 2, sc['scale'][0],
                               fin['rho'])
    return sc, runs, uniform, at


def chi2_band(n):
    """1 +- 4 sqrt(2 / n): four standard deviations of the mean of n chi-square(1) variables."""
    return 1.0 - 4.0 * math.sqrt(2.0 / n), 1.0 + 4.0 * math.sqrt(2.0 / n)


def rho_rms(rho, sc):
    return float(np.sqrt(np.mean((np.asarray(rho) - sc['rho_true'][0]) ** 2)))
