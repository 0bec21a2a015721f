"""The float64 restatements of the gradient of the depth regularisation (include/islam_hip.h, islam_depth_regularize_vjp; DESIGN.md
section 3.33), a helper module beside dense_ba_reg_f64.py and not a test file.

regularize_vjp_reference_link: the header's closed forms in numpy on the sets regularize_reference_link found, every window walked
offset by offset in row-major order on all pixels at once (the style of dense_ba_reg_f64).  Beside every gradient it returns its
*scale* (section 3.31's notion): the sum of the magnitudes of the element's terms with every difference split into its products
(e_k = rho_k - mean into |rho_k| + |mean|, s2_j - f e_k^2 into s2_j + f (|rho_k| + |mean|)^2, rho_m - rho_f likewise), and with the
scale of a cotangent that came from a later stage in the place of its magnitude.  A bound is 2^-52 K scale.

regularize_torch_link: the smooth arithmetic of the four stages in torch float64 on the same fixed sets, for torch.autograd.grad.

The two counts K (u = 2^-53 is one rounding; two computations that each err by at most c u scale differ by at most 2^-52 c scale):
  K_DEVICE, device against closed forms.  rho2, s2, rho3 and S_j are the forward's own bits on both sides, so only the derivative terms
  count.  Stage 4, worst element g3s = g_rho ((rho_m - rho_f) / D) + g_s (s_m / D)^2: rho_m 1, D 1, rho_f 4 more, the difference 1, the
  quotient 1, the product 1 (10 with D); the other term 6; their sum 1: 11.  Stage 3, per term: w 3, q = g3 w / S 2, then q w (rho2_k -
  rho3_j) 6 more; a window's sum of at most 25 terms and the start value 25: 11 + 5 + 6 + 25 = 47.  Stage 2, per term: w 1, w / S 2, e
  1; g2s_j (w (w / S) (s2_j - f e e)) 11, the sum of two terms per cell over at most 25 cells 50: 47 + 11 + 50 = 108.
  K_AUTOGRAD, closed forms against autograd.  Autograd differentiates every quotient through its numerator and its denominator
  apart, two chains where a closed form has one term, and carries the terms through the mean inside the scatter, which sum to zero
  and which the closed forms drop; the split scale bounds the magnitude of each of these.  At most twice the count above: 216."""
import numpy as np
import torch

from tests import dense_ba_reg_f64 as reg
from tests.dense_ba_reg_f64 import FLAG_GATED, FLAG_MEAS, FLAG_PROP, compat, shifted, window

K_DEVICE, K_AUTOGRAD = 108, 216
U52, U24 = 2.0 ** -52, 2.0 ** -24
STAGE_KEYS = ('occl_radius', 'occl_min', 'fill_radius', 'fill_min', 'fill_inflate', 'smooth_radius', 'reg_gate')


def cluster_maps(r1, s1, valid1, r, g2):
    """Stage 2's choices at every pixel as dense_ba_reg_f64.fill_holes makes them: (has, ra, sa, n, Sw), the anchor and the size and
    sum of weights of the cluster around it.  r1, s1 hold 1 where not valid1."""
    has, ra, sa = np.zeros(r1.shape, bool), np.zeros(r1.shape), np.ones(r1.shape)
    for dv, du in window(r):
        vk, rk, sk = shifted(valid1, dv, du, False), shifted(r1, dv, du, 1.0), shifted(s1, dv, du, 1.0)
        take = vk & (~has | (rk > ra))
        ra, sa, has = np.where(take, rk, ra), np.where(take, sk, sa), has | vk
    n, Sw = np.zeros(r1.shape, int), np.zeros(r1.shape)
    for dv, du in window(r):
        vk, rk, sk = shifted(valid1, dv, du, False), shifted(r1, dv, du, 1.0), shifted(s1, dv, du, 1.0)
        member = has & vk & compat(rk, sk, ra, sa, g2)
        Sw, n = np.where(member, Sw + 1.0 / sk, Sw), n + member
    return has, ra, sa, n, Sw


def smooth_weight_sums(r2, s2, valid2, r, dist_var, g2):
    """S_j of stage 3 in the forward's order (1 where not valid2)."""
    Sw = np.zeros(r2.shape)
    for dv, du in window(r):
        vk, rk, sk = shifted(valid2, dv, du, False), shifted(r2, dv, du, 1.0), shifted(s2, dv, du, 1.0)
        member = valid2 & vk & compat(rk, sk, r2, s2, g2)
        Sw = np.where(member, Sw + 1.0 / (sk + dist_var * float(du * du + dv * dv)), Sw)
    return np.where(valid2, Sw, 1.0)


def fusion_rows(ref, flags, has_meas):
    """The row of the fusion table per pixel as the kernel reads it from ``flags``: (prop, meas, gated) bool maps."""
    f = np.asarray(flags).astype(int) & (FLAG_PROP | FLAG_MEAS | FLAG_GATED)
    f = np.where(ref['valid2'], f, f & FLAG_MEAS)
    if not has_meas:
        f = f & ~(FLAG_MEAS | FLAG_GATED)
    return (f & FLAG_PROP) != 0, (f & FLAG_MEAS) != 0, (f & FLAG_GATED) != 0


def regularize_vjp_reference_link(ref, flags, dist_var=0.0, depth_next=None, var_next=None, grad_inv_depth=None, grad_var_inv_depth=None,
                                  occl_radius=1, occl_min=2, fill_radius=1, fill_min=3, fill_inflate=1.0, smooth_radius=1, reg_gate=3.0):
    """islam_depth_regularize_vjp for one link.  ref: regularize_reference_link's dict for the same inputs and stage arguments (its
    sets and its stage values rho2, var2, rho3; a link with a status has empty sets); flags: the forward pass's.  Cotangents (H,W) or
    None (zero), read only where the row says something is known.  Returns a dict: grad_inv_depth, grad_var_inv_depth (float64),
    grad_depth_next, grad_var_next (float64, before the float32 rounding; None without a measurement), scale_* beside each, and
    n_fill_terms (how many (filled j, source k) pairs pass a gradient)."""
    g2, f = float(reg_gate) * float(reg_gate), float(fill_inflate)
    valid1, filled, valid2 = ref['valid0'] & ~ref['removed'], ref['filled'], ref['valid2']
    r2, s2, r3 = ref['rho2'], ref['var2'], ref['rho3']
    shape = r2.shape
    has_meas = depth_next is not None
    prop, meas, gated = fusion_rows(ref, flags, has_meas)
    known = prop | meas
    with np.errstate(all='ignore'):
        gr = np.where(known, 0.0 if grad_inv_depth is None else grad_inv_depth, 0.0)
        gs = np.where(known, 0.0 if grad_var_inv_depth is None else grad_var_inv_depth, 0.0)
        # ---- stage 4
        rm = 1.0 / np.where(meas, np.asarray(depth_next, np.float32), np.float32(1.0)).astype(np.float64) if has_meas else np.ones(shape)
        sm = np.where(meas, np.asarray(var_next, np.float32).astype(np.float64), 1.0) if has_meas else np.ones(shape)
        fused, only_m, only_p = prop & meas & ~gated, meas & ~(prop & ~gated), prop & ~meas
        D = s2 + sm
        rf, wp, wm = (r3 * sm + rm * s2) / D, sm / D, s2 / D
        arf = (np.abs(r3) * sm + rm * s2) / D
        g3r = np.where(fused, gr * wp, np.where(only_p, gr, 0.0))
        c3r = np.abs(g3r)
        g3s = np.where(fused, gr * ((rm - rf) / D) + gs * (wp * wp), np.where(only_p, gs, 0.0))
        c3s = np.where(fused, np.abs(gr) * ((rm + arf) / D) + np.abs(gs) * (wp * wp), np.abs(g3s))
        g_rm = np.where(fused, gr * wm, np.where(only_m, gr, 0.0))
        g_sm = np.where(fused, gr * ((r3 - rf) / D) + gs * (wm * wm), np.where(only_m, gs, 0.0))
        c_sm = np.where(fused, np.abs(gr) * ((np.abs(r3) + arf) / D) + np.abs(gs) * (wm * wm), np.abs(g_sm))
        gdn, cdn = -(rm * rm) * g_rm, (rm * rm) * np.abs(g_rm)
        # ---- stage 3, gathered at k over j = k + (dv, du)
        if smooth_radius:
            S = smooth_weight_sums(r2, s2, valid2, smooth_radius, float(dist_var), g2)
            g2r, c2r, g2s, c2s = np.zeros(shape), np.zeros(shape), g3s.copy(), c3s.copy()
            for dv, du in window(smooth_radius):
                vj, rj, sj = shifted(valid2, dv, du, False), shifted(r2, dv, du, 1.0), shifted(s2, dv, du, 1.0)
                member = valid2 & vj & compat(r2, s2, rj, sj, g2)
                w = 1.0 / (s2 + float(dist_var) * float(du * du + dv * dv))
                Sj, r3j = shifted(S, dv, du, 1.0), shifted(r3, dv, du, 1.0)
                q, cq = shifted(g3r, dv, du, 0.0) * w / Sj, shifted(c3r, dv, du, 0.0) * w / Sj
                g2r, c2r = np.where(member, g2r + q, g2r), np.where(member, c2r + cq, c2r)
                g2s, c2s = np.where(member, g2s - q * w * (r2 - r3j), g2s), np.where(member, c2s + cq * w * (np.abs(r2) + np.abs(r3j)), c2s)
        else:
            g2r, c2r, g2s, c2s = g3r, c3r, g3s, c3s
        # ---- stage 2, gathered at a valid1 k over the filled j = k + (dv, du)
        g1r, c1r, g1s, c1s = g2r.copy(), c2r.copy(), g2s.copy(), c2s.copy()
        n_terms = 0
        if fill_radius:
            r1, s1 = np.where(valid1, r2, 1.0), np.where(valid1, s2, 1.0)      # a valid1 pixel keeps its input through stage 2
            _, ra, sa, _, Sf = cluster_maps(r1, s1, valid1, fill_radius, g2)
            w = 1.0 / s1
            for dv, du in window(fill_radius):
                fj = shifted(filled, dv, du, False)
                member = valid1 & fj & compat(r1, s1, shifted(ra, dv, du, 1.0), shifted(sa, dv, du, 1.0), g2)
                n_terms += int(member.sum())
                mj, s2j = shifted(r2, dv, du, 1.0), shifted(s2, dv, du, 1.0)
                e, ae, wS = r1 - mj, np.abs(r1) + np.abs(mj), w / np.where(fj, shifted(Sf, dv, du, 1.0), 1.0)
                ar, cr, as_, cs = (shifted(a, dv, du, 0.0) for a in (g2r, c2r, g2s, c2s))
                g1r = np.where(member, g1r + (ar * wS + as_ * (2.0 * f * e * wS)), g1r)
                c1r = np.where(member, c1r + (cr * wS + cs * (2.0 * f * ae * wS)), c1r)
                g1s = np.where(member, g1s + (as_ * (w * wS * (s2j - f * (e * e))) - ar * (w * wS * e)), g1s)
                c1s = np.where(member, c1s + (cs * (w * wS * (s2j + f * (ae * ae))) + cr * (w * wS * ae)), c1s)
    z = np.zeros(shape)
    out = dict(grad_inv_depth=np.where(valid1, g1r, z), grad_var_inv_depth=np.where(valid1, g1s, z), scale_inv_depth=np.where(valid1, c1r, z),
               scale_var_inv_depth=np.where(valid1, c1s, z), grad_depth_next=None, grad_var_next=None, scale_depth_next=None,
               scale_var_next=None, n_fill_terms=n_terms, valid1=valid1, rows=(prop, meas, gated))
    if has_meas:
        out.update(grad_depth_next=gdn, grad_var_next=g_sm, scale_depth_next=cdn, scale_var_next=c_sm)
    return out


def _tshift(a, dv, du, r):
    H, W = a.shape
    return torch.nn.functional.pad(a, (r, r, r, r), value=1.0)[r + dv:r + dv + H, r + du:r + du + W]


def regularize_torch_link(rho, var, ref, flags, dist_var=0.0, depth_next=None, var_next=None, occl_radius=1, occl_min=2, fill_radius=1,
                          fill_min=3, fill_inflate=1.0, smooth_radius=1, reg_gate=3.0):
    """The smooth arithmetic of islam_depth_regularize on the fixed sets of ``ref`` in torch float64: rho, var (H,W) tensors that hold
    any finite value where ref['valid0'] is False, depth_next, var_next float32 tensors or None.  Every decision (the sets, compat,
    the anchors, the row of the fusion table) is taken from numpy values and enters as a constant mask.  Returns (rho_f, s_f), zeros
    where nothing is known."""
    g2, f = float(reg_gate) * float(reg_gate), float(fill_inflate)
    T = lambda m: torch.from_numpy(np.ascontiguousarray(m))
    valid1n, filledn, valid2n = ref['valid0'] & ~ref['removed'], ref['filled'], ref['valid2']
    r2n, s2n = ref['rho2'], ref['var2']
    one = torch.ones_like(rho)
    r1, s1 = torch.where(T(valid1n), rho, one), torch.where(T(valid1n), var, one)
    r2, s2 = r1, s1
    if fill_radius:
        r1n, s1n = np.where(valid1n, r2n, 1.0), np.where(valid1n, s2n, 1.0)
        has, ra, sa, n, _ = cluster_maps(r1n, s1n, valid1n, fill_radius, g2)
        members = []
        for dv, du in window(fill_radius):
            vk, rk, sk = shifted(valid1n, dv, du, False), shifted(r1n, dv, du, 1.0), shifted(s1n, dv, du, 1.0)
            members.append(T(filledn & has & vk & compat(rk, sk, ra, sa, g2)))
        Sw, Swr = torch.zeros_like(rho), torch.zeros_like(rho)
        for m, (dv, du) in zip(members, window(fill_radius)):
            rk, sk = _tshift(r1, dv, du, fill_radius), _tshift(s1, dv, du, fill_radius)
            Sw, Swr = Sw + torch.where(m, 1.0 / sk, 0 * one), Swr + torch.where(m, rk / sk, 0 * one)
        Swd = torch.where(T(filledn), Sw, one)
        mean = Swr / Swd
        Se = torch.zeros_like(rho)
        for m, (dv, du) in zip(members, window(fill_radius)):
            rk, sk = _tshift(r1, dv, du, fill_radius), _tshift(s1, dv, du, fill_radius)
            Se = Se + torch.where(m, (rk - mean) ** 2 / sk, 0 * one)
        r2 = torch.where(T(filledn), mean, r1)
        s2 = torch.where(T(filledn), f * (T(n.astype(np.float64)) / Swd + Se / Swd), s1)
    r3 = r2
    if smooth_radius:
        num, den = torch.zeros_like(rho), torch.zeros_like(rho)
        for dv, du in window(smooth_radius):
            vk, rk, sk = shifted(valid2n, dv, du, False), shifted(r2n, dv, du, 1.0), shifted(s2n, dv, du, 1.0)
            m = T(valid2n & vk & compat(rk, sk, r2n, s2n, g2))
            w = 1.0 / (_tshift(s2, dv, du, smooth_radius) + float(dist_var) * float(du * du + dv * dv))
            num, den = num + torch.where(m, w * _tshift(r2, dv, du, smooth_radius), 0 * one), den + torch.where(m, w, 0 * one)
        r3 = torch.where(T(valid2n), num / torch.where(T(valid2n), den, one), r2)
    prop, meas, gated = fusion_rows(ref, flags, depth_next is not None)
    fused, only_m, only_p = T(prop & meas & ~gated), T(meas & ~(prop & ~gated)), T(prop & ~meas)
    if depth_next is not None:
        rm = 1.0 / torch.where(T(meas), depth_next, torch.ones_like(depth_next)).double()
        sm = torch.where(T(meas), var_next, torch.ones_like(var_next)).double()
    else:
        rm, sm = one, one
    tot = s2 + sm
    zero = 0 * one
    rf = torch.where(fused, (r3 * sm + rm * s2) / tot, torch.where(only_m, rm, torch.where(only_p, r3, zero)))
    sf = torch.where(fused, s2 * sm / tot, torch.where(only_m, sm, torch.where(only_p, s2, zero)))
    return rf, sf


def share(name, got, want, scale, K, extra=None):
    """The largest |got - want| / bound over the elements, bound = 2^-52 K scale (+ extra); an element with a zero bound must agree
    exactly.  Prints the figure (the tests' tables) and returns it."""
    got, want, scale = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(scale, np.float64)
    bound = U52 * K * scale + (0.0 if extra is None else extra)
    diff = np.abs(got - want)
    assert np.isfinite(diff).all(), name
    exact = bound == 0
    assert np.array_equal(got[exact], want[exact]), name
    s = float((diff[~exact] / bound[~exact]).max()) if (~exact).any() else 0.0
    print('%s: share of the bound %.3f (K %d), max |grad| %.3e' % (name, s, K, float(np.abs(want).max())))
    return s
