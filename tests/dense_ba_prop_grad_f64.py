"""The float64 restatements of the gradient of depth propagation (include/islam_hip.h, islam_depth_propagate_vjp; DESIGN.md section
3.31), a helper module beside dense_ba_prop_f64.py and not a test file.

propagate_vjp_reference: the closed forms of the header in numpy, on the source and flags a forward pass returned.  Beside every
gradient it returns its scale: the sum of the magnitudes of the element's terms, every difference of the formulas split into its two
products ((rho_m - rho_f) / D into rho_m / D and rho_f / D, J / rho' - 1 / rho into its two quotients, 1 - 2 a rho' / rho likewise, the
cross and quaternion products of the pose chain term by term), which is what a rounding bound is relative to.

restatement_link: the smooth pieces in torch float64, on the same fixed winners and rows, for torch.autograd; its camera_inverse and
quaternion algebra follow dense_ba_prop_f64.camera_inverse operation by operation.

Rounding counts (u = 2^-52, relative to the scale of the element).
K_AD, closed forms against autograd on the same T^-1 bits (asserted by the test): the longest monomial of a pixel gradient is
gr rho_f / D x 2 J s x 2 J (J / rho'): J (4 roundings from a, rho', rho), D (1), rho_f (4), three more factors of J or rho' (4 each) and
nine products and quotients, below 32 on either side, so K_AD = 64.  grad_motion adds the sums over the pixels (pairwise in numpy, any
order in torch: log2(H W) + 8 <= 32 each) and the pose chain (four quaternion or cross products deep, 8 roundings a level on either
side): K_AD_MOTION = 64 + 64 + 64 = 192.
K_GRAD, the device against the closed forms: T^-1 differs (32 roundings an entry), which dense_ba_prop_f64 carries into rho' (K_RHO),
J (2 K_RHO + 20), s' (K_VAR), D (K_VAR + 1) and rho_f (K_FUSE).  The worst monomial above holds rho_f / D, three factors of J and one of
1 / rho': K_FUSE + K_VAR + 1 + 3 (2 K_RHO + 20) + K_RHO, and the 32 of its own evaluation on either side:
K_GRAD = K_FUSE + K_VAR + 7 K_RHO + 128.  The float32 outputs add one float32 rounding of the value.  grad_motion adds the device's
sums (a thread's serial run, six shuffle levels, four waves, 64 rows: below 96), numpy's (32) and the chain on a T^-1 that is 32
roundings off (64 on either side): K_MOTION = K_GRAD + 256."""
import numpy as np
import torch

from oracle import lie
from tests.dense_ba_prop_f64 import K_FUSE, K_RHO, K_VAR, camera_inverse
from tests.dense_reproj_f64 import OK

K_AD = 64
K_AD_MOTION = 192
K_GRAD = K_FUSE + K_VAR + 7 * K_RHO + 128
K_MOTION = K_GRAD + 256
U32 = 2.0 ** -24          # one rounding to float32


# ------------------------------------------------------------------------------------------------ the pose chain
# m = -1: the product as written; m = +1 on the magnitudes of the operands: every term's magnitude added (the scale).
def _cross(a, b, m):
    return np.array([a[1] * b[2] + m * a[2] * b[1], a[2] * b[0] + m * a[0] * b[2], a[0] * b[1] + m * a[1] * b[0]])


def _qact_vjp(q, p, g, m):
    """The cotangents of q and p in p + w uv + u x uv, uv = 2 u x p (lie.quat_act) from the cotangent g of the result."""
    u, w = q[:3], q[3]
    uv = 2.0 * _cross(u, p, m)
    guv = w * g + _cross(g, u, m)
    gu = _cross(uv, g, m) + 2.0 * _cross(p, guv, m)
    return np.append(gu, g @ uv), g + 2.0 * _cross(guv, u, m)


def _qmul_vjp_a(g, b, m):
    return np.array([g[0] * b[3] + m * g[1] * b[2] + g[2] * b[1] + m * g[3] * b[0], g[0] * b[2] + g[1] * b[3] + m * g[2] * b[0] + m * g[3] * b[1],
                     m * g[0] * b[1] + g[1] * b[0] + g[2] * b[3] + m * g[3] * b[2], g[0] * b[0] + g[1] * b[1] + g[2] * b[2] + g[3] * b[3]])


def _qmul_vjp_b(a, g, m):
    return np.array([g[0] * a[3] + g[1] * a[2] + m * g[2] * a[1] + m * g[3] * a[0], m * g[0] * a[2] + g[1] * a[3] + g[2] * a[0] + m * g[3] * a[1],
                     g[0] * a[1] + m * g[1] * a[0] + g[2] * a[3] + m * g[3] * a[2], g[0] * a[0] + g[1] * a[1] + g[2] * a[2] + g[3] * a[3]])


def pose_chain_vjp(motion, rgb2imu, G4, absolute=False):
    """The cotangent G4 of (R20, R21, R22, t_z), (R, t) = camera_inverse(motion, rgb2imu), chained to the plain components [t, q xyzw]
    of motion: (7,).  absolute: the scale instead, the same chain on the magnitudes of every operand with every term added."""
    m = 1.0 if absolute else -1.0
    f = np.abs if absolute else (lambda x: x)
    M = np.asarray(motion, np.float64)
    G4 = np.asarray(G4, np.float64)
    T = M
    if rgb2imu is not None:
        C = np.asarray(rgb2imu, np.float64)
        Ci = lie.se3_inv(C)
        A = lie.se3_mul(Ci, M)
        T = lie.se3_mul(A, C)
    qi, Tt = f(lie.quat_inv(T[3:])), f(T[:3])
    g0, g1, g2 = 2.0 * G4[0], 2.0 * G4[1], 2.0 * G4[2]
    x, y, z, w = qi
    gqi = np.array([g0 * z + g1 * w + m * 2.0 * g2 * x, g1 * z + m * g0 * w + m * 2.0 * g2 * y, g0 * x + g1 * y, g1 * x + m * g0 * y])
    gq, gTt = _qact_vjp(qi, Tt, np.array([0.0, 0.0, m * G4[3]]), m)
    gqi = gqi + gq
    gTq = np.array([m * gqi[0], m * gqi[1], m * gqi[2], gqi[3]])
    if rgb2imu is None:
        return np.concatenate([gTt, gTq])
    gq, _ = _qact_vjp(f(A[3:]), f(C[:3]), gTt, m)
    gAq = gq + _qmul_vjp_a(gTq, f(C[3:]), m)
    _, gMt = _qact_vjp(f(Ci[3:]), f(M[:3]), gTt, m)
    return np.concatenate([gMt, _qmul_vjp_b(f(Ci[3:]), gAq, m)])


# ------------------------------------------------------------------------------------------------ the closed forms
def rows_of(flags, source, status, has_meas):
    """The row of the fusion table of every target, from the forward pass's flags and source (flat bool arrays): both (fused, not
    gated), only_m (measured only, or gated), only_p (propagated only), and prop (a winner's hypothesis is differentiated)."""
    fl, src = np.asarray(flags).ravel().astype(np.int64), np.asarray(source).ravel().astype(np.int64)
    prop = ((fl & 1) != 0) & (src >= 0) & (int(status) == OK)
    meas = ((fl & 2) != 0) & bool(has_meas)
    both = prop & meas & ((fl & 4) == 0)
    return dict(both=both, only_m=meas & ~both, only_p=prop & ~meas, prop=both | (prop & ~meas), src=np.where(prop, src, 0))


def propagate_vjp_reference_link(rho, var, motion, rgb2imu, intr, process_var, depth_next, var_next, source, flags, status, g_rho, g_var):
    """islam_depth_propagate_vjp for one link, numpy float64.  source, flags, status: the forward pass's (propagate_reference_link's);
    g_rho, g_var (H,W) or None: the cotangents of rho_f and s_f, read only where flags is not 0.  Returns a dict: grad_inv_depth,
    grad_var_inv_depth, grad_depth_next, grad_var_next (H,W) float64 (the last two None without a measurement), grad_motion (7), and
    under 'scale' the sums of the magnitudes of every element's terms under the same names; 'pixel_terms' (4): the four pose sums."""
    rho, var = np.asarray(rho, np.float64), np.asarray(var, np.float64)
    H, W = rho.shape
    n = H * W
    has_meas = depth_next is not None
    rw = rows_of(flags, source, status, has_meas)
    both, only_m, only_p, prop, i = rw['both'], rw['only_m'], rw['only_p'], rw['prop'], rw['src']
    any_ = both | only_m | only_p
    cot = lambda g: np.zeros(n) if g is None else np.where(any_, np.asarray(g, np.float64).ravel(), 0.0)
    gr, gs = cot(g_rho), cot(g_var)
    fx, fy, cx, cy = (float(x) for x in intr)
    R, t = camera_inverse(motion, rgb2imu)
    xh, yh = ((i % W).astype(np.float64) - cx) / fx, ((i // W).astype(np.float64) - cy) / fy
    r, s = np.where(prop, rho.ravel()[i], 1.0), np.where(prop, var.ravel()[i], 1.0)
    a = R[2, 0] * xh + R[2, 1] * yh + R[2, 2]
    rp = 1.0 / (a / r + t[2])
    J = a * (rp * rp) / (r * r)
    sp = J * J * s + float(process_var)
    meas = both | only_m
    dn = np.where(meas, np.asarray(depth_next, np.float32).ravel().astype(np.float64), 1.0) if has_meas else np.ones(n)
    sm = np.where(meas, np.asarray(var_next, np.float32).ravel().astype(np.float64), 1.0) if has_meas else np.ones(n)
    rm = 1.0 / dn
    D = sp + sm
    rf = (rp * sm + rm * sp) / D
    wp, wm = sm / D, sp / D
    z = np.zeros(n)
    pick = lambda vb, vp, vm: np.where(both, vb, np.where(only_p, vp, np.where(only_m, vm, 0.0)))
    ag, ags = np.abs(gr), np.abs(gs)
    # the fusion table: value and scale of the cotangents of rho', s', rho_m, s_m
    g_rp, A_rp = pick(gr * wp, gr, z), pick(ag * wp, ag, z)
    g_sp, A_sp = pick(gr * ((rm - rf) / D) + gs * (wp * wp), gs, z), pick(ag * (rm + rf) / D + ags * (wp * wp), ags, z)
    g_rm, A_rm = pick(gr * wm, z, gr), pick(ag * wm, z, ag)
    g_sm, A_sm = pick(gr * ((rp - rf) / D) + gs * (wm * wm), z, gs), pick(ag * (rp + rf) / D + ags * (wm * wm), z, ags)
    # the warp
    ir = 1.0 / r
    g_J, A_J = 2.0 * J * s * g_sp, 2.0 * np.abs(J) * s * A_sp
    rp2 = rp * rp
    G_rho, A_rho = g_rp * J + g_J * (2.0 * J * (J / rp - ir)), A_rp * np.abs(J) + A_J * (2.0 * np.abs(J) * (np.abs(J) / rp + ir))
    G_s, A_s = J * J * g_sp, J * J * A_sp
    G_a = g_J * (rp2 * (ir * ir) * (1.0 - 2.0 * a * rp * ir)) - g_rp * rp2 * ir
    A_a = A_J * (rp2 * (ir * ir) * (1.0 + 2.0 * np.abs(a) * rp * ir)) + A_rp * rp2 * ir
    G_tz, A_tz = g_J * (-2.0 * J * rp) - g_rp * rp2, A_J * (2.0 * np.abs(J) * rp) + A_rp * rp2
    out = dict(grad_inv_depth=np.zeros(n), grad_var_inv_depth=np.zeros(n), grad_depth_next=None, grad_var_next=None)
    scale = dict(grad_inv_depth=np.zeros(n), grad_var_inv_depth=np.zeros(n), grad_depth_next=None, grad_var_next=None)
    out['grad_inv_depth'][i[prop]], out['grad_var_inv_depth'][i[prop]] = G_rho[prop], G_s[prop]          # a winner wins one target
    scale['grad_inv_depth'][i[prop]], scale['grad_var_inv_depth'][i[prop]] = A_rho[prop], A_s[prop]
    if has_meas:
        out['grad_depth_next'], out['grad_var_next'] = -(rm * rm) * g_rm, g_sm
        scale['grad_depth_next'], scale['grad_var_next'] = (rm * rm) * A_rm, A_sm
    on = lambda x: np.where(prop, x, 0.0)
    G4 = np.array([on(G_a * xh).sum(), on(G_a * yh).sum(), on(G_a).sum(), on(G_tz).sum()])
    A4 = np.array([on(A_a * np.abs(xh)).sum(), on(A_a * np.abs(yh)).sum(), on(A_a).sum(), on(A_tz).sum()])
    live = int(status) == OK
    out['grad_motion'] = pose_chain_vjp(motion, rgb2imu, G4) if live else np.zeros(7)
    scale['grad_motion'] = pose_chain_vjp(motion, rgb2imu, A4, absolute=True) if live else np.zeros(7)
    for d in (out, scale):
        for k in ('grad_inv_depth', 'grad_var_inv_depth', 'grad_depth_next', 'grad_var_next'):
            if d[k] is not None:
                d[k] = d[k].reshape(H, W)
    out['scale'], out['pixel_terms'] = scale, G4
    return out


def propagate_vjp_reference(rho, var, motion, rgb2imu, intr, process_var, depth_next, var_next, source, flags, status, g_rho, g_var):
    """propagate_vjp_reference_link for every link of a batch: a list of dicts.  intr (4) or (B,4); process_var a number or (B,)."""
    B = rho.shape[0]
    intr = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (B, 4))
    pv = np.broadcast_to(np.asarray(process_var, np.float64).reshape(-1), (B,))
    at = lambda x, b: None if x is None else x[b]
    return [propagate_vjp_reference_link(rho[b], var[b], motion[b], rgb2imu, intr[b], pv[b], at(depth_next, b), at(var_next, b), source[b], flags[b],
                                         status[b], at(g_rho, b), at(g_var, b)) for b in range(B)]


# ------------------------------------------------------------------------------------------------ the torch restatement
def _t_cross(a, b):
    return torch.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _t_qact(q, p):
    u, w = q[:3], q[3]
    uv = 2.0 * _t_cross(u, p)
    return p + w * uv + _t_cross(u, uv)


def _t_qmul(a, b):
    return torch.stack([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                        a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _t_mul(X, Y):
    return torch.cat([X[:3] + _t_qact(X[3:], Y[:3]), _t_qmul(X[3:], Y[3:])])


def _t_inv(X):
    qi = torch.cat([-X[3:6], X[6:]])
    return torch.cat([-_t_qact(qi, X[:3]), qi])


def torch_camera_inverse(motion, rgb2imu):
    """dense_ba_prop_f64.camera_inverse in torch, operation by operation: (the third row of R (3), t_z)."""
    M = motion
    if rgb2imu is not None:
        C = torch.as_tensor(np.asarray(rgb2imu, np.float64))
        M = _t_mul(_t_mul(_t_inv(C), M), C)
    Ti = _t_inv(M)
    x, y, z, w = Ti[3], Ti[4], Ti[5], Ti[6]
    return torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]), Ti[2]


def restatement_link(rho, var, motion, rgb2imu, intr, process_var, depth_next, var_next, source, flags, status):
    """The smooth pieces of one link in torch float64 on the fixed winners and rows of a forward pass.  rho, var (H,W), motion (7) and,
    with a measurement, depth_next, var_next (H,W) are float64 torch tensors (leaves that may require a gradient; the measurement
    holds the float32 values).  Returns (rho_f, s_f) flat (H W,), 0 and NaN where nothing is known."""
    H, W = rho.shape
    n = H * W
    has_meas = depth_next is not None
    rw = rows_of(flags, source, status, has_meas)
    tb = lambda k: torch.from_numpy(rw[k])
    both, only_m, only_p, prop, i = tb('both'), tb('only_m'), tb('only_p'), tb('prop'), tb('src')
    fx, fy, cx, cy = (float(x) for x in intr)
    R2, tz = torch_camera_inverse(motion, rgb2imu)
    xh, yh = ((i % W).double() - cx) / fx, ((i // W).double() - cy) / fy
    one = torch.ones(n, dtype=torch.float64)
    r, s = torch.where(prop, rho.reshape(-1)[i], one), torch.where(prop, var.reshape(-1)[i], one)
    a = R2[0] * xh + R2[1] * yh + R2[2]
    rp = 1.0 / (a / r + tz)
    J = a * (rp * rp) / (r * r)
    sp = J * J * s + float(process_var)
    meas = both | only_m
    dn = torch.where(meas, depth_next.reshape(-1), one) if has_meas else one
    sm = torch.where(meas, var_next.reshape(-1), one) if has_meas else one
    rm = 1.0 / dn
    D = sp + sm
    zero, nan = torch.zeros(n, dtype=torch.float64), torch.full((n,), float('nan'), dtype=torch.float64)
    rf = torch.where(both, (rp * sm + rm * sp) / D, torch.where(only_p, rp, torch.where(only_m, rm, zero)))
    sf = torch.where(both, sp * sm / D, torch.where(only_p, sp, torch.where(only_m, sm, nan)))
    return rf, sf
