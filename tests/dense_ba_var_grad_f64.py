"""The float64 restatements of the gradient of the posterior depth variance (include/islam_hip.h, islam_dense_ba_depth_var_vjp;
DESIGN.md section 3.32), a helper module beside dense_ba_var_f64.py and not a test file.

variance_vjp_reference_link: the closed forms of the header in numpy, on the valid set and robust branch of ba_map_reference_link /
variance_reference.  Beside every gradient it returns its scale: the same chain run on the magnitudes of the forward pass's per-pixel
quantities (the rows of J_cam, jd, d, Q, R ray, dr/dQ, r, c, c', S_cam^-1, the cotangent) with every difference of the backward
formulas turned into a sum, i.e. the sum of the magnitudes of the element's terms, every difference split into its two products.

restatement_link: v as a function of (rho, motion, flow) in torch float64 on the same fixed valid set and Huber branch, S_cam recomputed
inside it from the same tensors, for torch.autograd; its camera_inverse and quaternion algebra follow
dense_ba_prop_f64.camera_inverse operation by operation (the helpers of dense_ba_prop_grad_f64).

Rounding counts (u = 2^-52, relative to the scale of the element; S_cam^-1 is accounted for separately by 64 cond(S_cam), as section
3.27 does).  A forward quantity of a pixel carries at most K_VAR = 128 roundings, the count of tests/dense_ba_var_f64.py for the
longest forward path.  The longest monomial of a pixel gradient runs G -> n -> phi_h -> phi_c -> r~ -> Q~ -> rho~:
  g_j [c_j^2 (S^-1 a_j)(S^-1 a_j)^T / h_dd,j^2] . a_i a_i^T  c_i^2 / h_dd,i^2  k_i  2 c'_i r_i  J_q,i  (R ray)_i / rho_i^2
with the forward factors c_j (2), a_j = J^T jd (2 x 2), h_dd,j (2) of the pixel j of the sum and a_i (2 x 2), c_i (2), h_dd,i (2),
k_i = jd.jd (2), c'_i, r_i, an entry of J_q, of R ray, and rho_i^2 (5) of the pixel itself: 23 factors, 23 x 128 = 2944.  The backward
arithmetic itself (matrix-vector products over six entries, the partials of phi, the chain through J_q and Q) stays below 128
roundings on either side (256), and the sum of G over the pixels below 96 on the device (a thread's serial run, six shuffle levels,
four waves, 64 rows) and 32 in numpy (128): K_GRAD = 2944 + 256 + 128 = 3328.  grad_flow, float32, adds one float32 rounding of the
value.  grad_motion adds the sums of the 12 pose terms (96 + 32) and the chain through the quaternion algebra (64 on either side):
K_MOTION = K_GRAD + 256.  The same K_GRAD / K_MOTION serve the comparison of the closed forms with autograd, whose forward values are
its own."""
import numpy as np
import torch

from oracle import lie
from tests import dense_ba_prop_grad_f64 as pg
from tests.dense_ba_var_f64 import K_VAR, ba_map_reference_link
from tests.dense_reproj_f64 import OK, _user, link_front

K_GRAD = 23 * K_VAR + 256 + 128
K_MOTION = K_GRAD + 256
U32 = 2.0 ** -24          # one rounding to float32
NAMES = ('grad_inv_depth', 'grad_flow', 'grad_motion')


# ------------------------------------------------------------------------------------------------ the forward quantities of a link
def link_terms(depth, flow, mask, motion, rgb2imu, intr, wb, m, rho, kernel=None):
    """ba_map_reference_link's dict of one link (m None: ones) with what the backward chain needs beside it, from the same link_front
    call: Q (H,W,3), mray = R ray, d = -R ray / rho^2, fa, fb, fc, fd (dr/dQ), iz, cp, xh, yh, s, and out (H,W) bool: the pixel is on
    the outer branch of a Huber kernel."""
    from islam_amd import robust
    depth = np.asarray(depth)
    m = np.ones(depth.shape, np.float32) if m is None else m
    r = ba_map_reference_link(depth, flow, mask, motion, rgb2imu, intr, wb, m, rho, kernel)
    usable = r['prior'] & np.isfinite(r['rho']) & (r['rho'] > 0)
    rs = np.where(usable, r['rho'], 1.0)
    f = link_front(1.0 / rs, flow, _user(mask, depth.shape) & usable, motion, rgb2imu, intr, kernel)
    assert np.array_equal(f['valid'], r['valid'])
    out = (f['s'] > kernel.delta ** 2) if isinstance(kernel, robust.Huber) else np.zeros(depth.shape, bool)
    Qz = f['Qz']
    r.update(Q=np.stack([f['Qx'], f['Qy'], Qz], -1), mray=f['dQ'], d=-f['dQ'] / (rs * rs)[..., None], fa=f['a'], fb=f['bq'], fc=f['cq'], fd=f['dq'],
             iz=1.0 / Qz, cp=f['cp'], xh=f['ray'][..., 0], yh=f['ray'][..., 1], s=f['s'], out=out & r['valid'], rs=rs, usable=usable)
    return r


# ------------------------------------------------------------------------------------------------ the closed forms
def _chain(F, Sinv, g, s, marginal, zero_G):
    """The backward chain over the N valid pixels.  F: the forward quantities (N,...) and Sinv (6,6), g (N); s = -1: the values,
    s = +1 on the magnitudes of every operand: every term's magnitude added (the scale).  Returns (rho~ (N), flow~ (N,2), the 12 pose
    terms (N,12), G (6,6))."""
    ju, jv, jdu, jdv, c, cp, hdd, ru, rv = (F[k] for k in ('ju', 'jv', 'jdu', 'jdv', 'c', 'cp', 'hdd', 'ru', 'rv'))
    Q, mr, d, fa, fb, fc, fd, iz, rho, xh, yh = (F[k] for k in ('Q', 'mray', 'd', 'fa', 'fb', 'fc', 'fd', 'iz', 'rs', 'xh', 'yh'))
    col = lambda x: x[:, None]
    ih = 1.0 / hdd
    ih2, c2 = ih * ih, c * c
    kk = jdu * jdu + jdv * jdv
    a6 = ju * col(jdu) + jv * col(jdv)
    n6 = np.zeros_like(a6)
    Sa, Gu, Gv, Ga, G = n6, n6, n6, n6, np.zeros((6, 6))
    qq = nn = tau = np.zeros_like(c)
    if marginal:
        Sa = a6 @ Sinv
        y = col(c) * Sa
        if not zero_G:
            G = s * np.einsum('n,ni,nj->ij', g * ih2, y, y)
        Gu, Gv = ju @ G, jv @ G
        Ga = col(jdu) * Gu + col(jdv) * Gv
        qq, nn, tau = (a6 * Sa).sum(1), (a6 * Ga).sum(1), (ju * Gu).sum(1) + (jv * Gv).sum(1)
    ph = c2 * nn * ih2 + s * (g * ih2) + s * (2.0 * g * c2 * qq * (ih2 * ih))
    pc = 2.0 * g * c * qq * ih2 + tau + s * (2.0 * c * nn * ih) + kk * ph
    pk, pq, pn = c * ph, g * c2 * ih2, s * (c2 * ih)
    ab = 2.0 * (col(pq) * Sa + col(pn) * Ga)
    Ju, Jv = col(jdu) * ab + col(2.0 * c) * Gu, col(jdv) * ab + col(2.0 * c) * Gv
    bju, bjv = (ju * ab).sum(1) + 2.0 * pk * jdu, (jv * ab).sum(1) + 2.0 * pk * jdv
    Qx, Qy, Qz = Q[:, 0], Q[:, 1], Q[:, 2]
    ba = bju * d[:, 0] + s * Ju[:, 0] + s * Ju[:, 4] * Qz + Ju[:, 5] * Qy
    bb = bju * d[:, 2] + s * Ju[:, 2] + s * Ju[:, 3] * Qy + Ju[:, 4] * Qx
    bc = bjv * d[:, 1] + s * Jv[:, 1] + Jv[:, 3] * Qz + s * Jv[:, 5] * Qx
    bd = bjv * d[:, 2] + s * Jv[:, 2] + s * Jv[:, 3] * Qy + Jv[:, 4] * Qx
    bru, brv = 2.0 * cp * pc * ru, 2.0 * cp * pc * rv
    bQ = np.stack([Ju[:, 4] * fb + Jv[:, 4] * fd + s * Jv[:, 5] * fc + fa * bru + s * fa * iz * bb,
                   Ju[:, 5] * fa + s * Ju[:, 3] * fb + s * Jv[:, 3] * fd + fc * brv + s * fc * iz * bd,
                   Jv[:, 3] * fc + s * Ju[:, 4] * fa + fb * bru + fd * brv + s * iz * (fa * ba + 2.0 * fb * bb + fc * bc + 2.0 * fd * bd)], 1)
    bd3 = np.stack([bju * fa, bjv * fc, bju * fb + bjv * fd], 1)
    zi = 1.0 / rho
    k2 = zi * zi
    bm = col(zi) * bQ + s * col(k2) * bd3
    g_rho = s * k2 * (bQ * mr).sum(1) + 2.0 * (k2 * zi) * (bd3 * mr).sum(1)
    g_flow = np.stack([s * bru, s * brv], 1)
    pose = np.concatenate([bm[:, [0]] * col(xh), bm[:, [0]] * col(yh), bm[:, [0]], bm[:, [1]] * col(xh), bm[:, [1]] * col(yh), bm[:, [1]],
                           bm[:, [2]] * col(xh), bm[:, [2]] * col(yh), bm[:, [2]], bQ], 1)
    return g_rho, g_flow, pose, G


def _qmat_vjp(q, G, m):
    x, y, z, w = q
    return 2.0 * np.array([(G[1] + G[3]) * y + (G[2] + G[6]) * z + (G[7] + m * G[5]) * w + m * 2.0 * (G[4] + G[8]) * x,
                           (G[1] + G[3]) * x + (G[5] + G[7]) * z + (G[2] + m * G[6]) * w + m * 2.0 * (G[0] + G[8]) * y,
                           (G[2] + G[6]) * x + (G[5] + G[7]) * y + (G[3] + m * G[1]) * w + m * 2.0 * (G[0] + G[4]) * z,
                           (G[7] + m * G[5]) * x + (G[2] + m * G[6]) * y + (G[3] + m * G[1]) * z])


def pose_chain_vjp(motion, rgb2imu, G12, absolute=False):
    """The cotangent G12 of (R row-major (9), t (3)), (R, t) = camera_inverse(motion, rgb2imu), chained to the plain components
    [t, q xyzw] of motion: (7,).  absolute: the scale instead, the same chain on the magnitudes of every operand with every term added."""
    m = 1.0 if absolute else -1.0
    f = np.abs if absolute else (lambda x: x)
    M = np.asarray(motion, np.float64)
    G12 = np.asarray(G12, np.float64)
    T = M
    if rgb2imu is not None:
        C = np.asarray(rgb2imu, np.float64)
        Ci = lie.se3_inv(C)
        A = lie.se3_mul(Ci, M)
        T = lie.se3_mul(A, C)
    qi, Tt = f(lie.quat_inv(T[3:])), f(T[:3])
    gq, gTt = pg._qact_vjp(qi, Tt, m * G12[9:], m)          # ti = -qact(qi, T.t)
    gqi = _qmat_vjp(qi, G12[:9], m) + gq
    gTq = np.array([m * gqi[0], m * gqi[1], m * gqi[2], gqi[3]])
    if rgb2imu is None:
        return np.concatenate([gTt, gTq])
    gq, _ = pg._qact_vjp(f(A[3:]), f(C[:3]), gTt, m)
    gAq = gq + pg._qmul_vjp_a(gTq, f(C[3:]), m)
    _, gMt = pg._qact_vjp(f(Ci[3:]), f(M[:3]), gTt, m)
    return np.concatenate([gMt, pg._qmul_vjp_b(f(Ci[3:]), gAq, m)])


_FIELDS = ('ju', 'jv', 'jdu', 'jdv', 'c', 'cp', 'hdd', 'ru', 'rv', 'Q', 'mray', 'd', 'fa', 'fb', 'fc', 'fd', 'iz', 'rs', 'xh', 'yh')


def variance_vjp_reference_link(r, Scam, marginal, g, motion, rgb2imu, status=OK, zero_G=False):
    """islam_dense_ba_depth_var_vjp for one link, numpy float64.  r: link_terms' dict; Scam (6,6): S_cam of the same state; g (H,W): the
    cotangent of v, read at the valid pixels only; zero_G: the cotangent of S_cam forced to zero (the gradient at a frozen S_cam).
    Returns a dict: grad_inv_depth (H,W), grad_flow (2,H,W), grad_motion (7), under 'scale' the sums of the magnitudes of every
    element's terms under the same names, 'G' (6,6) and 'pose_terms' (12)."""
    H, W = r['valid'].shape
    out = dict(grad_inv_depth=np.zeros((H, W)), grad_flow=np.zeros((2, H, W)), grad_motion=np.zeros(7), G=np.zeros((6, 6)), pose_terms=np.zeros(12))
    scale = dict(grad_inv_depth=np.zeros((H, W)), grad_flow=np.zeros((2, H, W)), grad_motion=np.zeros(7))
    out['scale'] = scale
    sel = r['valid']
    if int(status) != OK or not sel.any():
        return out
    F = {k: np.asarray(r[k], np.float64)[sel] for k in _FIELDS}
    gs = np.asarray(g, np.float64)[sel]
    Sinv = np.linalg.inv(Scam) if marginal else np.zeros((6, 6))
    g_rho, g_flow, pose, G = _chain(F, Sinv, gs, -1.0, marginal, zero_G)
    a_rho, a_flow, a_pose, _ = _chain({k: np.abs(v) for k, v in F.items()}, np.abs(Sinv), np.abs(gs), 1.0, marginal, zero_G)
    out['grad_inv_depth'][sel], scale['grad_inv_depth'][sel] = g_rho, a_rho
    for k in range(2):
        out['grad_flow'][k][sel], scale['grad_flow'][k][sel] = g_flow[:, k], a_flow[:, k]
    G12, A12 = pose.sum(0), a_pose.sum(0)
    out['grad_motion'], scale['grad_motion'] = pose_chain_vjp(motion, rgb2imu, G12), pose_chain_vjp(motion, rgb2imu, A12, absolute=True)
    out['G'], out['pose_terms'] = G, G12
    return out


# ------------------------------------------------------------------------------------------------ the torch restatement
def torch_camera_inverse(motion, rgb2imu):
    """dense_ba_prop_f64.camera_inverse in torch, operation by operation: (R (3,3), t (3))."""
    M = motion
    if rgb2imu is not None:
        C = torch.as_tensor(np.asarray(rgb2imu, np.float64))
        M = pg._t_mul(pg._t_mul(pg._t_inv(C), M), C)
    Ti = pg._t_inv(M)
    x, y, z, w = Ti[3], Ti[4], Ti[5], Ti[6]
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)]),
                     torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)]),
                     torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)])])
    return R, Ti[:3]


def restatement_link(rho, motion, flow, r, rgb2imu, intr, kernel, marginal):
    """v at the valid pixels of one link as a function of rho (H,W), motion (7) and flow (2,H,W), float64 torch tensors (leaves that
    may require a gradient), on the valid set r['valid'] and the Huber branch r['out'] of the forward restatement r (link_terms), the
    weights r['w'] held fixed; S_cam is the sum over the same pixels of the same tensors.  Returns (v (N,), S_cam (6,6))."""
    from islam_amd import robust
    H, W = r['valid'].shape
    fx, fy, cx, cy = (float(x) for x in intr)
    R, t = torch_camera_inverse(motion, rgb2imu)
    sel = torch.from_numpy(r['valid'])
    vv, uu = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    u, v = uu[sel], vv[sel]
    xh, yh = (u - cx) / fx, (v - cy) / fy
    ray = torch.stack([xh, yh, torch.ones_like(xh)], -1)
    rs = rho[sel]
    z = 1.0 / rs
    Q = (z[:, None] * ray) @ R.T + t
    mr = ray @ R.T
    Qx, Qy, Qz = Q[:, 0], Q[:, 1], Q[:, 2]
    ru = fx * (Qx / Qz) + cx - (flow[0][sel] + u)
    rv = fy * (Qy / Qz) + cy - (flow[1][sel] + v)
    s = ru * ru + rv * rv
    if kernel is None:
        c = torch.ones_like(s)
    elif isinstance(kernel, robust.Huber):
        outer = torch.from_numpy(r['out'])[sel]
        c = torch.where(outer, kernel.delta / torch.sqrt(torch.where(outer, s, torch.ones_like(s))), torch.ones_like(s))
    else:
        c = 1.0 / (1.0 + s / kernel.delta ** 2)
    a, bq, cq, dq = fx / Qz, -fx * Qx / Qz ** 2, fy / Qz, -fy * Qy / Qz ** 2
    zero = torch.zeros_like(a)
    ju = torch.stack([-a, zero, -bq, -bq * Qy, bq * Qx - a * Qz, a * Qy], -1)
    jv = torch.stack([zero, -cq, -dq, cq * Qz - dq * Qy, dq * Qx, -cq * Qx], -1)
    k = -1.0 / (rs * rs)
    jdu = (a * mr[:, 0] + bq * mr[:, 2]) * k
    jdv = (cq * mr[:, 1] + dq * mr[:, 2]) * k
    w = torch.from_numpy(np.asarray(r['w'], np.float64))[sel]
    hdd = c * (jdu * jdu + jdv * jdv) + w
    h = c[:, None] * (ju * jdu[:, None] + jv * jdv[:, None])
    S = (c[:, None, None] * (ju[:, :, None] * ju[:, None, :] + jv[:, :, None] * jv[:, None, :]) - h[:, :, None] * h[:, None, :] / hdd[:, None, None]).sum(0)
    vout = 1.0 / hdd
    if marginal:
        vout = vout + (h * torch.linalg.solve(S, h.T).T).sum(1) / (hdd * hdd)
    return vout, S


def used(got, want, scale, k, cond=0.0, extra=0.0):
    """The largest |got - want| / (2^-52 (k + 64 cond) scale + extra |want|) over the elements with terms; the others must be exact zeros."""
    got, want, scale = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(scale, np.float64)
    d = np.abs(got - want)
    none = scale == 0
    assert (got[none] == 0).all() and (want[none] == 0).all()
    bound = 2.0 ** -52 * (k + 64.0 * cond) * scale + extra * np.abs(want)
    return float((d[~none] / bound[~none]).max()) if (~none).any() else 0.0
