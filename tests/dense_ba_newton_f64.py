"""The float64 numpy restatement of the joint refinement's gradient with the exact (Newton) Hessian and per-pixel prior weights
(include/islam_hip.h, islam_dense_ba_newton_weights / islam_dense_ba_newton_vjp), a helper module beside
dense_ba_grad_f64.py and not a test file.  Built on dense_reproj_f64's ba_reference_link and link_front, with a weight map on
dense_ba_var_f64's ba_map_reference_link: the exact per-pixel blocks n_pp, n_pd, n_dd with the Gauss-Newton fallback
(newton_blocks_link), the camera-frame sums of S_N and u_cam with the sum of the magnitudes of their parts, lambda_p and lambda_d
(newton_adjoint_reference_link), the gradient of Phi = lambda^T G in depth and flow with per-element sum|term|
(newton_vjp_reference_link), their composition (newton_implicit_gradient) and the batch form with the status rule
(newton_implicit_gradient_batch).  tests/test_dense_ba_newton_cpu.py checks this module against second central differences of the
cost, an explicitly assembled system and re-refinement; tests/test_dense_ba_newton_gpu.py holds the kernels to it."""
import numpy as np

from tests.dense_ba_var_f64 import ba_map_reference_link
from tests.dense_reproj_f64 import TRIU, _fsum_cols, _user, ba_reference_link, link_front, tangent_from_pose_grad

# Roundings in one term of a camera-frame sum of S_N or u_cam, counted from ba_newton_partial_kernel's arithmetic as section 3.25 counts
# its 112: section 3.23's 64 for everything up to c, c', r and dr/dQ, then 1/rho (1), R ray (10), -1/rho^2 and d (5), w_i (1), M (8),
# y and n (7), an entry of J_q^T M J_q (8), of B (3), K (1), K d (5), d.K d, n.d, 2/rho and n_dd (15), 1/n_dd (1), an entry of K D_p
# (5), of D_p^T K D_p (5), of C (6), of n_pd with n x d (10), the Schur term and the sum (4): 159, rounded up.
K_NEWTON = 192


def _skew(v):
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _front(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel, m):
    """The joint restatement at (motion, rho) (with the map m when given), the link_front call it makes, and the pixels' weights."""
    if m is None:
        r = ba_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel)
        wmap = np.full(depth.shape, float(w))
    else:
        r = ba_map_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, m, rho, kernel)
        wmap = r['w']
    usable = r['prior'] & np.isfinite(r['rho']) & (r['rho'] > 0)
    f = link_front(1.0 / np.where(usable, r['rho'], 1.0), flow, _user(mask, depth.shape) & usable, motion, rgb2imu, intr, kernel)
    assert np.array_equal(f['valid'], r['valid'])
    return r, f, wmap


def _blocks(Jq, M, y, Q, d, rho, w, iz, mag):
    """n_pp (N,6,6), n_pd (N,6), n_dd (N) and n from the header's formulas.  mag: every product taken positive (the arguments are then
    the magnitudes of the leaves), which gives the sum of the magnitudes of the parts."""
    sg = 1.0 if mag else -1.0
    N = Q.shape[0]
    n = np.einsum('nki,nk->ni', Jq, y)
    K = np.einsum('nki,nkl,nlj->nij', Jq, M, Jq)
    Bm = np.zeros((N, 3, 3))
    Bm[:, :, 2] += n
    Bm[:, 2, :] += n
    K = K + sg * iz[:, None, None] * Bm
    X = np.abs(_skew(Q)) if mag else _skew(Q)
    Dp = np.concatenate([np.broadcast_to(sg * np.eye(3), (N, 3, 3)), X], -1)
    C = np.zeros((N, 6, 6))
    sn = np.abs(_skew(n)) if mag else _skew(n)
    C[:, :3, 3:] = 0.5 * sn
    C[:, 3:, :3] = 0.5 * (sn if mag else -sn)
    nQ = np.einsum('ni,ni->n', n, Q)
    C[:, 3:, 3:] = 0.5 * (n[:, :, None] * Q[:, None, :] + Q[:, :, None] * n[:, None, :]) + sg * nQ[:, None, None] * np.eye(3)
    Kd = np.einsum('nij,nj->ni', K, d)
    npp = np.einsum('nki,nkl,nlj->nij', Dp, K, Dp) + C
    nxd = np.einsum('nij,nj->ni', sn, d)          # n x d
    npd = np.einsum('nki,nk->ni', Dp, Kd) + np.concatenate([np.zeros((N, 3)), nxd], -1)
    ndd = np.einsum('ni,ni->n', d, Kd) + sg * (2.0 / rho) * np.einsum('ni,ni->n', n, d) + w
    return npp, npd, ndd


def newton_blocks_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel=None, m=None):
    """The exact blocks of one link at the state (motion, rho), camera frame, over the whole image: npp (H,W,6,6), npd (H,W,6), ndd (H,W)
    (at a pixel with a prior that is invalid at the state npp = npd = 0 and ndd = w_i; without a usable prior everything is 0),
    fallback (H,W) bool: the valid pixels whose exact n_dd is not > 0 and which carry the Gauss-Newton blocks c J_cam^T J_cam, h_pd,
    h_dd instead, ndd_exact (H,W; the exact n_dd before the fallback, NaN outside the valid set) and ndd_parts (H,W; the sum of the
    magnitudes of its parts), the same blocks from the magnitudes of the leaves (npp_abs, npd_abs; ndd_amp = sum|parts of n_dd| /
    |n_dd| >= 1, what a rounding of n_dd's parts is amplified by in 1 / n_dd), gn = dict(npp, npd, ndd): the Gauss-Newton blocks of
    every pixel, and r, f, w: the restatements underneath and the pixels' weights."""
    r, f, wmap = _front(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel, m)
    Hh, Ww = depth.shape
    valid = r['valid']
    a, bq, cq, dq, c, cp, ru, rv, Qz = (f[k][valid] for k in ('a', 'bq', 'cq', 'dq', 'c', 'cp', 'ru', 'rv', 'Qz'))
    Q = np.stack([f['Qx'][valid], f['Qy'][valid], Qz], -1)
    rs = r['rho'][valid]
    d = -f['dQ'][valid] / (rs * rs)[:, None]
    zero = np.zeros_like(a)
    Jq = np.stack([np.stack([a, zero, bq], -1), np.stack([zero, cq, dq], -1)], -2)
    rr = np.stack([ru, rv], -1)
    M = c[:, None, None] * np.eye(2) + 2.0 * cp[:, None, None] * rr[:, :, None] * rr[:, None, :]
    ww = wmap[valid]
    npp, npd, ndd = _blocks(Jq, M, c[:, None] * rr, Q, d, rs, ww, 1.0 / Qz, False)
    Mabs = c[:, None, None] * np.eye(2) + 2.0 * np.abs(cp)[:, None, None] * np.abs(rr[:, :, None] * rr[:, None, :])
    app, apd, add = _blocks(np.abs(Jq), Mabs, c[:, None] * np.abs(rr), np.abs(Q), np.abs(d), rs, ww, 1.0 / Qz, True)
    # the Gauss-Newton blocks of section 3.25
    Jc = np.stack([r['ju'][valid], r['jv'][valid]], -2)
    gpp = c[:, None, None] * np.einsum('nki,nkj->nij', Jc, Jc)
    gpd, gdd = r['hpd'][valid], r['hdd'][valid]
    fb = ~(ndd > 0)
    exact = ndd.copy()
    jd = np.stack([r['jdu'][valid], r['jdv'][valid]], -1)
    gapp = c[:, None, None] * np.einsum('nki,nkj->nij', np.abs(Jc), np.abs(Jc))
    gapd = c[:, None] * np.einsum('nki,nk->ni', np.abs(Jc), np.abs(jd))
    npp, npd, ndd = np.where(fb[:, None, None], gpp, npp), np.where(fb[:, None], gpd, npd), np.where(fb, gdd, ndd)
    app, apd = np.where(fb[:, None, None], gapp, app), np.where(fb[:, None], gapd, apd)
    amp = np.where(fb, 1.0, add / np.abs(np.where(fb, 1.0, ndd)))

    def image(x, fill=0.0):
        full = np.full((Hh, Ww) + x.shape[1:], fill)
        full[valid] = x
        return full

    ndd_img = image(ndd)
    off = r['prior'] & ~valid
    ndd_img[off] = wmap[off]
    gn = dict(npp=image(gpp), npd=image(gpd), ndd=image(gdd))
    return dict(npp=image(npp), npd=image(npd), ndd=ndd_img, fallback=image(fb, False).astype(bool), ndd_exact=image(exact, np.nan),
                ndd_parts=image(add, np.nan), npp_abs=image(app), npd_abs=image(apd), ndd_amp=image(amp, 1.0), gn=gn, r=r, f=f, w=wmap,
                valid=valid, prior=r['prior'], A=r['A'], count=r['count'])


def _sym(tri):
    S = np.zeros((6, 6))
    S[TRIU] = tri
    return S + np.triu(S, 1).T


def newton_adjoint_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, v_p, v_d=None, kernel=None, m=None, S=None, blocks=None):
    """The adjoint solve N lambda = -v of one link with the exact Hessian N, by per-pixel elimination.  Arguments of
    ba_adjoint_reference_link plus m (H,W) or None: the weight map; S (6,6) or None: the body-frame S_N to solve with (None: the
    restatement's own); blocks: newton_blocks_link's dict at this state when the caller has it.  Returns a dict: s_cam (21: the upper
    triangle of S_N,cam, each the correctly rounded sum of its terms), s_abs (21: the sum over the pixels of the magnitudes of the parts),
    u_cam, u_abs (6), fallback (the count), S (body frame), lam_p, lam_cam, lam_d (H,W), A, valid, prior, count, blocks."""
    k = newton_blocks_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel, m) if blocks is None else blocks
    v_d = np.zeros(depth.shape) if v_d is None else np.asarray(v_d, np.float64)
    sel, A = k['valid'], k['A']
    npp, npd, ndd, amp = k['npp'][sel], k['npd'][sel], k['ndd'][sel], k['ndd_amp'][sel]
    app, apd = k['npp_abs'][sel], k['npd_abs'][sel]
    if 's_cam' not in k:          # the sums of S_N,cam do not depend on v: computed once per state (sums of magnitudes need no fsum)
        first = npp[:, TRIU[0], TRIU[1]]
        second = (npd[:, :, None] * npd[:, None, :] / ndd[:, None, None])[:, TRIU[0], TRIU[1]]
        k['s_cam'] = _fsum_cols(first - second)
        k['s_abs'] = (app[:, TRIU[0], TRIU[1]] + (apd[:, :, None] * apd[:, None, :] * (amp / np.abs(ndd))[:, None, None])[:, TRIU[0], TRIU[1]]).sum(0)
    s_cam, s_abs = k['s_cam'], k['s_abs']
    kk = v_d[sel] / ndd
    u = _fsum_cols(npd * kk[:, None]) if v_d.any() else np.zeros(6)
    u_abs = (apd * (np.abs(kk) * amp)[:, None]).sum(0)
    SN = A.T @ _sym(s_cam) @ A
    S = SN if S is None else np.asarray(S, np.float64)
    lam_p = -np.linalg.solve(S, np.asarray(v_p, np.float64) - A.T @ u)
    lam_cam = A @ lam_p
    return dict(s_cam=s_cam, s_abs=s_abs, u_cam=u, u_abs=u_abs, fallback=int(k['fallback'].sum()), S=S, S_own=SN, lam_p=lam_p, lam_cam=lam_cam,
                lam_d=newton_lambda_d(k, lam_cam, v_d), A=A, valid=sel, prior=k['prior'], count=k['count'], blocks=k)


def newton_lambda_d(k, lam_cam, v_d):
    """lambda_d = -(v_d + n_pd^T lambda_cam) / n_dd at every pixel with a prior (n_pd = 0, n_dd = w_i at an invalid one), 0 elsewhere."""
    with np.errstate(all='ignore'):
        ld = -(v_d + k['npd'] @ lam_cam) / np.where(k['prior'], k['ndd'], 1.0)
    return np.where(k['prior'], ld, 0.0)


def newton_vjp_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, lam_p, v_d=None, kernel=None, m=None, blocks=None):
    """dPhi/d(depth, flow) of one link, Phi = lam_p^T g_p + sum lam_d g_d with the state, lambda and the valid set held fixed: section
    3.26's data gradient with lambda_d from the exact n_pd, n_dd.  Returns ba_vjp_reference_link's dict: grad_depth = w_i lam_d /
    depth^2, grad_flow = -(c q + 2 c' (q.r) r), abs_depth, abs_flow (per element the sum of |term|, the products of lambda_d included:
    (|v_d| + |n_pd|_parts . |lambda_cam|) / |n_dd| times n_dd's amplification), lam_d, valid, prior, s."""
    k = newton_blocks_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, kernel, m) if blocks is None else blocks
    r, f, wmap = k['r'], k['f'], k['w']
    v_d = np.zeros(depth.shape) if v_d is None else np.asarray(v_d, np.float64)
    valid, prior = k['valid'], k['prior']
    lam_cam = k['A'] @ np.asarray(lam_p, np.float64)
    lam_d = newton_lambda_d(k, lam_cam, v_d)
    z = np.where(prior, np.asarray(depth, np.float64), 1.0)
    grad_depth = np.where(prior, wmap * lam_d / (z * z), 0.0)
    la = np.abs(lam_cam)
    a, bq, cq, dq, Qx, Qy, Qz = (np.abs(f[x]) for x in ('a', 'bq', 'cq', 'dq', 'Qx', 'Qy', 'Qz'))
    zero = np.zeros_like(a)
    with np.errstate(all='ignore'):          # an invalid pixel may hold anything
        c, cp, ru, rv = r['c'], np.where(valid, f['cp'], 0.0), r['ru'], r['rv']
        du, dv = r['ju'] @ lam_cam, r['jv'] @ lam_cam
        qu, qv = du + r['jdu'] * lam_d, dv + r['jdv'] * lam_d
        k2 = 2.0 * cp * (qu * ru + qv * rv)
        eu, ev = c * qu + k2 * ru, c * qv + k2 * rv
        jua = np.stack([a, zero, bq, bq * Qy, bq * Qx + a * Qz, a * Qy], -1)
        jva = np.stack([zero, cq, dq, cq * Qz + dq * Qy, dq * Qx, cq * Qx], -1)
        dR = np.abs(f['dQ'])
        kk = 1.0 / np.where(valid, r['rho'], 1.0) ** 2
        jdua, jdva = (a * dR[..., 0] + bq * dR[..., 2]) * kk, (cq * dR[..., 1] + dq * dR[..., 2]) * kk
        dua, dva = jua @ la, jva @ la
        lda = np.where(prior, (np.abs(v_d) + k['npd_abs'] @ la) * k['ndd_amp'] / np.abs(np.where(prior, k['ndd'], 1.0)), 0.0)
        rua = np.abs(f['fx'] * (f['Qx'] / f['Qz'])) + abs(f['cx']) + np.abs(f['fl'][0]) + f['u']
        rva = np.abs(f['fy'] * (f['Qy'] / f['Qz'])) + abs(f['cy']) + np.abs(f['fl'][1]) + f['v']
        qua, qva = dua + jdua * lda, dva + jdva * lda
        k2a = 2.0 * np.abs(cp) * (qua * rua + qva * rva)
        eua, eva = c * qua + k2a * rua, c * qva + k2a * rva
    img = lambda x: np.where(valid, x, 0.0)
    return dict(grad_depth=grad_depth, grad_flow=np.stack([img(-eu), img(-ev)]), abs_depth=np.where(prior, wmap * lda / (z * z), 0.0),
                abs_flow=np.stack([img(eua), img(eva)]), lam_d=lam_d, valid=valid, prior=prior, s=np.where(valid, f['s'], np.nan))


def newton_implicit_gradient(depth, flow, mask, motion, rgb2imu, intr, w, rho, grad7, v_d=None, kernel=None, m=None, S=None):
    """The implicit-function gradient with the exact Hessian in depth and flow of a loss with gradient grad7 on [t, q xyzw] of the refined
    pose and v_d on the refined inverse depths, at the state (motion, rho).  Returns newton_vjp_reference_link's dict with the adjoint's
    (s_cam, s_abs, u_cam, u_abs, fallback, lam_p, S, S_own, A, count, blocks) added."""
    adj = newton_adjoint_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, tangent_from_pose_grad(motion, grad7), v_d, kernel, m, S)
    out = newton_vjp_reference_link(depth, flow, mask, motion, rgb2imu, intr, w, rho, adj['lam_p'], v_d, kernel, m, adj['blocks'])
    out.update({x: adj[x] for x in ('s_cam', 's_abs', 'u_cam', 'u_abs', 'fallback', 'lam_p', 'S', 'S_own', 'A', 'count', 'blocks')})
    return out


def newton_implicit_gradient_batch(depth, flow, mask, motion, rgb2imu, intr, w, rho, grad7, v_d=None, status=None, kernel=None, m=None, S=None):
    """newton_implicit_gradient for every link of a batch with the status rule of the entry points: an incoming status passes through,
    a prior weight that is not > 0 gives 3 (BADPRIOR), an S_N that is not finite or has no Cholesky factor gives 2 (NOTPD); such a link
    gets lam_p = 0 and zeros in both gradients, the others carry on.  w a number or (B,), m (B,H,W) or None, S (B,6,6) or None (the
    restatement's own S_N).  Returns (list of dicts, the outgoing status (B))."""
    B = depth.shape[0]
    intr = np.broadcast_to(np.asarray(intr, np.float64).reshape(-1, 4), (B, 4))
    w = np.broadcast_to(np.asarray(w, np.float64).reshape(-1), (B,))
    out, st = [], np.zeros(B, int) if status is None else np.array(status, int)
    zeros = lambda: dict(grad_depth=np.zeros(depth.shape[1:]), grad_flow=np.zeros((2,) + depth.shape[1:]), lam_p=np.zeros(6), fallback=0)
    for b in range(B):
        if st[b] == 0 and not w[b] > 0:
            st[b] = 3
        if st[b] != 0:
            out.append(zeros())
            continue
        args = (depth[b], flow[b], None if mask is None else mask[b], motion[b], rgb2imu, intr[b], float(w[b]), rho[b])
        mb = None if m is None else m[b]
        k = newton_blocks_link(*args, kernel, mb)
        adj = newton_adjoint_reference_link(*args, np.zeros(6), None, kernel, mb, S=np.eye(6), blocks=k)
        SN = adj['S_own'] if S is None else np.asarray(S[b], np.float64)
        try:
            if not np.isfinite(SN).all():
                raise np.linalg.LinAlgError
            np.linalg.cholesky(SN)
        except np.linalg.LinAlgError:
            st[b] = 2
            z = zeros()
            z['fallback'] = adj['fallback']
            out.append(z)
            continue
        out.append(newton_implicit_gradient(*args, grad7[b], None if v_d is None else v_d[b], kernel, mb, SN))
    return out, st


def newton_dense_system(k):
    """The exact (6 + n) x (6 + n) matrix of one link assembled explicitly from newton_blocks_link's dict: unknowns [xi (6, body frame);
    rho_i of every pixel with a prior].  Returns (matrix, the flat indices of those pixels)."""
    idx = np.flatnonzero(k['prior'].ravel())
    n, A = idx.size, k['A']
    Mx = np.zeros((6 + n, 6 + n))
    Mx[:6, :6] = A.T @ k['npp'].reshape(-1, 6, 6).sum(0) @ A
    pd = k['npd'].reshape(-1, 6)[idx] @ A
    Mx[:6, 6:] = pd.T
    Mx[6:, :6] = pd
    Mx[6:, 6:] = np.diag(k['ndd'].ravel()[idx])
    return Mx, idx
