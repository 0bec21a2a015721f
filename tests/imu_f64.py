"""Tests only: NumPy float64 transcription of the IMU derivative kernels -- sample_element / join of islam_amd/csrc/imu_cov.hip,
sample_rot / join of imu_bias_jac.hip, preint_bwd_kernel with JlT of imu_preint.hip, bias_correct_kernel and gyro_bias_solve_kernel --
the same formulas, the same thresholds, the same series, folded one sample after the other (the kernels fold lane chunks and scan
trees: another association order of the same joins).  It is NOT a reference: tests/test_imu_golden_cpu.py measures its error against
the 60-digit reference of tests/golden/make_imu_golden.py, which gives the rounding floor of these formulas in float64 and from it the
tolerances of tests/test_imu_golden_gpu.py, and it runs the mutants below to show that the tolerances are tight enough to see them.
(The forward's transcription is oracle.cwrap.imu_integrate, bit-exact by contract.)

`mutant(name)` switches one deliberate mistake on for the duration of a with-block."""
import contextlib

import numpy as np

# one name per deliberate mistake (see test_imu_golden_cpu.py for what each one is)
MUTANTS = ('A_t2', 'B_t2', 'C_t2', 'jr_jl', 'jlt_c1_t2', 'jlt_c2_t2', 'jlt_swap_c1_c2', 'jlt_c1_one_minus_cos', 'bc_im_t2', 'bc_re_t2',
           'log_atan', 'log_no_flip', 'init_jac_block')
_on = set()
I3 = np.eye(3)


@contextlib.contextmanager
def mutant(name):
    assert name in MUTANTS, name
    _on.add(name)
    try:
        yield
    finally:
        _on.discard(name)


def _t2(name):
    """Factor of the second term of a series: 1, or 0 under the mutant that drops it."""
    return 0.0 if name in _on else 1.0


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def conj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def rot3(q, p):
    u, w = q[:3], q[3]
    c = 2.0 * np.cross(u, p)
    return p + w * c + np.cross(u, c)


# ------------------------------------------------------------------ imu_cov.hip / imu_bias_jac.hip
def sample_rot(d, w):
    """R = Exp(w d)^T and Jr(w d) of one sample (sample_element of imu_cov.hip, sample_rot of imu_bias_jac.hip)."""
    th = w * d
    th2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2]
    t = np.sqrt(th2)
    if t > 1e-3:
        s, sh = np.sin(t), np.sin(0.5 * t)
        A, B, C = s / t, 2.0 * sh * sh / th2, (t - s) / (th2 * t)
    else:
        A = 1.0 - _t2('A_t2') * th2 * (1.0 / 6.0) + th2 * th2 * (1.0 / 120.0)
        B = 0.5 - _t2('B_t2') * th2 * (1.0 / 24.0) + th2 * th2 * (1.0 / 720.0)
        C = 1.0 / 6.0 - _t2('C_t2') * th2 * (1.0 / 120.0) + th2 * th2 * (1.0 / 5040.0)
    K = hat(th)
    K2 = K @ K
    sB = -B if 'jr_jl' in _on else B
    return I3 - A * K + B * K2, I3 - sB * K + C * K2


def _phi(d, R, a):
    P = np.eye(9)
    ax = hat(a)
    P[0:3, 0:3], P[3:6, 0:3], P[6:9, 0:3] = R, -d * ax, -(0.5 * d * d) * ax
    P[6:9, 3:6] = d * I3
    return P


def _sym(Q):
    """What stsym / the packed storage keep: the mean of a diagonal block and its transpose, the lower off-diagonal blocks mirrored."""
    S = np.tril(Q, -1)
    S = S + S.T + np.diag(np.diag(Q))
    for b in range(3):
        k = slice(3 * b, 3 * b + 3)
        S[k, k] = 0.5 * (Q[k, k] + Q[k, k].T)
    return S


def _join_maps(lo_phi, hi_phi):
    """Phi' and T of join(): the later element's v and p rows turned by W = R_lo^T."""
    W = lo_phi[0:3, 0:3].T
    T = np.eye(9)
    T[3:6, 3:6] = T[6:9, 6:9] = W
    P2 = hi_phi.copy()
    P2[3:6, 0:3], P2[6:9, 0:3] = W @ hi_phi[3:6, 0:3], W @ hi_phi[6:9, 0:3]
    return P2, T


def _fold(dt, gyro, acc, seg, motion, first, sample, join):
    """Rows of the per-frame fold (motion) or of the running prefix behind `first` (world); element = (Phi, X)."""
    n = len(seg) - 1
    rows = [] if motion else [first[1]]
    prefix = first
    for i in range(n):
        E = None
        for j in range(int(seg[i]), int(seg[i + 1])):
            X = sample(dt[j], gyro[j], acc[j], j)
            E = X if E is None else join(E, X)
        if motion:
            rows.append(np.zeros_like(first[1]) if E is None else E[1])
        else:
            if E is not None:
                prefix = join(prefix, E)
            rows.append(prefix[1])
    return np.stack(rows) if rows else np.zeros((0,) + first[1].shape)


def cov(dt, gyro, acc, seg, gyro_cov, acc_cov, motion, init_cov=None):
    """islam_imu_preint_cov: (rows, 9, 9)."""
    dt, gyro, acc = (np.asarray(a, np.float64) for a in (dt, gyro, acc))
    sg, sa = np.broadcast_to(np.asarray(gyro_cov, np.float64), (3,)), np.broadcast_to(np.asarray(acc_cov, np.float64), (3,))

    def sample(d, w, a, j):
        R, J = sample_rot(d, w)
        Q = np.zeros((9, 9))
        Q[0:3, 0:3] = (J * (sg * d * d)) @ J.T
        hd2 = 0.5 * d * d
        Q[3:6, 3:6], Q[6:9, 3:6], Q[3:6, 6:9], Q[6:9, 6:9] = np.diag(d * d * sa), np.diag(hd2 * d * sa), np.diag(hd2 * d * sa), np.diag(hd2 * hd2 * sa)
        return _phi(d, R, a), _sym(Q)

    def join(lo, hi):
        P2, T = _join_maps(lo[0], hi[0])
        return P2 @ lo[0], _sym(P2 @ lo[1] @ P2.T + T @ hi[1] @ T.T)

    Q0 = np.zeros((9, 9)) if init_cov is None or motion else 0.5 * (np.asarray(init_cov, np.float64) + np.asarray(init_cov, np.float64).T)
    return _fold(dt, gyro, acc, seg, motion, (np.eye(9), Q0), sample, join)


def bias_jac(dt, gyro, acc, seg, motion, init_jac=None):
    """islam_imu_preint_bias_jac: (rows, 9, 6)."""
    dt, gyro, acc = (np.asarray(a, np.float64) for a in (dt, gyro, acc))

    def sample(d, w, a, j):
        R, J = sample_rot(d, w)
        G = np.zeros((9, 6))
        G[0:3, 0:3], G[3:6, 3:6], G[6:9, 3:6] = -d * J, -d * I3, -(0.5 * d * d) * I3
        return _phi(d, R, a), G

    def join(lo, hi):
        P2, T = _join_maps(lo[0], hi[0])
        G = P2 @ lo[1] + T @ hi[1]
        if 'init_jac_block' not in _on:
            G[0:3, 3:6] = 0.0            # the (dphi, b_a) block is not stored
        return P2 @ lo[0], G

    G0 = np.zeros((9, 6))
    if init_jac is not None and not motion:
        G0 = np.array(init_jac, dtype=np.float64)
        if 'init_jac_block' not in _on:
            G0[0:3, 3:6] = 0.0
    return _fold(dt, gyro, acc, seg, motion, (np.eye(9), G0), sample, join)


# ------------------------------------------------------------------ imu_preint.hip: forward intermediates and preint_bwd_kernel
def _so3exp_fwd(p):
    th2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
    th = np.sqrt(th2)
    if th > 2.220446049250313e-16:
        imag, real = np.sin(0.5 * th) / th, np.cos(0.5 * th)
    else:
        imag, real = 0.5 - (1.0 / 48.0) * th2 + (1.0 / 3840.0) * th2 * th2, 1.0 - (1.0 / 8.0) * th2 + (1.0 / 384.0) * th2 * th2
    return np.array([p[0] * imag, p[1] * imag, p[2] * imag, real])


def JlT(w, u):
    """Jl(w)^T u"""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    th = np.sqrt(th2)
    if th > 1e-4:
        sh = np.sin(0.5 * th)
        c1 = (1.0 - np.cos(th)) / th2 if 'jlt_c1_one_minus_cos' in _on else 2.0 * sh * sh / th2
        c2 = (th - np.sin(th)) / (th2 * th)
    else:
        c1, c2 = 0.5 - _t2('jlt_c1_t2') * th2 / 24.0, 1.0 / 6.0 - _t2('jlt_c2_t2') * th2 / 120.0
    if 'jlt_swap_c1_c2' in _on:
        c1, c2 = c2, c1
    wu = np.cross(w, u)
    return u + (-c1) * wu + c2 * np.cross(w, wu)


def preint_bwd(dt, gyro, acc, seg, init_rot, gravity, motion, g_pos, g_rot, g_vel):
    """islam_imu_preint_bwd in float64: (g_gyro, g_acc).  incre_r, the frame-start rotations and the frame sums are those of the
    forward, taken sequentially.  g_rot: (rows, 4), left tangent in slots 0..2."""
    dt, gyro, acc = (np.asarray(a, np.float64) for a in (dt, gyro, acc))
    n, S = len(seg) - 1, len(dt)
    g = np.array([0.0, 0.0, gravity])
    ir, R0, loc = [], [np.asarray(init_rot, np.float64)], np.zeros((n, 7))
    for i in range(n):
        a0, F = int(seg[i]), int(seg[i + 1] - seg[i])
        A = [np.array([0.0, 0.0, 0.0, 1.0])]
        for j in range(F):
            A.append(qmul(A[-1], _so3exp_fwd(gyro[a0 + j] * dt[a0 + j])))
        ir.append(A)
        r0 = R0[-1]
        iv, ip, it = np.zeros(3), np.zeros(3), 0.0
        for j in range(F):
            d = dt[a0 + j]
            ra = rot3(A[j], acc[a0 + j] - rot3(conj(qmul(r0, A[j + 1])), g))
            ip = ip + (iv * d + ra * 0.5 * (d * d))
            iv = iv + ra * d
            it = it + d
        loc[i, 0:3], loc[i, 3:6], loc[i, 6] = rot3(r0, iv), rot3(r0, ip), it
        R0.append(qmul(r0, A[F]) if F > 0 else r0)
    gv, gp, gR = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    if motion:
        gv[:], gp[:] = g_vel, g_pos
    else:
        pb, vb = g_pos[n].copy(), g_vel[n].copy()
        for i in range(n - 1, -1, -1):
            gv[i], gp[i] = vb, pb
            if seg[i + 1] == seg[i]:
                vb, pb = g_vel[i].copy(), g_pos[i] + pb
            else:
                vb, pb = g_vel[i] + vb + loc[i, 6] * pb, g_pos[i] + pb
    g_gyro, g_acc = np.zeros((S, 3)), np.zeros((S, 3))
    for i in range(n):
        a0, F = int(seg[i]), int(seg[i + 1] - seg[i])
        if F == 0:
            continue
        Ri, A = R0[i], ir[i]
        RiT = conj(Ri)
        Vb, Pb = rot3(RiT, gv[i]), rot3(RiT, gp[i])
        gRl = np.cross(loc[i, 0:3], gv[i]) + np.cross(loc[i, 3:6], gp[i])
        Sa = g_rot[i, :3].copy() if motion else np.zeros(3)
        carry, Tk = np.zeros(3), 0.0
        for k in range(F - 1, -1, -1):
            d = dt[a0 + k]
            Qk1 = qmul(Ri, A[k + 1])
            av = acc[a0 + k] - rot3(conj(Qk1), g)
            ra = rot3(A[k], av)
            rab = d * Vb + (d * (0.5 * d + Tk)) * Pb
            ab = rot3(conj(A[k]), rab)
            g_acc[a0 + k] = ab
            Qb = np.cross(rot3(Qk1, -1.0 * ab), g)
            gRl = gRl + Qb
            Sa = Sa + rot3(RiT, Qb) + carry
            wb = JlT(gyro[a0 + k] * d, rot3(conj(A[k]), Sa))
            g_gyro[a0 + k] = wb * d
            carry = np.cross(ra, rab)
            Tk += d
        gR[i] = gRl
    Tn = np.zeros(3) if motion else g_rot[n, :3].copy()
    for i in range(n - 1, -1, -1):
        local = gR[i].copy()
        gR[i] = Tn
        Tn = local + Tn + (np.zeros(3) if motion else g_rot[i, :3])
    for i in range(n):
        a0, F = int(seg[i]), int(seg[i + 1] - seg[i])
        if F == 0 or not gR[i].any():
            continue
        extra = rot3(conj(R0[i]), gR[i])
        for k in range(F):
            d = dt[a0 + k]
            g_gyro[a0 + k] += JlT(gyro[a0 + k] * d, rot3(conj(ir[i][k]), extra)) * d
    return g_gyro, g_acc


# ------------------------------------------------------------------ bias_correct_kernel, gyro_bias_solve_kernel
def bias_correct(jac, rot, vel, pos, dbg, dba, dtype=np.float64):
    """islam_imu_bias_correct: (rot, vel, pos) in `dtype` from inputs rounded to it."""
    rot, vel, pos = (np.asarray(a, dtype).astype(np.float64) for a in (rot, vel, pos))
    b = np.concatenate([dbg, dba])
    th = jac[:, 0:3, 0:3] @ dbg
    dv, dp = jac[:, 3:6, :] @ b, jac[:, 6:9, :] @ b
    t2 = (th * th).sum(1)
    t = np.sqrt(t2)
    big = t > 1e-4
    ts = np.where(big, t, 1.0)
    im = np.where(big, np.sin(0.5 * ts) / ts, 0.5 - _t2('bc_im_t2') * t2 * (1.0 / 48.0))
    re = np.where(big, np.cos(0.5 * ts), 1.0 - _t2('bc_re_t2') * t2 * (1.0 / 8.0))
    q = qmul(rot, np.concatenate([th * im[:, None], re[:, None]], 1))
    q = q * (1.0 / np.sqrt((q * q).sum(1)))[:, None]
    return q.astype(dtype), (vel + dv).astype(dtype), (pos + dp).astype(dtype)


def gyro_bias_solve(jac, rot_imu, rot_ref, weight):
    """islam_imu_gyro_bias_solve: (x, H)."""
    q = qmul(conj(np.asarray(rot_imu, np.float64)), np.asarray(rot_ref, np.float64))
    if 'log_atan' not in _on and 'log_no_flip' not in _on:
        q = np.where(q[:, 3:] < 0.0, -q, q)
    vn = np.sqrt((q[:, :3] ** 2).sum(1))
    big = vn > 1e-8 * q[:, 3]
    vs = np.where(big, vn, 1.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        ang = np.arctan(vs / q[:, 3]) if 'log_atan' in _on else np.arctan2(vs, q[:, 3])
        k = np.where(big, 2.0 * ang / vs, 2.0 / q[:, 3])
        r = k[:, None] * q[:, :3]
    J = jac[:, 0:3, 0:3]
    keep = (weight != 0.0) & np.isfinite(r).all(1) & np.isfinite(weight)          # (a row without a finite residual is left out)
    H = np.einsum('i,iab,iac->bc', weight[keep], J[keep], J[keep])
    gvec = np.einsum('i,iab,ia->b', weight[keep], J[keep], r[keep])
    l00 = np.sqrt(H[0, 0])
    l10, l20 = H[0, 1] / l00, H[0, 2] / l00
    l11 = np.sqrt(H[1, 1] - l10 * l10)
    l21 = (H[1, 2] - l20 * l10) / l11
    l22 = np.sqrt(H[2, 2] - l20 * l20 - l21 * l21)
    y0 = gvec[0] / l00
    y1 = (gvec[1] - l10 * y0) / l11
    y2 = (gvec[2] - l20 * y0 - l21 * y1) / l22
    x2 = y2 / l22
    x1 = (y1 - l21 * x2) / l11
    x0 = (y0 - l10 * x1 - l20 * x2) / l00
    return np.array([x0, x1, x2]), H
