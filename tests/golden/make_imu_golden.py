"""Writes tests/golden/imu_cases.npz: IMU streams whose per-sample rotation angles |gyro| dt run from 0 across every series /
closed-form switch of the IMU derivative kernels up to 6 rad, and reference outputs computed with mpmath at 60 digits and rounded to
float64 -- for islam_imu_preint_cov, islam_imu_preint_bias_jac, islam_imu_preint (forward and backward), islam_imu_bias_correct and
islam_imu_gyro_bias_solve.

    python -m tests.golden.make_imu_golden          (from the repository root; needs mpmath; under a minute on eight cores)

The reference uses no closed-form coefficient (the mp arithmetic is tests/golden/make_lie_golden.py's):
  * Exp: the power series of the quaternion exponential; Jr = sum_n (-K)^n / (n+1)!, summed until the terms vanish;
  * Log: 2 atan2(|v|, w) v/|v| on the quaternion with w >= 0;
  * covariance and bias Jacobians: Sigma <- A Sigma A^T + Q and J <- A J - B one sample after the other, A, B, Q as
    include/islam_hip.h defines them (the (dphi, b_a) block of init_jac dropped, the symmetric part of init_cov taken);
  * forward: the frame loop of oracle/imu_preint_body.inc (tests/helpers.py::imu_preint_torch states it in torch): the acceleration
    turned by the rotation in front of the sample, gravity taken out in the frame behind it, p += v d + a d^2 / 2, v += a d,
    R <- R Exp(w d); init_rot is (1/2, -1/2, 1/2, 1/2), EXACTLY of unit norm, so that q (.) q^-1 is a rotation matrix to 60 digits;
  * backward: central differences with step 1e-20 of that integrator, of
        L = sum_rows wp . pos + wv . vel + wr . Log(rot_perturbed rot_nominal^-1)
    (a rotation row contributes its LEFT tangent: PyPose's convention, which islam_imu_preint_bwd reads from slots 0..2 of g_rot).
    In motion mode too a gyro sample moves every LATER frame (pos and vel are turned by the frame's start rotation, and gravity
    is taken out in it), so both modes re-integrate the sample's frame and walk the frames behind it.  That walk is exact and cheap
    because a frame's sums are affine in the gravity vector seen from its start: iv = iv_acc - Mv R0^T g, ip = ip_acc - Mp R0^T g;
  * bias correction and gyro-bias solve: the definitions of include/islam_hip.h (the 3x3 normal equations by Cramer's rule).
Inputs enter the mp arithmetic exactly from their float64 values -- or, for the float32 cases, from their float32 values -- so a
comparison measures the rounding inside the code under test only.  See tests/test_imu_golden_cpu.py for how the floors and
tolerances stored beside the references are measured."""
import multiprocessing
import os

import numpy as np

from tests.golden import make_lie_golden as L

PI = 3.141592653589793
# 0 | tiny | below every switch | both sides of 1e-4 (JlT, bias_correct's Exp) | where (1 - cos th) / th^2 cancels worst | both sides of
# 1e-3 (sample_element, sample_rot) | mid | both sides of pi/2 (the half angle crosses the forward's pi/4 argument reduction) | large |
# next to pi | beyond pi
ANGLES = (0.0, 1e-12, 1e-8, 3e-5, 1e-4 * (1 - 1e-3), 1e-4 * (1 + 1e-3), 1.5e-4, 2e-4, 1e-3 * (1 - 1e-3), 1e-3 * (1 + 1e-3), 1e-2, 0.1, 0.6,
          1.0, PI / 2 * (1 - 1e-3), PI / 2 * (1 + 1e-3), 2.0, 3.0, PI - 1e-6, 4.0, 6.0)
COUNTS = (0, 1, 2, 3, 7, 10, 64, 65, 130)
BC_ANGLES = (0.0, 1e-12, 1e-8, 1e-4 * (1 - 1e-3), 1e-4 * (1 + 1e-3), 1e-2, 1.0, 3.0)
SOLVE_ANGLES = (0.0, 1e-12, 2e-8 * (1 - 1e-2), 2e-8 * (1 + 1e-2), 1e-3, 1.0, 3.0, PI - 1e-6)
BC_SMALL = 6                     # the first BC_SMALL angles stay at or below 1e-2
A_FRAMES, B_FRAMES, B_LONG, BC_ROWS, SOLVE_ROWS = 110, 260, 70, 32, 300
GYRO_COV, ACC_COV = (1.6968e-4) ** 2, (2.0e-3) ** 2          # tests/test_imu_cov_gpu.py
GRAVITY = 9.81
INIT_ROT = (0.5, -0.5, 0.5, 0.5)
INIT_POS, INIT_VEL = (1.0, 2.0, 3.0), (0.5, -1.0, 0.2)
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'imu_cases.npz')
IU = np.triu_indices(9)
DTYPES = {'f64': np.float64, 'f32': np.float32}
_f, _out, _qmul, _qinv = L._f, L._out, L._qmul, L._qinv


# ------------------------------------------------------------------ mp arithmetic on plain lists
def _hat(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def _qmat(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def _T(A):
    return [list(r) for r in zip(*A)]


def _mv(A, v):
    return [sum(a * b for a, b in zip(r, v)) for r in A]


def _mm(A, B):
    out = [[0] * len(B[0]) for _ in A]
    for i, row in enumerate(A):
        o = out[i]
        for l, a in enumerate(row):
            if a == 0:
                continue
            for j, b in enumerate(B[l]):
                if b != 0:
                    o[j] = o[j] + a * b
    return out


def _add(A, B, s=1):
    return [[a + s * b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def _zeros(r, c):
    return [[0] * c for _ in range(r)]


def _eye(n):
    return [[int(i == j) for j in range(n)] for i in range(n)]


def _mat(a):
    a = np.asarray(a, dtype=np.float64)
    return [_f(r) for r in a]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def sample_parts(d, w):
    """(Exp(w d) as a quaternion, as a matrix, Jr(w d)) of one sample."""
    phi = [w[0] * d, w[1] * d, w[2] * d]
    q = L._so3_exp(phi)
    return q, _qmat(q), L._V([-p for p in phi])


def _step(Sig, J, DR, d, dr, Jr, a, sg, sa):
    A = _zeros(9, 9)
    Ra = _mm(DR, _hat(a))
    hd2 = d * d / 2
    for i in range(3):
        for j in range(3):
            A[i][j] = dr[j][i]
            A[3 + i][j] = -Ra[i][j] * d
            A[6 + i][j] = -Ra[i][j] * hd2
        A[3 + i][3 + i], A[6 + i][3 + i], A[6 + i][6 + i] = 1, d, 1
    B = _zeros(9, 6)
    for i in range(3):
        for j in range(3):
            B[i][j] = Jr[i][j] * d
            B[3 + i][3 + j] = DR[i][j] * d
            B[6 + i][3 + j] = DR[i][j] * hd2
    var = list(sg) + list(sa)
    Bs = [[b * v for b, v in zip(row, var)] for row in B]
    return _add(_mm(_mm(A, Sig), _T(A)), _mm(Bs, _T(B))), _add(_mm(A, J), B, -1), _mm(DR, dr)


def ref_cov_jac(parts, dt, acc, seg, frames, motion, init_cov=None, init_jac=None):
    """Rows of Sigma and J for frames [0, frames) of the stream: motion -> one row per frame, world -> row 0 = the start and one row
    behind every frame.  parts[j] = sample_parts of sample j, dt / acc lists of mpf."""
    mp = L._mp()
    sg, sa = [mp.mpf(GYRO_COV)] * 3, [mp.mpf(ACC_COV)] * 3
    Sig, J, DR = _zeros(9, 9), _zeros(9, 6), _eye(3)
    if not motion:
        C = _mat(init_cov)
        Sig = [[(C[i][j] + C[j][i]) / 2 for j in range(9)] for i in range(9)]
        J = _mat(init_jac)
        for i in range(3):
            for j in range(3, 6):
                J[i][j] = 0
    cov, jac = ([], []) if motion else ([Sig], [J])
    for i in range(frames):
        if motion:
            Sig, J, DR = _zeros(9, 9), _zeros(9, 6), _eye(3)
        for j in range(int(seg[i]), int(seg[i + 1])):
            Sig, J, DR = _step(Sig, J, DR, dt[j], parts[j][1], parts[j][2], acc[j], sg, sa)
        cov.append(Sig)
        jac.append(J)
    return (np.stack([np.array([_out(r) for r in S])[IU] for S in cov]), np.stack([np.array([_out(r) for r in S]) for S in jac]))


def frame_local(qs, ds, accs):
    """The sums of one frame from the rotation at its start, as affine maps of u = R0^T g:
    (A_F, iv_acc, ip_acc, Mv, Mp, t, F) with iv = iv_acc - Mv u, ip = ip_acc - Mp u."""
    mp = L._mp()
    A, RA = [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)], _eye(3)
    iv, ip, Mv, Mp, it = [0, 0, 0], [0, 0, 0], _zeros(3, 3), _zeros(3, 3), 0
    for q, d, a in zip(qs, ds, accs):
        A1 = _qmul(A, q)
        RA1 = _qmat(A1)
        N, ra, hd2 = _mm(RA, _T(RA1)), _mv(RA, a), d * d / 2
        ip = [ip[c] + iv[c] * d + ra[c] * hd2 for c in range(3)]
        iv = [iv[c] + ra[c] * d for c in range(3)]
        Mp = [[Mp[r][c] + Mv[r][c] * d + N[r][c] * hd2 for c in range(3)] for r in range(3)]
        Mv = [[Mv[r][c] + N[r][c] * d for c in range(3)] for r in range(3)]
        it = it + d
        A, RA = A1, RA1
    return A, iv, ip, Mv, Mp, it, len(qs)


def frame_out(lc, lp, lr, lv, g, motion):
    """(pos, rot, vel) row of one frame and the state behind it."""
    mp = L._mp()
    A, iva, ipa, Mv, Mp, it, F = lc
    z3 = [mp.mpf(0)] * 3
    if F == 0:                           # no samples: velocity zeroed, position and rotation held
        if motion:
            return (z3, [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)], z3), (lp, lr, lv)
        return (lp, lr, z3), (lp, lr, z3)
    R = _qmat(lr)
    u = [R[2][0] * g, R[2][1] * g, R[2][2] * g]
    mvu, mpu = _mv(Mv, u), _mv(Mp, u)
    rv, rp = _mv(R, [iva[c] - mvu[c] for c in range(3)]), _mv(R, [ipa[c] - mpu[c] for c in range(3)])
    sr = _qmul(lr, A)
    if motion:
        return (rp, A, rv), (lp, sr, lv)
    sp, sv = [lp[c] + rp[c] + lv[c] * it for c in range(3)], [lv[c] + rv[c] for c in range(3)]
    return (sp, sr, sv), (sp, sr, sv)


class Stream:
    """A stream in mp: samples, per-sample Exp, per-frame sums, and the nominal forward rows / frame-start states of both modes."""

    def __init__(self, dt, gyro, acc, seg, gravity, frames=None, dtype=np.float64):
        self.seg = [int(s) for s in seg]
        self.n = len(self.seg) - 1 if frames is None else frames
        self.dt, self.gyro, self.acc = _f(dt), _mat(gyro), _mat(acc)
        self.g = _f([gravity])[0]
        self.q = {}
        self.loc = [self.local(i) for i in range(self.n)]
        self.rows, self.state = {}, {}
        for motion in (True, False):
            mp = L._mp()
            p0, q0, v0 = (_f(np.asarray(a, dtype=dtype)) for a in (INIT_POS, INIT_ROT, INIT_VEL))       # (enter as the forward reads them)
            st = ([mp.mpf(0)] * 3 if motion else p0, q0, [mp.mpf(0)] * 3 if motion else v0)
            rows, states = ([] if motion else [st]), []
            for i in range(self.n):
                states.append(st)
                row, st = frame_out(self.loc[i], *st, self.g, motion)
                rows.append(row)
            self.rows[motion], self.state[motion] = rows, states

    def expq(self, j):
        if j not in self.q:
            self.q[j] = L._so3_exp([w * self.dt[j] for w in self.gyro[j]])
        return self.q[j]

    def local(self, i, s=None, gyro=None, acc=None):
        """frame_local of frame i, sample s replaced"""
        a, b = self.seg[i], self.seg[i + 1]
        qs = [self.expq(j) if j != s or gyro is None else L._so3_exp([w * self.dt[j] for w in gyro]) for j in range(a, b)]
        return frame_local(qs, self.dt[a:b], [self.acc[j] if j != s or acc is None else acc for j in range(a, b)])

    def forward(self, motion):
        r = self.rows[motion]
        return tuple(np.stack([_out(row[k]) for row in r]) for k in range(3))

    def loss_from(self, motion, i, lc, cot, rot_moved):
        """The part of L that frame i's sums reach, with frame i's sums replaced by lc."""
        wp, wr, wv = cot
        st, tot = self.state[motion][i], 0
        for k in range(i, self.n):
            (pos, rot, vel), st = frame_out(lc if k == i else self.loc[k], *st, self.g, motion)
            row = k if motion else k + 1
            tot = tot + _dot(wp[row], pos) + _dot(wv[row], vel)
            if rot_moved and (k == i or not motion):
                tot = tot + _dot(wr[row], L._so3_log(_qmul(rot, _qinv(self.rows[motion][row][1]))))
            if motion and not rot_moved:
                break
        return tot

    def grad(self, motion, s, cot):
        """d L / d gyro_s (3), d L / d acc_s (3) by central differences"""
        mp = L._mp()
        h = mp.mpf(10) ** -20
        i = max(k for k in range(self.n) if self.seg[k] <= s)         # (the last of several frames that start at s is the one that holds it)
        out = []
        for kind in ('gyro', 'acc'):
            base = self.gyro[s] if kind == 'gyro' else self.acc[s]
            for c in range(3):
                v = []
                for sgn in (1, -1):
                    x = list(base)
                    x[c] = x[c] + sgn * h
                    lc = self.local(i, s, **{kind: x})
                    v.append(self.loss_from(motion, i, lc, cot, kind == 'gyro'))
                out.append((v[0] - v[1]) / (2 * h))
        return out


def ref_bias_correct(J, rot, vel, pos, dbg, dba):
    """One row: DR Exp(J_phig dbg) renormalised, dv + J_vg dbg + J_va dba, dp + J_pg dbg + J_pa dba (all lists of mpf; J 9x6)."""
    mp = L._mp()
    b = list(dbg) + list(dba)
    q = _qmul(rot, L._so3_exp([_dot(J[r][:3], dbg) for r in range(3)]))
    n = mp.sqrt(_dot(q, q))
    return [v / n for v in q], [vel[r] + _dot(J[3 + r], b) for r in range(3)], [pos[r] + _dot(J[6 + r], b) for r in range(3)]


def ref_solve(jac, rot_imu, rot_ref, weight):
    """(x, H, residual angle of every row) of the weighted normal equations"""
    mp = L._mp()
    H, g, ang = _zeros(3, 3), [0, 0, 0], []
    for i in range(len(jac)):
        r = L._so3_log(_qmul(_qinv(_f(rot_imu[i])), _f(rot_ref[i])))
        ang.append(mp.sqrt(_dot(r, r)))
        w = _f([weight[i]])[0]
        Jp = _mat(jac[i][0:3, 0:3])
        for a in range(3):
            g[a] = g[a] + w * sum(Jp[k][a] * r[k] for k in range(3))
            for b in range(3):
                H[a][b] = H[a][b] + w * sum(Jp[k][a] * Jp[k][b] for k in range(3))
    return _out(L._solve3(H, g)), np.array([_out(r) for r in H]), _out(ang)


# ------------------------------------------------------------------ inputs
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _stream(rng, counts, angle_index):
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    S = int(seg[-1])
    dt = rng.uniform(0.004, 0.012, S)
    gyro = _unit(rng, S) * (np.array([ANGLES[k] for k in angle_index(S)]) / dt)[:, None]
    acc = rng.normal(0, 1.0, (S, 3)) + np.array([0, 0, 9.81])
    return seg, dt, gyro, acc


def make_inputs():
    rng = np.random.default_rng(20250314)
    na = len(ANGLES)
    # stream A: one sample per angle, then ragged frames; empty frames at the border of the 64-frame scan block and at the end
    counts = np.concatenate([np.ones(na, dtype=np.int64), rng.choice(COUNTS[:6], A_FRAMES - na)])
    for i, c in ((30, 64), (70, 65), (90, 130), (63, 0), (64, 0), (A_FRAMES - 1, 0), (40, 7), (41, 10), (42, 3), (43, 2)):
        counts[i] = c
    a_seg, a_dt, a_gyro, a_acc = _stream(rng, counts, lambda S: [s if s < na else (s - na) % na for s in range(S)])
    assert len(a_dt) <= 700, len(a_dt)
    M = rng.normal(size=(9, 9))
    scale = np.array([1e-3] * 3 + [1e-2] * 3 + [1e-3] * 3)
    init_cov = (M @ M.T / 9.0) * scale[:, None] * scale[None, :]
    init_jac = rng.normal(0, 1.0, (9, 6)) * np.array([0.1] * 6 + [0.01] * 3)[:, None]
    # stream B: more frames than the backward kernel has lanes, 0..2 samples each, and one long frame
    counts = rng.integers(0, 3, B_FRAMES)
    counts[100] = B_LONG
    counts[0], counts[255], counts[256], counts[B_FRAMES - 1] = 2, 1, 2, 1
    b_seg, b_dt, b_gyro, b_acc = _stream(rng, counts, lambda S: [(s + 3) % na for s in range(S)])
    z = dict(a_seg=a_seg, a_dt=a_dt, a_gyro=a_gyro, a_acc=a_acc, init_cov=init_cov, init_jac=init_jac, b_seg=b_seg, b_dt=b_dt, b_gyro=b_gyro,
             b_acc=b_acc)
    for mode, rows in (('motion', B_FRAMES), ('world', B_FRAMES + 1)):
        for k in ('wp', 'wr', 'wv'):
            z['b_%s_%s' % (k, mode)] = rng.normal(size=(rows, 3))
    # gyro-bias solve: rotations and weights (the Jacobians are stream A's, filled in by make_references)
    z['s_rot_imu'] = rng.normal(size=(SOLVE_ROWS, 4))
    z['s_rot_imu'] /= np.linalg.norm(z['s_rot_imu'], axis=1, keepdims=True)
    z['s_axis'] = _unit(rng, SOLVE_ROWS)
    z['s_angle'] = np.array([SOLVE_ANGLES[i % len(SOLVE_ANGLES)] for i in range(SOLVE_ROWS)])
    z['s_negated'] = np.arange(SOLVE_ROWS) % 3 == 2          # (3 and len(SOLVE_ANGLES) = 8 are coprime: every angle is negated somewhere)
    w = rng.uniform(0.2, 3.0, SOLVE_ROWS)
    w[rng.random(SOLVE_ROWS) < 0.1] = 0.0
    z['s_weight'] = w
    # stream C: one frame of one sample per angle; run in motion mode without gravity and with a rotation cotangent alone, its gyro
    # gradient is d Jl(w d)^T wr and nothing else
    c_seg, c_dt, c_gyro, c_acc = _stream(rng, np.ones(na, dtype=np.int64), lambda S: list(range(S)))
    z.update(c_seg=c_seg, c_dt=c_dt, c_gyro=c_gyro, c_acc=c_acc, c_wr=rng.normal(size=(na, 3)))
    z['bc_dir'], z['bc_dba'] = _unit(rng, len(BC_ANGLES)), rng.normal(0, 0.1, (len(BC_ANGLES), 3))
    return z


def rounded(z, key, name):
    return np.asarray(z[key], dtype=DTYPES[name]).astype(np.float64)


def stream_a(z, name, frames=None):
    dt, gyro, acc = (rounded(z, k, name) for k in ('a_dt', 'a_gyro', 'a_acc'))
    return Stream(dt, gyro, acc, z['a_seg'], float(DTYPES[name](GRAVITY)), frames, DTYPES[name])


def _grad_task(args):
    motion, s = args
    return _out(_GRAD_STREAM.grad(motion, s, _GRAD_COT[motion]))


_GRAD_STREAM, _GRAD_COT = None, None


def cotangents(z):
    return {motion: tuple([_f(r) for r in z['b_%s_%s' % (k, 'motion' if motion else 'world')]] for k in ('wp', 'wr', 'wv')) for motion in (True, False)}


def make_references(z):
    global _GRAD_STREAM, _GRAD_COT
    for name in DTYPES:
        st = stream_a(z, name)
        parts = [sample_parts(st.dt[j], st.gyro[j]) for j in range(len(st.dt))]
        for motion, mode in ((True, 'motion'), (False, 'world')):
            z['cov_%s_%s_ref' % (mode, name)], z['jac_%s_%s_ref' % (mode, name)] = ref_cov_jac(parts, st.dt, st.acc, st.seg, st.n, motion,
                                                                                            z['init_cov'], z['init_jac'])
            for k, a in zip(('pos', 'rot', 'vel'), st.forward(motion)):
                z['fwd_%s_%s_%s_ref' % (k, mode, name)] = a
    # bias correction: the first BC_ROWS motion rows of stream A; per angle of BC_ANGLES one dbg, scaled so that row k hits it
    J = z['jac_motion_f64_ref'][:BC_ROWS]
    z['bc_dbg'] = np.stack([z['bc_dir'][k] * (a / np.linalg.norm(J[k, 0:3, 0:3] @ z['bc_dir'][k])) for k, a in enumerate(BC_ANGLES)])
    for name in DTYPES:
        inc = [np.asarray(z['fwd_%s_motion_f64_ref' % k][:BC_ROWS], dtype=DTYPES[name]).astype(np.float64) for k in ('rot', 'vel', 'pos')]
        out = [[ref_bias_correct(_mat(J[r]), _f(inc[0][r]), _f(inc[1][r]), _f(inc[2][r]), _f(z['bc_dbg'][k]), _f(z['bc_dba'][k]))
                for r in range(BC_ROWS)] for k in range(len(BC_ANGLES))]
        for c, key in enumerate(('rot', 'vel', 'pos')):
            z['bc_%s_%s_ref' % (key, name)] = np.array([[_out(row[c]) for row in call] for call in out])
    # gyro-bias solve: the Jacobians of stream A's non-empty motion rows, cycled; rot_ref = rot_imu Exp(axis angle), a third negated
    full = np.nonzero(np.diff(z['a_seg']) > 0)[0]
    z['s_jac_row'] = full[np.arange(SOLVE_ROWS) % len(full)]
    ref = np.stack([_out(_qmul(_f(z['s_rot_imu'][i]), L._so3_exp(_f(z['s_axis'][i] * z['s_angle'][i])))) for i in range(SOLVE_ROWS)])
    ref[z['s_angle'] == 0.0] = z['s_rot_imu'][z['s_angle'] == 0.0]
    z['s_rot_ref'] = np.where(z['s_negated'][:, None], -ref, ref)
    z['solve_x_ref'], z['solve_H_ref'], z['s_angle_ref'] = ref_solve(solve_jac(z), z['s_rot_imu'], z['s_rot_ref'], z['s_weight'])
    # backward: stream C, then stream B
    z['bwd_gyro_single_ref'] = np.stack([ref_single(z, s) for s in range(len(z['c_dt']))])
    _GRAD_STREAM, _GRAD_COT = Stream(z['b_dt'], z['b_gyro'], z['b_acc'], z['b_seg'], GRAVITY), cotangents(z)
    S = len(z['b_dt'])
    with multiprocessing.get_context('fork').Pool(min(8, os.cpu_count() or 1)) as pool:
        for motion, mode in ((True, 'motion'), (False, 'world')):
            g = np.stack(pool.map(_grad_task, [(motion, s) for s in range(S)], chunksize=4))
            z['bwd_gyro_%s_ref' % mode], z['bwd_acc_%s_ref' % mode] = g[:, :3], g[:, 3:]
    return z


def ref_single(z, s):
    """d L / d gyro_s of stream C"""
    mp = L._mp()
    st = Stream(z['c_dt'], z['c_gyro'], z['c_acc'], z['c_seg'], 0.0)
    zero = [[mp.mpf(0)] * 3] * st.n
    return _out(st.grad(True, s, (zero, [_f(r) for r in z['c_wr']], zero))[:3])


def solve_jac(z):
    return z['jac_motion_f64_ref'][z['s_jac_row']]


def full_cov(tri):
    out = np.zeros(tri.shape[:-1] + (9, 9))
    out[..., IU[0], IU[1]] = tri
    out[..., IU[1], IU[0]] = tri
    return out


QUANTITIES = ('cov_single', 'cov_motion', 'cov_world', 'jac_single', 'jac_motion', 'jac_world', 'bwd_gyro_motion', 'bwd_acc_motion',
              'bwd_gyro_world', 'bwd_acc_world', 'bwd_gyro_single', 'bc_rot_small_f64', 'bc_rot_f64', 'bc_vel_f64', 'bc_pos_f64', 'bc_rot_f32', 'bc_vel_f32', 'bc_pos_f32', 'solve_x',
              'solve_H')
FORWARD = tuple('fwd_%s_%s_%s' % (k, mode, name) for name in DTYPES for mode in ('motion', 'world') for k in ('pos', 'rot', 'vel'))


def _rel(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max()))


def errors(z, out):
    """Per quantity the error of `out`, outputs of the code under test under the names of the references without '_ref' (any subset;
    a quantity that covers both input types takes the larger error of those present).  The measures are those of the kernels' own GPU
    tests: cs_error (tests/test_imu_cov_gpu.py) for covariances, block_error (tests/test_imu_bias_jac_gpu.py) for Jacobians,
    max|x - ref| / max|ref| for the gradients (tests/test_imu_bwd_gpu.py) and the bias estimate, h_error (tests/test_imu_align_gpu.py) for H; the corrected
    increments and the forward rows: max|x - ref| / max(1, max|ref|).  'single' = the first len(ANGLES) motion rows, one sample each;
    'bc_rot_small' = the corrections by at most 1e-2 rad, where Exp's series and its switch are not drowned by the rounding of a
    3 rad angle; 'bwd_gyro_single' = stream C."""
    from tests.test_imu_align_gpu import h_error
    from tests.test_imu_bias_jac_gpu import block_error
    from tests.test_imu_cov_gpu import cs_error
    na, o = len(ANGLES), {}

    def put(q, e):
        e, prev = float(e), o.get(q, 0.0)
        o[q] = prev if e <= prev or prev != prev else e           # (the larger one; a NaN stays)
    for name in DTYPES:
        for mode in ('motion', 'world'):
            k = 'cov_%s_%s' % (mode, name)
            if k in out:
                ref = full_cov(z[k + '_ref'])
                put('cov_' + mode, cs_error(out[k], ref))
                if mode == 'motion':
                    put('cov_single', cs_error(out[k][:na], ref[:na]))
            k = 'jac_%s_%s' % (mode, name)
            if k in out:
                put('jac_' + mode, block_error(out[k], z[k + '_ref']))
                if mode == 'motion':
                    put('jac_single', block_error(out[k][:na], z[k + '_ref'][:na]))
        for key in ('rot', 'vel', 'pos'):
            k = 'bc_%s_%s' % (key, name)
            if k in out:
                put(k, _rel(out[k], z[k + '_ref']))
                if key == 'rot' and name == 'f64':
                    put('bc_rot_small_f64', _rel(out[k][:BC_SMALL], z[k + '_ref'][:BC_SMALL]))
    for k in FORWARD:
        if k in out:
            put(k, _rel(out[k], z[k + '_ref']))
    for k in ['bwd_%s_%s' % (key, mode) for mode in ('motion', 'world') for key in ('gyro', 'acc')] + ['bwd_gyro_single']:
        if k in out:
            put(k, np.abs(out[k] - z[k + '_ref']).max() / np.abs(z[k + '_ref']).max())
    if 'solve_x' in out:
        put('solve_x', np.abs(out['solve_x'] - z['solve_x_ref']).max() / np.abs(z['solve_x_ref']).max())
        put('solve_H', h_error(out['solve_H'], z['solve_H_ref']))
    return o


def bwd_cotangents(z, motion):
    """(g_pos, g_rot, g_vel) as the backward takes them: the rotation cotangent is [wr, 0]"""
    mode = 'motion' if motion else 'world'
    wr = z['b_wr_' + mode]
    return z['b_wp_' + mode], np.concatenate([wr, np.zeros((len(wr), 1))], 1), z['b_wv_' + mode]


def transcription_outputs(z):
    """Everything errors() wants from tests/imu_f64.py."""
    from tests import imu_f64 as T
    out = {}
    for name in DTYPES:
        dt, gyro, acc = (rounded(z, k, name) for k in ('a_dt', 'a_gyro', 'a_acc'))
        for motion, mode in ((True, 'motion'), (False, 'world')):
            out['cov_%s_%s' % (mode, name)] = T.cov(dt, gyro, acc, z['a_seg'], GYRO_COV, ACC_COV, motion, z['init_cov'])
            out['jac_%s_%s' % (mode, name)] = T.bias_jac(dt, gyro, acc, z['a_seg'], motion, z['init_jac'])
        inc = [z['fwd_%s_motion_f64_ref' % k][:BC_ROWS] for k in ('rot', 'vel', 'pos')]
        calls = [T.bias_correct(z['jac_motion_f64_ref'][:BC_ROWS], *inc, z['bc_dbg'][k], z['bc_dba'][k], DTYPES[name]) for k in range(len(BC_ANGLES))]
        for c, key in enumerate(('rot', 'vel', 'pos')):
            out['bc_%s_%s' % (key, name)] = np.stack([call[c] for call in calls]).astype(np.float64)
    for motion, mode in ((True, 'motion'), (False, 'world')):
        out['bwd_gyro_' + mode], out['bwd_acc_' + mode] = T.preint_bwd(z['b_dt'], z['b_gyro'], z['b_acc'], z['b_seg'], np.array(INIT_ROT), GRAVITY,
                                                                       motion, *bwd_cotangents(z, motion))
    na = len(ANGLES)
    cot_c = (np.zeros((na, 3)), np.concatenate([z['c_wr'], np.zeros((na, 1))], 1), np.zeros((na, 3)))
    out['bwd_gyro_single'] = T.preint_bwd(z['c_dt'], z['c_gyro'], z['c_acc'], z['c_seg'], np.array(INIT_ROT), 0.0, True, *cot_c)[0]
    out['solve_x'], out['solve_H'] = T.gyro_bias_solve(solve_jac(z), z['s_rot_imu'], z['s_rot_ref'], z['s_weight'])
    return out


def forward_outputs(z):
    """oracle.cwrap.imu_integrate (the forward's bit-exact restatement) on stream A."""
    from oracle import cwrap
    out = {}
    for name, dtype in DTYPES.items():
        for motion, mode in ((True, 'motion'), (False, 'world')):
            r = cwrap.imu_integrate(z['a_dt'], z['a_gyro'], z['a_acc'], z['a_seg'], INIT_POS, INIT_ROT, INIT_VEL, GRAVITY, motion, dtype)
            for k, a in zip(('pos', 'rot', 'vel'), r):
                out['fwd_%s_%s_%s' % (k, mode, name)] = a.astype(np.float64)
    return out


def main():
    z = make_references(make_inputs())
    errs = errors(z, transcription_outputs(z))
    # floor = the float64 transcription's error; tolerance of the GPU test = 16 floors (tests/test_imu_golden_cpu.py says why)
    z['quantities'] = np.array(QUANTITIES)
    z['floors'] = np.array([errs[q] for q in QUANTITIES])
    z['tolerances'] = 16.0 * z['floors']
    ferr = errors(z, forward_outputs(z))
    z['forward_names'] = np.array(FORWARD)
    z['forward_errors'] = np.array([ferr[q] for q in FORWARD])
    np.savez_compressed(PATH, **z)
    for q, f in zip(QUANTITIES, z['floors']):
        print('%-16s floor %.3e  tolerance %.3e' % (q, f, 16 * f))
    for q, f in zip(FORWARD, z['forward_errors']):
        print('%-24s error of the forward restatement %.3e' % (q, f))
    print('%d bytes' % os.path.getsize(PATH))


if __name__ == '__main__':
    main()
