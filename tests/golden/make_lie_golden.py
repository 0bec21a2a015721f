"""Writes tests/golden/lie_cases.npz: 3-D, large-angle inputs for the PVGO kernels that are built on islam_amd/csrc/lie_dev.h, and
reference outputs computed with mpmath at 60 digits and rounded to float64.

    python -m tests.golden.make_lie_golden          (from the repository root; needs mpmath)

The reference shares nothing with the closed forms of lie_dev.h / oracle/lie.py:
  * Exp: the rotation is the power series of the quaternion exponential exp(phi/2), the translation V(phi) rho with
    V = sum_n K^n/(n+1)!, K = [phi]x, both summed until the terms vanish at the working precision (= expm of the 4x4 twist);
  * Log: phi = 2 atan2(|v|, w) v/|v| on the quaternion with w >= 0 (the principal value on SO(3): independent of the
    quaternion's sign), rho = V(phi)^-1 t;
  * Jacobians: central differences of the residual functions themselves with step 1e-25 -- G, C, B with respect to
    Xj <- Exp(delta) Xj, the vo_loss gradient with respect to P <- Exp(delta) P.  No Jl^-1 or Q formula appears.
Inputs enter the mp arithmetic exactly from their float64 values (unit quaternions are NOT re-normalised: the products are the
same Hamilton products the kernels form), so a comparison measures the rounding inside the code under test only.

The chain has M = 200 links (four 64-lane blocks, the last one partial).  The residual rotation angles of the VO factor and of the IMU
rotation factor sweep ANGLES independently; a third of the links have the far node's quaternion negated (composed w < 0); residual
translations reach 5 m.  See tests/test_lie_golden_cpu.py for how the tolerances stored here are measured."""
import os

import numpy as np

DPS = 60
M_LINKS = 200
N_EDGES = 48
N_PARTIAL = 70                   # nodes of the sign = -1 retraction and of align (one full block and a partial one)
PI = 3.141592653589793
# 0 | tiny | both sides of the so3_log switch (vn = 1e-3, th = 2e-3) | both sides of the th2 = 1e-4 switch (so3_Jl, so3_Jl_inv; so3_exp
# in the retraction) | both sides of se3_Q's switch at th2 = 1e-2, and the switch itself | large | close to pi
ANGLES = (0.0, 1e-12, 1e-8, 1e-5, 2e-3 * (1 - 1e-3), 2e-3 * (1 + 1e-3), 1e-2 * (1 - 1e-3), 1e-2 * (1 + 1e-3), 0.1 * (1 - 1e-3), 0.1,
          0.1 * (1 + 1e-3), 1.0, 2.0, 3.0, PI - 1e-3, PI - 1e-6)
DX_ANGLES = (0.0, 1e-9, 1e-2 * (1 - 1e-3), 1e-2 * (1 + 1e-3), 0.5, 3.0, 6.0)
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, 'lie_cases.npz')


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ------------------------------------------------------------------ mp arithmetic on plain lists
def _f(x):
    """float64 array -> list of exact mpf."""
    mp = _mp()
    return [mp.mpf(float(v)) for v in np.asarray(x, dtype=np.float64).reshape(-1)]


def _out(x):
    return np.array([float(v) for v in x], dtype=np.float64)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz]


def _qinv(q):
    return [-q[0], -q[1], -q[2], q[3]]


def _qact(q, p):
    u = q[:3]
    uv = [2 * c for c in _cross(u, p)]
    c2 = _cross(u, uv)
    return [p[i] + q[3] * uv[i] + c2[i] for i in range(3)]


def _mul(X, Y):
    r = _qact(X[3:], Y[:3])
    return [X[0] + r[0], X[1] + r[1], X[2] + r[2]] + _qmul(X[3:], Y[3:])


def _inv(X):
    qi = _qinv(X[3:])
    r = _qact(qi, X[:3])
    return [-r[0], -r[1], -r[2]] + qi


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _V(phi):
    """sum_n K^n / (n+1)!"""
    mp = _mp()
    tiny = mp.mpf(10) ** -(DPS + 4)
    K = [[0, -phi[2], phi[1]], [phi[2], 0, -phi[0]], [-phi[1], phi[0], 0]]
    S = [[mp.mpf(i == j) for j in range(3)] for i in range(3)]
    term = [row[:] for row in S]
    n = 1
    while True:
        term = [[v / (n + 1) for v in row] for row in _mm(term, K)]
        S = [[S[i][j] + term[i][j] for j in range(3)] for i in range(3)]
        if max(abs(v) for row in term for v in row) < tiny:
            return S
        n += 1


def _so3_exp(phi):
    mp = _mp()
    tiny = mp.mpf(10) ** -(DPS + 4)
    p = [phi[0] / 2, phi[1] / 2, phi[2] / 2, mp.mpf(0)]
    term = [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)]
    S = term[:]
    n = 1
    while True:
        term = [v / n for v in _qmul(term, p)]
        S = [S[i] + term[i] for i in range(4)]
        if max(abs(v) for v in term) < tiny:
            return S
        n += 1


def _exp(xi):
    V = _V(xi[3:])
    return [sum(V[i][j] * xi[j] for j in range(3)) for i in range(3)] + _so3_exp(xi[3:])


def _so3_log(q):
    mp = _mp()
    if q[3] < 0:
        q = [-v for v in q]
    vn = mp.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    if vn == 0:
        return [mp.mpf(0)] * 3
    f = 2 * mp.atan2(vn, q[3]) / vn
    return [f * q[0], f * q[1], f * q[2]]


def _solve3(A, b):
    det = (A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0])
           + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]))
    out = []
    for c in range(3):
        B = [[b[i] if j == c else A[i][j] for j in range(3)] for i in range(3)]
        out.append((B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0])
                    + B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0])) / det)
    return out


def _log(X):
    phi = _so3_log(X[3:])
    return _solve3(_V(phi), X[:3]) + phi


def _central(fun, n):
    """Columns d fun / d delta_c, c < n, by central differences with step 1e-25 (error ~1e-50 f''' + 1e-35 rounding)."""
    mp = _mp()
    h = mp.mpf(10) ** -25
    cols = []
    for c in range(n):
        d = [mp.mpf(0)] * n
        d[c] = h
        fp = fun(d)
        d[c] = -h
        fm = fun(d)
        cols.append([(a - b) / (2 * h) for a, b in zip(fp, fm)])
    return cols           # cols[c][r]


# ------------------------------------------------------------------ references, one case at a time
def ref_vo(Xi, Xj, P):
    """e (6), G (9), C (9) of one VO factor: e = Log(P^-1 Xi^-1 Xj), derivative w.r.t. Xj <- Exp(delta) Xj."""
    pre = _mul(_inv(P), _inv(Xi))
    e = _log(_mul(pre, Xj))
    J = _central(lambda d: _log(_mul(pre, _mul(_exp(d), Xj))), 6)
    G = [J[c][r] for r in range(3) for c in range(3)]
    C = [J[c][r] for r in range(3) for c in range(3, 6)]
    return e, G, C


def ref_link(z, k):
    """Column k of lin (42 mpf) and the link's sum of squared residuals."""
    Xi, Xj = _f(z['nodes'][k]), _f(z['nodes'][k + 1])
    vi, vj = _f(z['vels'][k]), _f(z['vels'][k + 1])
    e, G, C = ref_vo(Xi, Xj, _f(z['poses'][k]))
    rpre = _qmul(_qinv(_f(z['drots'][k])), _qinv(Xi[3:]))
    er = _so3_log(_qmul(rpre, Xj[3:]))
    JB = _central(lambda d: _so3_log(_qmul(rpre, _qmul(_so3_exp(d), Xj[3:]))), 3)
    B = [JB[c][r] for r in range(3) for c in range(3)]
    dv, dp, dt = _f(z['dvels'][k]), _f(z['dtrans'][k]), _f(z['dts'][k])[0]
    rv = [dv[i] - (vj[i] - vi[i]) for i in range(3)]
    rt = [(Xj[i] - Xi[i]) - (dt * vi[i] + dp[i]) for i in range(3)]
    col = e + G + C + er + B + rv + rt
    return col, sum(v * v for v in e + er + rv + rt)


def ref_retract(z, n, sign):
    d = [sign * v for v in _f(z['dx'][n])]
    return _mul(_exp(d[:6]), _f(z['nodes'][n])) + [a + b for a, b in zip(_f(z['vels'][n]), d[6:])]


def ref_edge(z, e):
    """linearize_edges record (24), trans/rot loss (2), vo_loss gradient w.r.t. P <- Exp(delta) P under the weights (6)."""
    i, j = z['edges'][e]
    Xi, Xj, P = _f(z['nodes'][i]), _f(z['nodes'][j]), _f(z['edge_poses'][e])
    err, G, C = ref_vo(Xi, Xj, P)
    gt, gr = _f(z['g_trans'][e])[0], _f(z['g_rot'][e])[0]
    rel = _mul(_inv(Xi), Xj)

    def loss(d):
        r = _log(_mul(_inv(_mul(_exp(d), P)), rel))
        return [gt * sum(v * v for v in r[:3]) + gr * sum(v * v for v in r[3:])]
    g = [c[0] for c in _central(loss, 6)]
    return err + G + C, [sum(v * v for v in err[:3]), sum(v * v for v in err[3:])], g


def ref_align(z, n):
    T, S = _f(z['align_target']), _f(z['nodes'][0])
    X = _mul(_mul(T, _inv(S)), _f(z['nodes'][n]))
    return X + _qact(_qmul(T[3:], _qinv(S[3:])), _f(z['vels'][n]))


def ref_trial_link(z, k):
    """(sum r^2 at Exp(dx) X, JD.(2R+JD) with J, R = the float64 reference linearisation lin_ref) of link k."""
    Xi, Xj = ref_retract(z, k, 1), ref_retract(z, k + 1, 1)
    vi, vj = Xi[7:], Xj[7:]
    Xi, Xj = Xi[:7], Xj[:7]
    pre = _mul(_inv(_f(z['poses'][k])), _inv(Xi))
    e = _log(_mul(pre, Xj))
    er = _so3_log(_qmul(_qmul(_qinv(_f(z['drots'][k])), _qinv(Xi[3:])), Xj[3:]))
    dv, dp, dt = _f(z['dvels'][k]), _f(z['dtrans'][k]), _f(z['dts'][k])[0]
    rv = [dv[i] - (vj[i] - vi[i]) for i in range(3)]
    rt = [(Xj[i] - Xi[i]) - (dt * vi[i] + dp[i]) for i in range(3)]
    # the residual angles the trial step lands on are random: they must stay clear of pi, where the logarithm's sign is a convention
    assert max(sum(v * v for v in e[3:]), sum(v * v for v in er)) < (PI - 5e-7) ** 2, k
    sq = sum(v * v for v in e + er + rv + rt)
    L = _f(z['lin_ref'][:, k])
    di, dj = _f(z['dx'][k]), _f(z['dx'][k + 1])
    ddr, ddp = [dj[i] - di[i] for i in range(3)], [dj[3 + i] - di[3 + i] for i in range(3)]
    m = lambda o, v: [sum(L[o + 3 * r + c] * v[c] for c in range(3)) for r in range(3)]
    j0 = [a + b for a, b in zip(m(6, ddr), m(15, ddp))]
    j1, j3 = m(6, ddp), m(27, ddp)
    j2 = [di[6 + i] - dj[6 + i] for i in range(3)]
    j4 = [ddr[i] - dt * di[6 + i] for i in range(3)]
    qd = 0
    for j, o in ((j0, 0), (j1, 3), (j2, 36), (j3, 24), (j4, 39)):
        qd += sum(j[i] * (2 * L[o + i] + j[i]) for i in range(3))
    return sq, qd


# ------------------------------------------------------------------ inputs
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _norm_q(X):
    mp = _mp()
    n = mp.sqrt(sum(v * v for v in X[-4:]))
    return X[:-4] + [v / n for v in X[-4:]]


def make_inputs():
    rng = np.random.default_rng(20240611)
    M, N, E = M_LINKS, M_LINKS + 1, N_EDGES
    na = len(ANGLES)
    q = rng.normal(size=(N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q = np.where(q[:, 3:] < 0, -q, q)
    # translations within +-10 m; every third node close to the origin, so that some Jacobians are O(1) and not O(|t|)
    t = rng.uniform(-10, 10, (N, 3)) * np.where(np.arange(N) % 3 == 0, 0.02, 1.0)[:, None]
    nodes = np.concatenate([t, q], 1)
    vels = rng.uniform(-5, 5, (N, 3))
    dts = rng.uniform(0.05, 0.2, M)
    vo_ang = np.array([ANGLES[(5 * k) % na] for k in range(M)])
    imu_ang = np.array([ANGLES[(5 * k + 5 + k // na) % na] for k in range(M)])
    rho_len = np.where(np.arange(M) % 5 == 0, 5.0, rng.uniform(0, 5, M))
    E_vo = np.concatenate([_unit(rng, M) * rho_len[:, None], _unit(rng, M) * vo_ang[:, None]], 1)
    E_imu = _unit(rng, M) * imu_ang[:, None]
    flip = (np.arange(M) // na + np.arange(M)) % 3 == 2
    poses, drots = np.zeros((M, 7)), np.zeros((M, 4))
    for k in range(M):
        if vo_ang[k] == 0.0:                        # Xi == Xj, P the identity
            nodes[k + 1] = nodes[k]
            poses[k] = [0, 0, 0, 0, 0, 0, 1]
        else:
            poses[k] = _out(_norm_q(_mul(_mul(_inv(_f(nodes[k])), _f(nodes[k + 1])), _inv(_exp(_f(E_vo[k]))))))
        drots[k] = _out(_norm_q(_qmul(_qmul(_qinv(_f(nodes[k, 3:])), _f(nodes[k + 1, 3:])), _qinv(_so3_exp(_f(E_imu[k]))))))
        if flip[k]:                                 # double cover: the composed quaternions of link k get w < 0
            nodes[k + 1, 3:] = -nodes[k + 1, 3:]
    dvels = (vels[1:] - vels[:-1]) + rng.uniform(-1, 1, (M, 3))
    dtrans = (nodes[1:, :3] - nodes[:-1, :3]) - dts[:, None] * vels[:-1] + rng.uniform(-1, 1, (M, 3))
    # retraction updates: rotation sweep about random axes, translation / velocity parts up to 5
    dx = np.concatenate([_unit(rng, N) * rng.uniform(0, 5, (N, 1)),
                         _unit(rng, N) * np.array([DX_ANGLES[n % len(DX_ANGLES)] for n in range(N)])[:, None],
                         rng.uniform(-5, 5, (N, 3))], 1)
    # arbitrary edges: j = i + 1, i > j (neighbours and far), long range
    edges = []
    for e in range(E):
        a = int(rng.integers(0, N - 1))
        kind = e % 4
        if kind == 0:
            edges.append((a, a + 1))
        elif kind == 1:
            edges.append((a + 1, a))
        else:
            b = int((a + rng.integers(40, 160)) % N)
            edges.append((max(a, b), min(a, b)) if kind == 2 else (min(a, b), max(a, b)))
    edges = np.array(edges, dtype=np.int64)
    e_ang = np.array([ANGLES[(5 * e + 1) % na] for e in range(E)])
    E_e = np.concatenate([_unit(rng, E) * rng.uniform(0, 5, (E, 1)), _unit(rng, E) * e_ang[:, None]], 1)
    edge_poses = np.zeros((E, 7))
    for e, (i, j) in enumerate(edges):
        edge_poses[e] = _out(_norm_q(_mul(_mul(_inv(_f(nodes[i])), _f(nodes[j])), _inv(_exp(_f(E_e[e]))))))
        if e % 3 == 1:
            edge_poses[e, 3:] = -edge_poses[e, 3:]
    tq = rng.normal(size=4)
    align_target = np.concatenate([rng.uniform(-10, 10, 3), tq / np.linalg.norm(tq)])
    return dict(nodes=nodes, vels=vels, poses=poses, drots=drots, dtrans=dtrans, dvels=dvels, dts=dts, dx=dx, edges=edges,
                edge_poses=edge_poses, g_trans=rng.uniform(0.5, 1.5, E), g_rot=rng.uniform(1.0, 2.0, E), align_target=align_target,
                vo_angle=vo_ang, imu_angle=imu_ang, flipped=flip)


def make_references(z):
    M, N, E = M_LINKS, M_LINKS + 1, N_EDGES
    nblk = (M + 63) // 64
    mp = _mp()
    lin, sq = np.zeros((42, M)), []
    for k in range(M):
        col, s = ref_link(z, k)
        lin[:, k] = _out(col)
        sq.append(s)
    z['lin_ref'] = lin
    z['loss_part_ref'] = _out([sum(sq[64 * b:64 * b + 64], mp.mpf(0)) for b in range(nblk)])
    z['retract_pos_ref'] = np.stack([_out(ref_retract(z, n, 1)) for n in range(N)])
    z['retract_neg_ref'] = np.stack([_out(ref_retract(z, n, -1)) for n in range(N_PARTIAL)])
    z['align_ref'] = np.stack([_out(ref_align(z, n)) for n in range(N_PARTIAL)])
    er = [ref_edge(z, e) for e in range(E)]
    z['edge_lin_ref'] = np.stack([_out(r[0]) for r in er], 1)
    z['vo_loss_ref'] = np.stack([_out(r[1]) for r in er])
    z['vo_grad_ref'] = np.stack([_out(r[2]) for r in er])
    tl = [ref_trial_link(z, k) for k in range(M)]
    z['trial_link_ref'] = np.stack([_out(r) for r in tl])
    z['trial_part_ref'] = np.stack([_out([sum((r[c] for r in tl[64 * b:64 * b + 64]), mp.mpf(0)) for c in range(2)])
                                    for b in range(nblk)])
    return z


QUANTITIES = ('res', 'G', 'C', 'B', 'loss_part', 'retract_nodes', 'retract_vels', 'edge_e', 'edge_G', 'edge_C', 'vo_loss', 'vo_grad',
              'align_nodes', 'align_vels', 'trial_nodes', 'trial_vels', 'trial_sq', 'trial_qd')


def case_errors(z, out):
    """Per quantity, the error of every case: max|x - ref| / max(1, max|ref|) over the entries of that quantity in that case.
    `out` holds outputs of the code under test (any subset of the groups) under the names of tests.lie_f64 / the kernels:
    lin (42,M), loss_part, retract_pos (nodes, vels), retract_neg, edge_lin (24,E), vo_loss (tl, rl), vo_grad (E,7), align (nodes, vels),
    trial (nodes_t, vels_t, part (nblk,2))."""
    def err(x, ref):
        x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        x, ref = x.reshape(len(ref), -1), ref.reshape(len(ref), -1)
        return np.abs(x - ref).max(1) / np.maximum(1.0, np.abs(ref).max(1))
    rp, rn, al = z['retract_pos_ref'], z['retract_neg_ref'], z['align_ref']
    o = {}
    if 'lin' in out:
        L, R = out['lin'].T, z['lin_ref'].T
        res_rows = np.r_[0:6, 24:27, 36:42]
        o.update(res=err(L[:, res_rows], R[:, res_rows]), G=err(L[:, 6:15], R[:, 6:15]), C=err(L[:, 15:24], R[:, 15:24]),
                 B=err(L[:, 27:36], R[:, 27:36]), loss_part=err(out['loss_part'], z['loss_part_ref']))
    if 'retract_pos' in out:
        o.update(retract_nodes=np.concatenate([err(out['retract_pos'][0], rp[:, :7]), err(out['retract_neg'][0], rn[:, :7])]),
                 retract_vels=np.concatenate([err(out['retract_pos'][1], rp[:, 7:]), err(out['retract_neg'][1], rn[:, 7:])]))
    if 'edge_lin' in out:
        EL, ER = out['edge_lin'].T, z['edge_lin_ref'].T
        o.update(edge_e=err(EL[:, :6], ER[:, :6]), edge_G=err(EL[:, 6:15], ER[:, 6:15]), edge_C=err(EL[:, 15:24], ER[:, 15:24]))
    if 'vo_loss' in out:
        o.update(vo_loss=err(np.stack(out['vo_loss'], 1), z['vo_loss_ref']), vo_grad=err(out['vo_grad'][:, :6], z['vo_grad_ref']))
    if 'align' in out:
        o.update(align_nodes=err(out['align'][0], al[:, :7]), align_vels=err(out['align'][1], al[:, 7:]))
    if 'trial' in out:
        o.update(trial_nodes=err(out['trial'][0], rp[:, :7]), trial_vels=err(out['trial'][1], rp[:, 7:]),
                 trial_sq=err(out['trial'][2][:, 0], z['trial_part_ref'][:, 0]), trial_qd=err(out['trial'][2][:, 1], z['trial_part_ref'][:, 1]))
    return o


def transcription_outputs(z):
    """Everything case_errors wants, from the float64 transcription tests/lie_f64.py."""
    from tests import lie_f64 as L
    a = (z['nodes'], z['vels'], z['poses'], z['drots'], z['dtrans'], z['dvels'], z['dts'])
    lin, part = L.linearize(*a)
    err6, tl, rl = L.vo_loss_fwd(z['nodes'], z['edges'], z['edge_poses'])
    n = N_PARTIAL
    return dict(lin=lin, loss_part=part, retract_pos=L.retract(z['nodes'], z['vels'], z['dx'], 1.0),
                retract_neg=L.retract(z['nodes'][:n], z['vels'][:n], z['dx'][:n], -1.0),
                edge_lin=L.linearize_edges(z['nodes'], z['edges'], z['edge_poses']), vo_loss=(tl, rl),
                vo_grad=L.vo_loss_bwd(z['edge_poses'], err6, z['g_trans'], z['g_rot']),
                align=L.align(z['nodes'][:n], z['vels'][:n], z['align_target']),
                trial=L.trial(*a[:2], z['dx'], *a[2:], z['lin_ref'])[:3])


def main():
    z = make_references(make_inputs())
    errs = case_errors(z, transcription_outputs(z))
    # floor = the float64 transcription's largest error over the cases; tolerance of the GPU test = 16 floors (an ulp or two in
    # sincos / atan / sqrt and contracted multiply-adds, carried through a handful of chained products: one order of magnitude)
    z['quantities'] = np.array(QUANTITIES)
    z['floors'] = np.array([errs[q].max() for q in QUANTITIES])
    z['tolerances'] = 16.0 * z['floors']
    np.savez(PATH, **z)
    for q, f in zip(QUANTITIES, z['floors']):
        print('%-14s floor %.3e  tolerance %.3e' % (q, f, 16 * f))
    print('%d bytes' % os.path.getsize(PATH))


if __name__ == '__main__':
    main()
