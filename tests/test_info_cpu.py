"""Per-factor information matrices of the PVGO LM (islam_amd.information, run_pvgo(info=...)) on the CPU: a
float64 restatement of the LM under block-diagonal weights (oracle.pvgo.LM.step with W = block_diag(Omega_k); dense, and banded with
per-link matrices for longer chains) that tests/test_info_gpu.py runs the HIP back-end against, the input condition of every case
that file uses, and PvgoInfo / PvgoInfo.from_imu_cov themselves."""
import functools

import numpy as np
import pytest

from oracle import pvgo as opvgo
from tests.helpers import chain_problem

UNIT = (1, 1, 1, 1)
LW = (1, 0.1, 10, 0.1)
GROUP_ROWS = (6, 3, 3, 3)
LONG_EDGES = (3, 11, 19, 28)          # the four long edges of closure_problem()


# ------------------------------------------------------------------ the restatement
class _DenseLinInfo(opvgo._DenseLin):
    """oracle.pvgo._DenseLin with W = block_diag(Omega_k); drop: VO edges whose rows are taken out of the normal equations."""

    def __init__(self, nodes, inp, res, A_e, B_k, omegas, drop=()):
        edges, dts = inp[0], inp[5]
        N = nodes.shape[0]
        self.N, self.dt = N, nodes.dtype
        self.J = opvgo.jacobian_dense(N, edges, A_e, B_k, dts, False, nodes)
        R = np.concatenate([r.reshape(-1) for r in res])
        WJ, WR = np.zeros_like(self.J), np.zeros_like(R)
        r0 = 0
        for g, (k, Om) in enumerate(zip(GROUP_ROWS, omegas)):
            n = Om.shape[0]
            rows = slice(r0, r0 + n * k)
            WJ[rows] = np.einsum('nij,njc->nic', Om, self.J[rows].reshape(n, k, -1)).reshape(n * k, -1)
            WR[rows] = np.einsum('nij,nj->ni', Om, R[rows].reshape(n, k)).reshape(-1)
            r0 += n * k
        keep = np.ones(self.J.shape[0], dtype=bool)
        for e in drop:
            keep[6 * e:6 * e + 6] = False
        self.A = self.J[keep].T @ WJ[keep]
        self.A = 0.5 * (self.A + self.A.T)
        self.b = -(self.J[keep].T @ WR[keep])
        self.diag = np.diagonal(self.A).copy()


class _BandedLinInfo(opvgo._BandedLin):
    """oracle.pvgo._BandedLin with one information matrix per link and group: the contract's table."""

    def __init__(self, nodes, inp, res, A_e, B_k, omegas):
        dts = np.asarray(inp[5]).reshape(-1)
        N = nodes.shape[0]
        M = N - 1
        dt = nodes.dtype
        self.N, self.dt, self.A_e, self.B_k, self.dts, self.J_rp = N, dt, A_e, B_k, dts, None
        O0, O1, O2, O3 = omegas
        e, rv, er, rt = res[:4]
        T = lambda a: np.swapaxes(a, 1, 2)
        mv = lambda a, v: (a @ v[:, :, None])[:, :, 0]
        S = T(A_e) @ O0 @ A_e
        S[:, :3, :3] += O3
        S[:, 3:, 3:] += T(B_k) @ O2 @ B_k
        S = 0.5 * (S + T(S))
        Hd = np.zeros((N, 9, 9), dt)
        Ho = np.zeros((M, 9, 9), dt)
        Hd[:-1, :6, :6] += S
        Hd[1:, :6, :6] += S
        Ho[:, :6, :6] = -S
        Hd[:-1, 6:, 6:] += O1 + (dts * dts)[:, None, None] * O3
        Hd[1:, 6:, 6:] += O1
        Ho[:, 6:, 6:] = -O1
        c = dts[:, None, None] * O3
        Hd[:-1, 0:3, 6:9] += c
        Hd[:-1, 6:9, 0:3] += c
        Ho[:, 6:9, 0:3] += -c
        gp = mv(T(A_e) @ O0, e)
        gp[:, 3:] += mv(T(B_k) @ O2, er)
        gp[:, :3] += mv(O3, rt)
        g = np.zeros((N, 9), dt)
        g[1:, :6] += gp
        g[:-1, :6] -= gp
        g[:-1, 6:] += mv(O1, rv) - dts[:, None] * mv(O3, rt)
        g[1:, 6:] -= mv(O1, rv)
        self.Hd, self.Ho = Hd, Ho
        self.b = (-g).reshape(-1)
        ab = np.zeros((18, 9 * N), dt)
        for r in range(9):
            for cc in range(9):
                if r >= cc:
                    ab[r - cc, cc::9] = Hd[:, r, cc]
                ab[9 + cc - r, r:9 * M:9] = Ho[:, r, cc]
        self.ab = ab
        self.diag = ab[0].copy()


class InfoLM(opvgo.LM):
    """oracle.pvgo.LM.step with W = block_diag(Omega_k) in the normal equations.  The loss and the trust-region term stay unweighted;
    clamp, cumulative damping and the reject limit are unchanged."""

    def __init__(self, nodes, vels, omegas, drop=(), **kw):
        super().__init__(nodes, vels, **kw)
        self.omegas, self.drop = omegas, tuple(drop)

    def step(self, inp, loss_weight):
        edges, poses, drots = inp[0], inp[1], inp[2]
        res = self._res(inp)
        R = np.concatenate([r.reshape(-1) for r in res])
        A_e, B_k = opvgo.jac_blocks(self.nodes, edges, poses, drots, res[0], res[2])
        if self.mode == 'dense':
            lin = _DenseLinInfo(self.nodes, inp, res, A_e, B_k, self.omegas, self.drop)
        else:
            assert not self.drop
            lin = _BandedLinInfo(self.nodes, inp, res, A_e, B_k, self.omegas)
        if self.loss is None:
            self.loss = opvgo.loss_unweighted(res)
        self.last = self.loss
        d = np.clip(lin.diag, self.min, self.max)
        self.reject_count = 0
        pg = self.strategy.pg
        while self.last <= self.loss:
            d = d + d * pg['damping']
            try:
                Dn, Dv = lin.solve(d)
            except (np.linalg.LinAlgError, opvgo.sla.LinAlgError):
                break
            self.nodes, self.vels = opvgo.retract(self.nodes, self.vels, Dn, Dv)
            self.loss = opvgo.loss_unweighted(self._res(inp))
            self.strategy.update(self.last, self.loss, lin.JD(Dn, Dv), R)
            if self.last < self.loss and self.reject_count < self.reject:
                self.nodes, self.vels = opvgo.retract(self.nodes, self.vels, -Dn, -Dv)
                self.trace.append((self.loss, pg['damping'], False, self.last))
                self.loss, self.reject_count = self.last, self.reject_count + 1
            else:
                self.trace.append((self.loss, pg['damping'], True, self.last))
                break
        self.step_losses.append(self.loss)
        return self.loss


def _inputs(prob):
    c = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    inp = (np.asarray(prob['links'], dtype=np.int64), c(prob['vo_motions']), c(prob['imu_drots']), c(prob['imu_dtrans']),
           c(prob['imu_dvels']), c(prob['dts']))
    return c(prob['init_nodes']), c(prob['init_vels']), inp


def run_info(prob, omegas, loss_weight=UNIT, mode='dense', drop=(), radius=1e4, max_steps=10):
    """oracle.pvgo.run_pvgo's loop with InfoLM (omegas None: oracle.pvgo.LM).  Returns (aligned nodes, aligned vels, optimizer)."""
    nodes0, vels0, inp = _inputs(prob)
    if omegas is None:
        opt = opvgo.LM(nodes0, vels0, radius=radius, vmin=1e-4, mode=mode)
    else:
        opt = InfoLM(nodes0, vels0, omegas, drop, radius=radius, vmin=1e-4, mode=mode)
    sched = opvgo.StopOnPlateau(opt, steps=max_steps, patience=3, decreasing=1e-3)
    while sched.continual():
        sched.step(opt.step(inp, loss_weight))
    nodes, vels = opvgo.align_to(opt.nodes, opt.vels, nodes0[0])
    return nodes, vels, opt


def margin(opt):
    """Smallest |last - loss| / last over the trials of an InfoLM run: how far every accept / reject verdict is from flipping."""
    return min(abs(t[3] - t[0]) / t[3] for t in opt.trace)


def pattern(opt):
    return ''.join('A' if t[2] else 'r' for t in opt.trace)


# ------------------------------------------------------------------ inputs
def random_omegas(E, M, lw, seed):
    """Omega_k = lw_g^2 Q diag(lambda) Q^T: Q from the QR of a seeded normal matrix, lambda log-uniform in [1/4, 4] (cond <= 16)."""
    rng = np.random.default_rng(seed)
    out = []
    for g, k in enumerate(GROUP_ROWS):
        Om = np.zeros((E if g == 0 else M, k, k))
        for i in range(Om.shape[0]):                       # factor by factor: Q, then lambda
            Q = np.linalg.qr(rng.normal(size=(k, k)))[0]
            lam = np.exp(rng.uniform(np.log(0.25), np.log(4.0), k))
            Om[i] = float(lw[g]) ** 2 * (Q * lam) @ Q.T
        out.append(0.5 * (Om + np.swapaxes(Om, 1, 2)))
    return out


def scalar_omegas(E, M, lw):
    return [np.broadcast_to(float(lw[g]) ** 2 * np.eye(k), (E if g == 0 else M, k, k)).copy() for g, k in enumerate(GROUP_ROWS)]


def closure_problem():
    """The 33-node loop-closure graph of tests/test_robust_gpu.py."""
    from tests.test_robust_gpu import _closure_problem
    return _closure_problem(33, {3: (0, 9), 11: (4, 17), 19: (30, 2), 25: (25, 26), 28: (31, 8)})


# every case tests/test_info_gpu.py runs against the restatement: name -> (N, loss weights, restatement mode)
CHAIN_CASES = {'n2': (2, UNIT, 'dense'), 'n9': (9, UNIT, 'dense'), 'n17': (17, UNIT, 'dense'), 'n130': (130, UNIT, 'banded'),
               'n257': (257, UNIT, 'banded'), 'n2_lw': (2, LW, 'dense'), 'n130_lw': (130, LW, 'banded')}


@functools.lru_cache(maxsize=None)
def chain_case(name):
    """(problem, omegas, loss weights, (nodes, vels, optimizer) of the restatement), computed once."""
    N, lw, mode = CHAIN_CASES[name]
    prob, _ = chain_problem(N)
    om = random_omegas(N - 1, N - 1, lw, 100 + N)
    return prob, om, lw, run_info(prob, om, lw, mode)


@functools.lru_cache(maxsize=None)
def closure_case(zero_long=False):
    prob = closure_problem()
    om = random_omegas(32, 32, UNIT, 133)
    if zero_long:
        om[0][list(LONG_EDGES)] = 0.0
    return prob, om, UNIT, run_info(prob, om, UNIT, 'dense', drop=LONG_EDGES if zero_long else ())


def pvgo_info(om):
    from islam_amd.information import PvgoInfo
    return PvgoInfo(vo=om[0], vel=om[1], rot=om[2], transvel=om[3])


# ------------------------------------------------------------------ tests: the restatement
@pytest.mark.parametrize('N,mode', [(2, 'dense'), (9, 'dense'), (17, 'dense'), (130, 'dense'), (130, 'banded')])
@pytest.mark.parametrize('lw', [UNIT, LW])
def test_scalar_information_takes_the_oracle_lms_steps(N, mode, lw):
    prob, _ = chain_problem(N)
    n0, v0, ref = run_info(prob, None, lw, mode)
    n1, v1, got = run_info(prob, scalar_omegas(N - 1, N - 1, lw), lw, mode)
    assert len(got.trace) == len(ref.trace) and len(got.step_losses) == len(ref.step_losses)
    assert [t[2] for t in got.trace] == [t[2] for t in ref.trace]
    np.testing.assert_allclose(n1, n0, atol=1e-12, rtol=0)
    np.testing.assert_allclose(v1, v0, atol=1e-12, rtol=0)


@pytest.mark.parametrize('N', [9, 17, 130])
def test_dense_and_banded_restatements_agree(N):
    prob, _ = chain_problem(N)
    om = random_omegas(N - 1, N - 1, UNIT, 100 + N)
    nd, vd, od = run_info(prob, om, UNIT, 'dense')
    nb, vb, ob = run_info(prob, om, UNIT, 'banded')
    assert pattern(od) == pattern(ob)
    np.testing.assert_allclose([t[0] for t in od.trace], [t[0] for t in ob.trace], rtol=1e-10)
    np.testing.assert_allclose([t[1] for t in od.trace], [t[1] for t in ob.trace], rtol=1e-10)
    np.testing.assert_allclose(nd, nb, atol=1e-9)
    np.testing.assert_allclose(vd, vb, atol=1e-9)


MARGIN = 1e-7      # a 1e-10 device difference in a trial loss cannot flip a verdict
# accept (A) / reject (r) per trial, as measured on this restatement (n2: the reject limit is reached)
PATTERNS = {'n2': 'A' + 16 * 'r' + 'A', 'n9': 'ArrrArrArrArArA', 'n17': 'AArrArrrArrArrArA', 'n130': 10 * 'A', 'n257': 10 * 'A',
            'n2_lw': 'AA' + 16 * 'r' + 'A', 'n130_lw': 'ArrrrrArArA', 'closure': 'rrrrArArArArArAAA'}


@pytest.mark.parametrize('name', sorted(CHAIN_CASES))
def test_input_condition_of_the_chain_cases(name):
    """Every trial of every case the GPU tests use keeps |last - loss| >= 1e-7 last, and the case cannot pass on scalar weights."""
    prob, om, lw, (nodes, vels, opt) = chain_case(name)
    print(name, len(opt.trace), 'trials', pattern(opt), 'margin %.2e' % margin(opt))
    assert margin(opt) >= MARGIN and pattern(opt) == PATTERNS[name]
    n0, _, _ = run_info(prob, None, lw, CHAIN_CASES[name][2])
    assert np.abs(nodes - n0).max() > 4e-4


@pytest.mark.parametrize('zero_long', [False, True])
def test_input_condition_of_the_closure_cases(zero_long):
    prob, om, lw, (nodes, vels, opt) = closure_case(zero_long)
    print('closure', zero_long, len(opt.trace), 'trials', pattern(opt), 'margin %.2e' % margin(opt))
    assert margin(opt) >= MARGIN and (zero_long or pattern(opt) == PATTERNS['closure'])
    n0, _, _ = run_info(prob, None, lw, 'dense')
    assert np.abs(nodes - n0).max() > 4e-4


def test_zero_information_equals_dropped_rows():
    """Omega = 0 on the long edges (what the device is given) and those rows taken out of the normal equations: the same LM."""
    prob, om, lw, (nodes, vels, opt) = closure_case(True)
    n1, v1, o1 = run_info(prob, om, lw, 'dense')
    assert pattern(o1) == pattern(opt)
    np.testing.assert_allclose(n1, nodes, atol=1e-12)
    np.testing.assert_allclose(v1, vels, atol=1e-12)


# ------------------------------------------------------------------ tests: PvgoInfo
def test_pvgo_info_shapes_and_symmetrisation():
    from islam_amd.information import PvgoInfo
    rng = np.random.default_rng(0)
    s = rng.uniform(0.5, 2.0, 5)
    d = rng.uniform(0.5, 2.0, (5, 6))
    full = random_omegas(5, 4, UNIT, 1)
    info = PvgoInfo(vo=s, vel=rng.uniform(0.5, 2, (4, 3)), rot=full[2])
    vo, vel, rot, tv = info.matrices(5, 4, (1, 2, 3, 0.5))
    np.testing.assert_array_equal(vo, s[:, None, None] * np.eye(6))
    assert vel.shape == (4, 3, 3) and np.all(vel[:, 0, 1] == 0)
    np.testing.assert_array_equal(rot, full[2])
    np.testing.assert_array_equal(tv, np.broadcast_to(0.25 * np.eye(3), (4, 3, 3)))          # None: loss_weight[g]^2 I
    np.testing.assert_array_equal(PvgoInfo(vo=d).vo, np.stack([np.diag(x) for x in d]))
    skew = full[0].copy()
    skew[:, 0, 1] += 0.01                                                       # not symmetric: (O + O^T) / 2
    got = PvgoInfo(vo=skew).vo
    np.testing.assert_allclose(got, 0.5 * (skew + np.swapaxes(skew, 1, 2)), rtol=0, atol=0)
    np.testing.assert_array_equal(got, np.swapaxes(got, 1, 2))
    import torch
    np.testing.assert_array_equal(PvgoInfo(vo=torch.tensor(full[0])).vo, full[0])
    zero = PvgoInfo(vo=np.zeros((5, 6, 6)))                                     # semi-definite: allowed
    assert not zero.vo.any()
    c = info.covs(5, 4, (1, 2, 3, 0.5))
    assert sorted(c) == ['imu_rot', 'imu_vel', 'transvel', 'vo_rot', 'vo_trans']
    np.testing.assert_allclose(c['vo_trans'], s)
    np.testing.assert_allclose(c['imu_rot'], np.trace(full[2], axis1=1, axis2=2) / 3)
    np.testing.assert_allclose(c['transvel'], 0.25)


def test_pvgo_info_packed_layout():
    om = random_omegas(7, 7, LW, 3)
    info = pvgo_info(om)
    info.transvel = None
    info_vo, info_imu = info.packed(7, 7, LW, 'cpu')
    assert info_vo.shape == (21, 7) and info_imu.shape == (18, 7) and info_vo.is_contiguous() and info_imu.is_contiguous()
    assert str(info_vo.dtype) == 'torch.float64'
    want_vo, want_imu = np.zeros((21, 7)), np.zeros((18, 7))
    tv = LW[3] ** 2 * np.eye(3)
    for k in range(7):
        c = 0
        for r in range(6):
            for cc in range(r, 6):
                want_vo[c, k] = om[0][k][r, cc]
                c += 1
        c = 0
        for m in (om[1][k], om[2][k], tv):
            for r in range(3):
                for cc in range(r, 3):
                    want_imu[c, k] = m[r, cc]
                    c += 1
    np.testing.assert_array_equal(info_vo.numpy(), want_vo)
    np.testing.assert_array_equal(info_imu.numpy(), want_imu)


def test_pvgo_info_validation_errors():
    from islam_amd.information import PvgoInfo
    good = random_omegas(4, 4, UNIT, 2)
    with pytest.raises(ValueError, match='vo.*shape'):
        PvgoInfo(vo=np.ones((4, 5)))
    with pytest.raises(ValueError, match='rot.*shape'):
        PvgoInfo(rot=np.ones((4, 3, 4)))
    with pytest.raises(ValueError, match='vel.*shape'):
        PvgoInfo(vel=np.float64(1.0))
    bad = good[1].copy()
    bad[2, 0, 0] = np.nan
    with pytest.raises(ValueError, match='vel: factor 2 .*non-finite'):
        PvgoInfo(vel=bad)
    bad = good[0].copy()
    bad[1] = -bad[1]
    bad[3] = -bad[3]
    with pytest.raises(ValueError, match='vo: factor 1 is not positive semi-definite'):
        PvgoInfo(vo=bad)
    with pytest.raises(ValueError, match='transvel: factor 0'):
        PvgoInfo(transvel=np.array([-1.0, 1.0]))
    assert PvgoInfo(vo=bad, validate=False).vo.shape == (4, 6, 6)               # validate=False: taken as given
    with pytest.raises(ValueError, match='vo: 4 factors given, the graph has 5'):
        PvgoInfo(vo=good[0]).packed(5, 4, UNIT, 'cpu')
    with pytest.raises(ValueError, match='rot: 4 factors given, the graph has 5'):
        PvgoInfo(rot=good[2]).packed(4, 5, UNIT, 'cpu')


def test_from_imu_cov():
    from scipy.spatial.transform import Rotation
    from islam_amd.information import PvgoInfo
    rng = np.random.default_rng(4)
    Mn = 6
    L = rng.normal(size=(Mn, 9, 9))
    cov = 1e-4 * (L @ np.swapaxes(L, 1, 2))
    q = Rotation.random(Mn, random_state=7).as_quat()
    R = Rotation.from_quat(q).as_matrix()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    for floor in (0.0, 1e-5):
        info = PvgoInfo.from_imu_cov(cov, rot=q, floor=floor)
        F = floor * np.eye(3)
        assert info.vo is None
        assert rel(info.rot, np.linalg.inv(cov[:, 0:3, 0:3] + F)) < 1e-10
        assert rel(info.vel, np.linalg.inv(R @ cov[:, 3:6, 3:6] @ np.swapaxes(R, 1, 2) + F)) < 1e-10
        assert rel(info.transvel, np.linalg.inv(R @ cov[:, 6:9, 6:9] @ np.swapaxes(R, 1, 2) + F)) < 1e-10
    ident = PvgoInfo.from_imu_cov(cov)
    assert rel(ident.vel, np.linalg.inv(cov[:, 3:6, 3:6])) < 1e-10
    import torch
    same = PvgoInfo.from_imu_cov(torch.tensor(cov), rot=torch.tensor(q))
    np.testing.assert_array_equal(same.vel, PvgoInfo.from_imu_cov(cov, rot=q).vel)
    empty = cov.copy()
    empty[4] = 0.0                                                              # a frame without samples
    with pytest.raises(ValueError, match='frame 4.*floor'):
        PvgoInfo.from_imu_cov(empty, rot=q)
    assert np.isfinite(PvgoInfo.from_imu_cov(empty, rot=q, floor=1e-6).rot).all()
    with pytest.raises(ValueError, match=r'\(M,9,9\)'):
        PvgoInfo.from_imu_cov(cov[:, :6, :6])
    with pytest.raises(ValueError, match='rot must be'):
        PvgoInfo.from_imu_cov(cov, rot=q[:3])
