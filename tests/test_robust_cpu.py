"""Robust kernels of the PVGO LM (islam_amd.robust, run_pvgo(kernel=...)) on the CPU: rho and rho' of each
kernel against their formulas and central differences, the parser of the ``kernel`` argument, and a float64 restatement of the
robust LM (oracle.pvgo.LM.step with sqrt(c)-scaled rows of R and J and sum rho as the loss) that tests/test_robust_gpu.py runs
the HIP back-end against.  With an inactive kernel the restatement follows oracle.pvgo.LM."""
import math

import numpy as np
import pytest
import torch

from oracle import lie
from oracle import pvgo as opvgo
from tests.helpers import chain_problem

LW = (1, 0.1, 10, 0.1)


# ------------------------------------------------------------------ the restatement
def factor_sq(res):
    """s_k = |r_k|^2 (unweighted) of every factor, per group: VO (E,), velocity, IMU rotation, translation-velocity (M,)."""
    return [np.sum(np.square(r), axis=1) for r in res[:4]]


def robust_loss(res, spec):
    return float(sum(np.sum(spec.rho(g, s)) for g, s in enumerate(factor_sq(res))))


def _row_weights(spec, res):
    """c_k = rho'(s_k) repeated over the factor's rows, in the order of the stacked residual [VO 6E | vel 3M | rot 3M | tv 3M]."""
    s = factor_sq(res)
    c = [np.asarray(spec.weight(g, s[g]), dtype=np.float64) for g in range(4)]
    return c, np.concatenate([np.repeat(c[0], 6), np.repeat(c[1], 3), np.repeat(c[2], 3), np.repeat(c[3], 3)])


class _BandedLinPerLink(opvgo._BandedLin):
    """oracle.pvgo._BandedLin with one weight per link and group (w4[g] of shape (M,)): the c-scaled normal equations."""

    def __init__(self, nodes, inp, res, A_e, B_k, w4):
        dts = np.asarray(inp[5]).reshape(-1)
        N = nodes.shape[0]
        M = N - 1
        dt = nodes.dtype
        self.N, self.dt, self.A_e, self.B_k, self.dts, self.J_rp = N, dt, A_e, B_k, dts, None
        w0, w1, w2, w3 = [np.asarray(x, dtype=dt) for x in w4]
        e, rv, er, rt = res[:4]
        I3 = np.eye(3, dtype=dt)
        S = w0[:, None, None] * (np.swapaxes(A_e, 1, 2) @ A_e)
        S[:, :3, :3] += w3[:, None, None] * I3
        S[:, 3:, 3:] += w2[:, None, None] * (np.swapaxes(B_k, 1, 2) @ B_k)
        Hd = np.zeros((N, 9, 9), dt)
        Ho = np.zeros((M, 9, 9), dt)
        Hd[:-1, :6, :6] += S
        Hd[1:, :6, :6] += S
        Ho[:, :6, :6] = -S
        Hd[:-1, 6:, 6:] += (w1 + w3 * dts * dts)[:, None, None] * I3
        Hd[1:, 6:, 6:] += w1[:, None, None] * I3
        Ho[:, 6:, 6:] = -w1[:, None, None] * I3
        c = (w3 * dts)[:, None, None] * I3
        Hd[:-1, 0:3, 6:9] += c
        Hd[:-1, 6:9, 0:3] += c
        Ho[:, 6:9, 0:3] += -c
        gp = w0[:, None] * (np.swapaxes(A_e, 1, 2) @ e[:, :, None])[:, :, 0]
        gp[:, 3:] += w2[:, None] * (np.swapaxes(B_k, 1, 2) @ er[:, :, None])[:, :, 0]
        gp[:, :3] += w3[:, None] * rt
        g = np.zeros((N, 9), dt)
        g[1:, :6] += gp
        g[:-1, :6] -= gp
        g[:-1, 6:] += w1[:, None] * rv - (w3 * dts)[:, None] * rt
        g[1:, 6:] -= w1[:, None] * rv
        self.b = (-g).reshape(-1)
        ab = np.zeros((18, 9 * N), dt)
        for r in range(9):
            for cc in range(9):
                if r >= cc:
                    ab[r - cc, cc::9] = Hd[:, r, cc]
                ab[9 + cc - r, r:9 * M:9] = Ho[:, r, cc]
        self.ab = ab
        self.diag = ab[0].copy()


class RobustLM(opvgo.LM):
    """oracle.pvgo.LM.step under robust kernels: rows of R and J scaled by sqrt(c_k), c_k = rho'(s_k) at the linearisation point;
    loss = sum rho(s_k).  Damping, clamp, cumulative damping, reject limit: unchanged."""

    def __init__(self, nodes, vels, spec, **kw):
        super().__init__(nodes, vels, **kw)
        self.spec = spec

    def step(self, inp, loss_weight):
        edges, poses, drots, dtrans, dvels, dts = inp
        E, M = edges.shape[0], self.nodes.shape[0] - 1
        dt = self.nodes.dtype
        res = self._res(inp)
        c, c_rows = _row_weights(self.spec, res)
        sc = np.sqrt(c_rows)
        R = np.concatenate([r.reshape(-1) for r in res]) * sc
        A_e, B_k = opvgo.jac_blocks(self.nodes, edges, poses, drots, res[0], res[2])
        if self.mode == 'dense':
            lin = opvgo._DenseLin(self.nodes, inp, res, A_e, B_k, opvgo.weight_vector(E, M, loss_weight, dt) * c_rows, self.ttj)
        else:
            lin = _BandedLinPerLink(self.nodes, inp, res, A_e, B_k, [loss_weight[g] ** 2 * c[g] for g in range(4)])
        if self.loss is None:
            self.loss = robust_loss(res, self.spec)
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
            self.loss = robust_loss(self._res(inp), self.spec)
            self.strategy.update(self.last, self.loss, lin.JD(Dn, Dv) * sc, R)
            if self.last < self.loss and self.reject_count < self.reject:
                self.nodes, self.vels = opvgo.retract(self.nodes, self.vels, -Dn, -Dv)
                self.trace.append((self.loss, pg['damping'], False))
                self.loss, self.reject_count = self.last, self.reject_count + 1
            else:
                self.trace.append((self.loss, pg['damping'], True))
                break
        self.step_losses.append(self.loss)
        return self.loss


def run_robust(prob, spec, loss_weight=LW, mode='dense', radius=1e4, max_steps=10):
    """oracle.pvgo.run_pvgo's loop with RobustLM (spec None: oracle.pvgo.LM).  Returns (aligned nodes, aligned vels, optimizer)."""
    c = lambda a: np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    nodes0, vels0 = c(prob['init_nodes']), c(prob['init_vels'])
    inp = (np.asarray(prob['links'], dtype=np.int64), c(prob['vo_motions']), c(prob['imu_drots']), c(prob['imu_dtrans']),
           c(prob['imu_dvels']), c(prob['dts']))
    if spec is None:
        opt = opvgo.LM(nodes0, vels0, radius=radius, vmin=1e-4, mode=mode)
    else:
        opt = RobustLM(nodes0, vels0, spec, radius=radius, vmin=1e-4, mode=mode)
    sched = opvgo.StopOnPlateau(opt, steps=max_steps, patience=3, decreasing=1e-3)
    while sched.continual():
        sched.step(opt.step(inp, loss_weight))
    nodes, vels = opvgo.align_to(opt.nodes, opt.vels, nodes0[0])
    return nodes, vels, opt


def corrupt(prob, edges=None, dt=1.5, dr=0.5):
    """Three VO motions (or `edges`) right-multiplied by a 1.5 m / 0.5 rad error: failed flow frames / wrong scale / false closures."""
    vo = np.asarray(prob['vo_motions'], dtype=np.float64).copy()
    E = vo.shape[0]
    if edges is None:
        edges = (E // 5, E // 2, (4 * E) // 5)
    for k, e in enumerate(edges):
        ax = np.eye(3)[k % 3]
        vo[e] = lie.se3_mul(vo[e], lie.se3_exp(np.concatenate([dt * ax, dr * np.eye(3)[(k + 1) % 3]])))
    return dict(prob, vo_motions=vo)


def pose_error(nodes, ref):
    return np.linalg.norm(lie.se3_log(lie.se3_mul(lie.se3_inv(ref), nodes)), axis=-1)


# ------------------------------------------------------------------ tests
def _fd(f, s, h):
    return (f(s + h) - f(s - h)) / (2 * h)


@pytest.mark.parametrize('delta', [0.3, 1.0, 2.5])
def test_kernels_match_their_formulas_and_derivatives(delta):
    from islam_amd.robust import Cauchy, Huber
    s = np.array([0.0, 0.01, 0.2, 0.5, 1.7, 4.0, 30.0, 1e4])
    h, c = Huber(delta), Cauchy(delta)
    d2 = delta * delta
    want_h = np.where(s <= d2, s, 2 * delta * np.sqrt(s) - d2)
    np.testing.assert_allclose(h(s), want_h, rtol=1e-15)
    np.testing.assert_allclose(h.weight(s), np.where(s <= d2, 1.0, delta / np.sqrt(np.maximum(s, d2))), rtol=1e-15)
    np.testing.assert_allclose(c(s), d2 * np.log(1 + s / d2), rtol=1e-12)      # (log1p: exact near s = 0)
    np.testing.assert_allclose(c.weight(s), 1 / (1 + s / d2), rtol=1e-15)
    # torch and scalar inputs give the same values
    np.testing.assert_allclose(h(torch.tensor(s)).numpy(), want_h, rtol=1e-15)
    np.testing.assert_allclose(c(torch.tensor(s)).numpy(), c(s), rtol=1e-15)
    assert [h(float(x)) for x in s] == pytest.approx(list(want_h), rel=1e-15)
    assert [c.weight(float(x)) for x in s] == pytest.approx(list(c.weight(s)), rel=1e-15)
    # rho' by central differences, away from Huber's kink and from 0
    for x in s[1:]:
        if abs(x - d2) < 1e-3:
            continue
        hh = 1e-6 * max(x, 1e-3)
        assert h.weight(float(x)) == pytest.approx(_fd(h, float(x), hh), rel=1e-6)
        assert c.weight(float(x)) == pytest.approx(_fd(c, float(x), hh), rel=1e-6)
    # continuity of Huber at delta^2 (value and slope)
    assert h(d2 * (1 + 1e-12)) == pytest.approx(d2, rel=1e-9) and h.weight(d2 * (1 + 1e-12)) == pytest.approx(1.0, rel=1e-9)


def test_parser_accepts_and_rejects():
    from islam_amd.robust import CAUCHY, HUBER, NONE, Cauchy, Huber, parse_kernel
    assert parse_kernel(None) is None
    assert parse_kernel([None] * 4) is None and parse_kernel((None,) * 4) is None
    sp = parse_kernel(Huber(0.5))
    assert sp.kinds == (HUBER,) * 4 and sp.deltas == (0.5,) * 4
    sp = parse_kernel([Cauchy(2.0), None, Huber(0.1), None])
    assert sp.kinds == (CAUCHY, NONE, HUBER, NONE) and sp.deltas == (2.0, 1.0, 0.1, 1.0)
    st = sp.struct()
    assert list(st.kind) == [CAUCHY, NONE, HUBER, NONE] and list(st.delta) == [2.0, 1.0, 0.1, 1.0]
    for bad in ([Huber()] * 3, [Huber()] * 5, [], 'huber', 1.0, [Huber(), None, 'x', None], {'vo': Huber()}):
        with pytest.raises(ValueError):
            parse_kernel(bad)
    for d in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            Huber(d)
        with pytest.raises(ValueError):
            Cauchy(d)


@pytest.mark.parametrize('mode', ['dense', 'banded'])
def test_inactive_huber_restatement_follows_the_oracle_lm(mode):
    """Huber(1e6) never leaves its quadratic branch: c = 1, rho(s) = s.  The restatement then takes the oracle's steps: the same
    accept / reject pattern, dampings and iterates; the losses differ only in the order the squares are summed."""
    from islam_amd.robust import Huber, parse_kernel
    prob, _ = chain_problem(33)
    prob = corrupt(prob)
    n0, v0, ref = run_robust(prob, None, mode=mode)
    n1, v1, rob = run_robust(prob, parse_kernel(Huber(1e6)), mode=mode)
    assert len(rob.trace) == len(ref.trace) >= 3
    assert [t[2] for t in rob.trace] == [t[2] for t in ref.trace]
    assert [t[1] for t in rob.trace] == [t[1] for t in ref.trace]
    np.testing.assert_allclose([t[0] for t in rob.trace], [t[0] for t in ref.trace], rtol=1e-14)
    np.testing.assert_array_equal(n1, n0)
    np.testing.assert_array_equal(v1, v0)


def test_restatement_dense_and_banded_agree_under_kernels():
    from islam_amd.robust import Cauchy, Huber, parse_kernel
    prob, _ = chain_problem(21)
    prob = corrupt(prob)
    for k in (Huber(0.05), [Cauchy(0.1), Huber(0.5), None, Cauchy(1.0)]):
        spec = parse_kernel(k)
        nd, vd, od = run_robust(prob, spec, mode='dense')
        nb, vb, ob = run_robust(prob, spec, mode='banded')
        assert [t[2] for t in od.trace] == [t[2] for t in ob.trace]
        np.testing.assert_allclose([t[0] for t in od.trace], [t[0] for t in ob.trace], rtol=1e-10)
        np.testing.assert_allclose(nd, nb, atol=1e-9)
        np.testing.assert_allclose(vd, vb, atol=1e-9)


# The outlier case of tests/test_robust_gpu.py, calibrated here: a 9-node window (the reference's own per-batch problem) under unit
# loss weights.  Measured on the restatement, largest pose error robust / least squares: Huber(0.1) 0.18, Cauchy(0.1) 0.075.  (On
# longer chains the ten LM steps of run_pvgo do not reach the robust optimum: at N = 64 the ratios are 0.41 / 0.23, at N = 257
# above 1 -- DESIGN.md section 3.10.)
OUTLIER_CASE = dict(N=9, lw=(1, 1, 1, 1), kernels=('huber', 'cauchy'), delta=0.1)
OUTLIER_RATIO = 0.25


def outlier_kernels():
    from islam_amd.robust import Cauchy, Huber
    return [{'huber': Huber, 'cauchy': Cauchy}[k](OUTLIER_CASE['delta']) for k in OUTLIER_CASE['kernels']]


def test_kernel_rejects_corrupted_vo_motions_in_the_restatement():
    """Three VO motions off by 1.5 m / 0.5 rad pull the least-squares trajectory away from the clean problem's solution; Huber and
    Cauchy keep the largest pose error under a quarter of that."""
    from islam_amd.robust import parse_kernel
    lw = OUTLIER_CASE['lw']
    prob, _ = chain_problem(OUTLIER_CASE['N'])
    target, _, _ = run_robust(prob, None, loss_weight=lw, mode='banded')
    bad = corrupt(prob)
    n_ls, _, _ = run_robust(bad, None, loss_weight=lw, mode='banded')
    worst_ls = pose_error(n_ls, target).max()
    assert worst_ls > 1.0
    for k in outlier_kernels():
        n_r, _, _ = run_robust(bad, parse_kernel(k), loss_weight=lw, mode='banded')
        assert pose_error(n_r, target).max() <= OUTLIER_RATIO * worst_ls, (k, pose_error(n_r, target).max(), worst_ls)
