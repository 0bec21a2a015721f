"""General-topology PVGO (arbitrary ``links``: loop closures as added or replaced edges, skipped frames) on the GPU -- SURVEY.md
section 8f rank 4; the contract on ``links`` is DESIGN.md section 3.20 (validate_graph below).

The chain fast path (islam_amd/csrc/pvgo.hip) needs links[k] = [k, k+1].  For any other edge set -- any number E >= 1 of VO edges on
the N nodes, more or fewer than the N - 1 IMU intervals, parallel and reversed edges among them -- this module runs the same LM
(pp.optim.LM + Cholesky + TrustRegion + StopOnPlateau as constructed at pvgo.py:169-172) on the normal equations PyPose factorises, but
never forms the Jacobian PyPose multiplies (rows x 10N).  There is ONE loop, _run_lm: residuals and Jacobian blocks per factor
from the HIP kernels (islam_pvgo_linearize_edges for the VO factors on arbitrary edges, islam_pvgo_linearize for the IMU factors, which
always couple consecutive nodes), cumulative damping, retraction, trial residuals and the trust-region term (J D)^T (2R + J D) from the
per-factor blocks.  It is given one of three linear systems, each with assemble(vo, lin, rpt, c_vo, c_imu) -> the clamped diagonal of
one linearisation, solve(d) -> the step (N,9) or None (failed), and ``extra`` entries for the result:
  * _DenseSystem: A = J^T W J (9N x 9N) and b = -J^T W r assembled block by block on the device (islam_pvgo_assemble_dense: O(E) work
    instead of the 2*rows*cols^2 dense product); fp64 POTRF / POTRS from rocSOLVER (the only O(N^3) piece), a second matrix per trial;
  * _DenseHipSystem: the same A and b with the project's own blocked Cholesky on v_mfma_f64_16x16x4_f64 (csrc/dense_chol.hip, DESIGN.md
    section 3.17), in place.  Both are sized by the dense matrix: (9N)^2 doubles (N = 5001: 16 GB of the 288 GB);
  * _BandPcgSystem, for long trajectories with a few loop closures (added or replaced edges): the IMU factors always couple
    consecutive nodes and a VO edge (i, j) adds S = w J^T J to the diagonal blocks of i and j and -S to the block (i, j), so
      A = B + R,  B = block-tridiagonal (all diagonal blocks, the couplings |i-j| = 1),  R = the off-band blocks of the k long edges,
    B is positive definite on its own, rank(R) <= 12 k, and conjugate gradients preconditioned with B^-1 -- the block-tridiagonal
    solver of the chain path, islam_pvgo_solve_chain, ~60 us per application at N = 5001 -- reaches the solution of the SAME normal
    equations in at most 12 k + 1 iterations.  Memory O(N + k).  B and R are assembled in place by one kernel
    (islam_pvgo_band_assemble) and A p is one launch (islam_pvgo_band_matvec); DESIGN.md section 3.20.

Robust kernels (``kernel``, an islam_amd.robust.RobustSpec): islam_pvgo_robust_weights gives the multiplier
c = rho'(s) of every VO edge and IMU-side factor and the loss sum rho(s); the scaled assembly entry points and the trust-region
term apply c per factor.  Every system uses the same multipliers and the same loss.

Per-factor information (``info``, the packed pair of islam_amd.information.PvgoInfo.packed): every system
assembles A = sum J^T Omega J and b = -sum J^T Omega r instead -- islam_pvgo_build_normal_info for the IMU groups
(islam_pvgo_build_normal_info9 when the pair carries one correlated 9x9 per link, section 3.22),
islam_pvgo_assemble_dense_info or islam_pvgo_band_assemble for the VO edges.  The loop, the loss and the trust-region term
are the unweighted ones above."""
import numpy as np
import torch

from . import ops
from ._lib import IslamHipError
from .lm_control import LMControl

_NOCLAMP = 1e300


def _linearize(nodes, vels, edges, poses, drots, dtrans, dvels, dts, dummy_poses):
    vo = ops.pvgo_linearize_edges(nodes, edges, poses)
    lin, _ = ops.pvgo_linearize(nodes, vels, dummy_poses, drots, dtrans, dvels, dts)     # IMU rows of `lin`; VO rows unused
    return vo, lin


class _Graph:
    """What _run_lm and gauss_newton_matrix both set up (float64 contiguous device tensors, N nodes): w, the four squared loss weights, and
    linearize(nodes, vels), with unit poses where islam_pvgo_linearize takes VO motions.  info: None, or the packed per-factor
    information (info_vo (21,E), info_imu (18,N-1) or info_imu9 (45,N-1)) of PvgoInfo.packed, which then replaces w in every assembly
    (ops.pvgo_build_normal_info tells the two IMU layouts apart by their row count)."""

    def __init__(self, nodes, edges, poses, drots, dtrans, dvels, dts, loss_weight, info=None):
        self.N, self.edges, self.dts, self.dev = nodes.shape[0], edges, dts, nodes.device
        self.w = [float(x) ** 2 for x in loss_weight[:4]]
        self.info = info
        if info is not None and tuple(info[0].shape) != (21, edges.shape[0]):
            raise ValueError('info_vo: (21, %d) expected, got %s' % (edges.shape[0], tuple(info[0].shape)))
        if info is not None and tuple(info[1].shape) not in ((18, self.N - 1), (45, self.N - 1)):       # three 3x3 or one 9x9 per link
            raise ValueError('info_imu: (18, %d) or (45, %d) expected, got %s' % (self.N - 1, self.N - 1, tuple(info[1].shape)))
        dummy = torch.zeros((self.N - 1, 7), dtype=torch.float64, device=self.dev)
        dummy[:, 6] = 1.0
        self.linearize = lambda nodes, vels: _linearize(nodes, vels, edges, poses, drots, dtrans, dvels, dts, dummy)

    def imu_part(self, lin, c_imu=None):
        """(Hd, Ho, rhs) of the IMU factors alone (no VO group, no clamp): the chain arrays the dense and the band assembly add the VO
        edges to, under the graph's weighting -- per-factor information, or w with the robust multipliers c_imu (3,N-1)."""
        if self.info is not None:
            return ops.pvgo_build_normal_info(lin, self.dts, self.N, None, self.info[1], -_NOCLAMP, _NOCLAMP)
        return ops.pvgo_build_normal(lin, self.dts, self.N, (0.0, self.w[1], self.w[2], self.w[3]), -_NOCLAMP, _NOCLAMP, c_imu=c_imu)

    @property
    def info_vo(self):
        return self.info[0] if self.info is not None else None


def validate_graph(N, links, n_motions, imu_rows=None):
    """The contract on a general-topology graph, checked on the host: ``links`` of shape (E, 2), E >= 1, node
    indices in [0, N), no self-loop (a factor between a node and itself has a zero Jacobian, and the node assembly would add its S
    twice to the diagonal); one VO motion per edge; imu_rows {name: rows}: N - 1 rows each (the IMU factors couple consecutive nodes).
    More or fewer edges than N - 1, parallel edges and edges (j, i) with j > i are all fine.  Raises ValueError naming the first
    offending edge; returns links as an (E, 2) int64 numpy array."""
    l = np.asarray(links.detach().cpu() if isinstance(links, torch.Tensor) else links)
    if l.ndim != 2 or l.shape[1] != 2:
        raise ValueError('links: shape (E, 2) expected, got %s' % (tuple(l.shape),))
    if l.shape[0] < 1:
        raise ValueError('links: at least one VO edge is needed (E = 0)')
    if l.dtype.kind not in 'iu':
        raise ValueError('links: integer node indices expected, got %s' % l.dtype)
    if N < 2:
        raise ValueError('a graph needs at least 2 nodes, got N = %d' % N)
    l = l.astype(np.int64)
    bad = np.nonzero(((l < 0) | (l >= N)).any(axis=1) | (l[:, 0] == l[:, 1]))[0]
    if bad.size:
        e = int(bad[0])
        i, j = int(l[e, 0]), int(l[e, 1])
        if i == j and 0 <= i < N:
            raise ValueError('links[%d] = (%d, %d) is a self-loop: a VO edge joins two different nodes' % (e, i, j))
        raise ValueError('links[%d] = (%d, %d): node index outside [0, %d)' % (e, i, j, N))
    if int(n_motions) != l.shape[0]:
        raise ValueError('one VO motion per edge: %d motions for %d edges' % (n_motions, l.shape[0]))
    for name, rows in (imu_rows or {}).items():
        if int(rows) != N - 1:
            raise ValueError('%s: %d rows, one per IMU interval expected (N - 1 = %d)' % (name, rows, N - 1))
    return l


def _validate_device_graph(nodes, edges, poses, drots, dtrans, dvels, dts):
    return validate_graph(nodes.shape[0], edges, poses.shape[0], dict(imu_drots=drots.shape[0], imu_dtrans=dtrans.shape[0],
                                                                         imu_dvels=dvels.shape[0], dts=dts.numel()))


def _loss(vo, lin):
    """Unweighted sum of squares over the model outputs (pvgo.py:64): pgerr | adjvelerr | imuroterr | transvelerr."""
    return (vo[0:6] ** 2).sum() + (lin[36:39] ** 2).sum() + (lin[24:27] ** 2).sum() + (lin[39:42] ** 2).sum()


def _node_adjacency(edges_host, N):
    """CSR of edge ends per node, entry = 2*edge + end, ascending: fixes the summation order of the diagonal blocks."""
    E = edges_host.shape[0]
    node = edges_host.reshape(-1)                          # entry index = 2*e + end
    order = np.argsort(node, kind='stable')
    ptr_ = np.zeros(N + 1, dtype=np.int64)
    np.add.at(ptr_, node + 1, 1)
    return np.cumsum(ptr_), order.astype(np.int64)


def _quality_term(vo, lin, edges, dts, D, c_vo=None, c_imu=None):
    """(J D)^T (2 R + J D) with the unweighted J, R of the linearisation point, factor by factor (each factor's term scaled by its
    robust multiplier when c_vo (E,), c_imu (3,M) are given)."""
    D6, Dv = D[:, :6], D[:, 6:]
    E = edges.shape[0]
    dp = D6[edges[:, 1]] - D6[edges[:, 0]]
    G = vo[6:15].t().reshape(E, 3, 3)
    C = vo[15:24].t().reshape(E, 3, 3)
    mv = lambda M, v: (M @ v[:, :, None])[:, :, 0]
    j0 = mv(G, dp[:, :3]) + mv(C, dp[:, 3:])
    j1 = mv(G, dp[:, 3:])
    dc = D6[1:] - D6[:-1]
    M = dc.shape[0]
    B = lin[27:36].t().reshape(M, 3, 3)
    j2 = Dv[:-1] - Dv[1:]
    j3 = mv(B, dc[:, 3:])
    j4 = dc[:, :3] - dts[:, None] * Dv[:-1]
    R0, R1 = vo[0:3].t(), vo[3:6].t()
    R2, R3, R4 = lin[36:39].t(), lin[24:27].t(), lin[39:42].t()
    if c_vo is not None:
        t = lambda j, r: (j * (2 * r + j)).sum(1)
        return (c_vo * (t(j0, R0) + t(j1, R1))).sum() + (c_imu[0] * t(j2, R2)).sum() + (c_imu[1] * t(j3, R3)).sum() + \
            (c_imu[2] * t(j4, R4)).sum()
    q = 0.0
    for j, r in ((j0, R0), (j1, R1), (j2, R2), (j3, R3), (j4, R4)):
        q = q + (j * (2 * r + j)).sum()
    return q


class _ReprojTerms:
    """The sparse reprojection factor (pvgo.py:53-61; 5th residual) of one linearisation point, in NODE coordinates.  The factor
    always couples consecutive nodes k, k+1 (motion = nodes[:-1].Inv() @ nodes[1:], whatever `links` holds), so its blocks land
    in the chain arrays (Hd, Ho, rhs) of either general-topology solver.  islam_pvgo_reproj_reduce gives, per link, J^T J / J^T r
    / r^T r in the coordinates eta of a left perturbation of T_k = C^-1 (X_k^-1 X_{k+1}) C; eta = M (delta_{k+1} - delta_k),
    M = Ad(C^-1 X_k^-1) = [[R, [t]x R], [0, R]] (reproj_link in csrc/pvgo.hip)."""

    def __init__(self, nodes, rp, dx=None):
        red = ops.pvgo_reproj_reduce(nodes, rp, dx)
        self.rr = red[:, 27].sum()                                        # unweighted r^T r over all links
        if dx is not None:
            return                                                        # trial point: only the loss is needed
        Mn, dev = red.shape[0], nodes.device
        iu = torch.triu_indices(6, 6, device=dev)
        S = torch.zeros((Mn, 6, 6), dtype=torch.float64, device=dev)
        S[:, iu[0], iu[1]] = red[:, :21]
        S = S + S.transpose(1, 2) - torch.diag_embed(S.diagonal(dim1=1, dim2=2))
        b = red[:, 21:27]
        from . import lietensor as pp
        C = pp.SE3(torch.tensor([float(v) for v in rp.rgb2imu], dtype=torch.float64, device=dev))
        Y = C.Inv() @ pp.SE3(nodes[:-1]).Inv()
        R = Y.rotation().matrix()
        T = pp._skew(Y.translation()) @ R
        Mm = torch.zeros((Mn, 6, 6), dtype=torch.float64, device=dev)
        Mm[:, :3, :3], Mm[:, :3, 3:], Mm[:, 3:, 3:] = R, T, R
        Mt = Mm.transpose(1, 2)
        self.S = Mt @ S @ Mm                                               # (M,6,6) unweighted J^T J w.r.t. (delta_{k+1} - delta_k)
        self.g = (Mt @ b[:, :, None])[:, :, 0]                             # (M,6)   unweighted J^T r
        self.w = float(rp.weight)

    def add_to_chain(self, Hd, Ho, rhs):
        """+w S on the pose blocks of nodes k and k+1, -w S on their coupling, b = -J^T W r: +w g at k, -w g at k+1."""
        wS, wg = self.w * self.S, self.w * self.g
        Hd[:-1, :6, :6] += wS
        Hd[1:, :6, :6] += wS
        Ho[:-1, :6, :6] -= wS
        rhs[:-1, :6] += wg
        rhs[1:, :6] -= wg

    def quality(self, D):
        """(J D)^T (2 R + J D) of the reprojection rows (unweighted, like the other factors)."""
        d = D[1:, :6] - D[:-1, :6]
        return (d * (2 * self.g + (self.S @ d[:, :, None])[:, :, 0])).sum()


class _DenseSystem:
    """A (9N x 9N) and b (9N) of one linearisation, factored by torch / rocSOLVER."""

    def __init__(self, g, vmin=None, vmax=None):
        self.g, self.vmin, self.vmax = g, vmin, vmax
        self.nptr, self.nadj = [torch.from_numpy(a).to(g.dev) for a in _node_adjacency(g.edges.cpu().numpy(), g.N)]
        self.A = torch.empty((9 * g.N, 9 * g.N), dtype=torch.float64, device=g.dev)
        self.b = torch.empty((9 * g.N,), dtype=torch.float64, device=g.dev)
        self.extra = {}

    def fill(self, vo, lin, rpt=None, c_vo=None, c_imu=None):
        """A (fully written) = J^T W J, undamped and unclamped, and b = -J^T W r.  rpt: _ReprojTerms; c_vo, c_imu: robust multipliers."""
        g = self.g
        Hd, Ho, rhs = g.imu_part(lin, c_imu)
        if rpt is not None:
            rpt.add_to_chain(Hd, Ho, rhs)
        ops.pvgo_assemble_dense(Hd, Ho, rhs, vo, g.edges, self.nptr, self.nadj, g.w[0], c_vo, g.info_vo, out=(self.A, self.b))      # the VO factors

    def assemble(self, vo, lin, rpt, c_vo, c_imu):
        self.fill(vo, lin, rpt, c_vo, c_imu)
        return self.A.diagonal().clamp(self.vmin, self.vmax).clone()          # A.diagonal().clamp_(min, max)

    def solve(self, d):
        """A second (9N)^2 matrix, L, lives until this returns: it is gone before the retraction."""
        self.A.diagonal().copy_(d)
        L, info = torch.linalg.cholesky_ex(self.A)
        if int(info) != 0 or not bool(torch.isfinite(L.diagonal()).all()):
            return None
        return torch.cholesky_solve(self.b[:, None], L)[:, 0].view(self.g.N, 9).contiguous()


class _DenseHipSystem(_DenseSystem):
    """The same A and b, factored in place: the upper triangle of A and the vector d in, L in A's lower triangle."""

    def __init__(self, g, vmin, vmax):
        super().__init__(g, vmin, vmax)
        self.cws = ops.dense_chol_workspace(9 * g.N, g.dev)

    def solve(self, d):
        info = ops.dense_chol_factor(self.A, d, self.cws)
        D = ops.dense_chol_solve(self.A, self.b, self.cws).view(self.g.N, 9)
        failed = torch.stack([info[0] != 0, ~torch.isfinite(D).all()]).any().item()          # one small read-back
        return None if failed else D


def gauss_newton_matrix(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj=None, info=None):
    """A = J^T W J (9N x 9N, device, fully written) at (nodes, vels): undamped, unclamped, no gauge fixed -- what run_lm_dense assembles
    before it damps the diagonal.  The VO factors may sit on any number of edges (validate_graph)."""
    _validate_device_graph(nodes, edges, poses, drots, dtrans, dvels, dts)
    if info is not None and reproj is not None:
        raise NotImplementedError('per-factor information with the reprojection factor is not implemented')
    sysm = _DenseSystem(_Graph(nodes, edges, poses, drots, dtrans, dvels, dts, loss_weight, info))
    vo, lin = sysm.g.linearize(nodes, vels)
    sysm.fill(vo, lin, _ReprojTerms(nodes, reproj) if reproj is not None else None)
    return sysm.A


def fix_gauge(A, anchor):
    """Hold the pose of node ``anchor`` fixed in the matrix the dense Cholesky reads: its six pose rows and columns become zero (in the
    strict upper triangle, which is all the factorisation reads of A) and the diagonal vector, A's own diagonal elsewhere, gets 1 in
    their places.  Returns that vector.  anchor None: nothing is fixed."""
    d = A.diagonal().clone()
    if anchor is not None:
        i = 9 * int(anchor)
        A[i:i + 6, :] = 0.0
        A[:, i:i + 6] = 0.0
        d[i:i + 6] = 1.0
    return d


def marginals_dense(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj=None, anchor=0, pairs=None, info=None):
    """Marginal covariances of a general-topology graph at (nodes, vels): Sigma = A^-1, A the undamped, unclamped Gauss-Newton matrix
    run_lm_dense assembles (with the reprojection factor when ``reproj`` is given), the pose of node ``anchor`` held fixed.  The project's
    Cholesky factors A in place, the factor is inverted in place (csrc/dense_inverse.hip) and only the
    requested 9 x 9 blocks of W^T W are formed: one (9N)^2 array in all.
    In: float64 contiguous device tensors; pairs (P,2) node index pairs or None (the graph's own edges).
    Returns (node_cov (N,9,9), pair_cov (P,9,9)); raises IslamHipError (ISLAM_ENOTPD) when the anchored matrix is not positive definite."""
    N = nodes.shape[0]
    if anchor is not None and not 0 <= int(anchor) < N:
        raise ValueError('anchor=%r is not a node of a graph of %d nodes' % (anchor, N))
    A = gauss_newton_matrix(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj, info)
    d = fix_gauge(A, anchor)
    info = ops.dense_chol_factor(A, d)
    bad = int(info.item())                                              # the one read-back
    if bad != 0:
        raise IslamHipError(-3, 'marginals_dense: non-positive pivot %d (anchored matrix not positive definite)' % bad)
    ops.dense_chol_invert_factor(A)
    return ops.pvgo_dense_cov_blocks(A, anchor, edges if pairs is None else pairs)


def _run_lm(nodes, vels, g, sysm, reproj, kernel, radius, max_steps, patience, decreasing):
    """The LM on the linear system ``sysm`` of the graph ``g``.  Returns (nodes, vels, info dict)."""
    ctl = LMControl(radius=radius, max_steps=max_steps, patience=patience, decreasing=decreasing)
    trials = 0
    while ctl.continual:
        vo, lin = g.linearize(nodes, vels)
        rpt = _ReprojTerms(nodes, reproj) if reproj is not None else None
        c_vo, c_imu, rho = ops.pvgo_robust_weights(vo, lin, kernel) if kernel is not None else (None, None, None)
        if not ctl.has_loss:
            ctl.set_initial_loss(float(rho) if kernel is not None else float(_loss(vo, lin) + (rpt.rr if rpt is not None else 0.0)))
        ctl.begin_step()
        d = sysm.assemble(vo, lin, rpt, c_vo, c_imu)
        while True:
            d = d + d * ctl.damping                                   # cumulative, like A.diagonal().add_(...)
            trials += 1
            D = sysm.solve(d)
            if D is None:
                print('Linear solver failed. Breaking optimization step...')
                ctl.solver_failed()
                break
            nt, vt = ops.pvgo_retract(nodes, vels, D, 1.0)
            vo_t, lin_t = g.linearize(nt, vt)
            st = _loss(vo_t, lin_t) if kernel is None else ops.pvgo_robust_weights(vo_t, lin_t, kernel, with_weights=False)[2]
            qt = _quality_term(vo, lin, g.edges, g.dts, D, c_vo, c_imu)
            if rpt is not None:
                st, qt = st + _ReprojTerms(nodes, reproj, D).rr, qt + rpt.quality(D)
            s, q = torch.stack([st, qt]).tolist()
            if ctl.after_trial(s, q):
                nodes, vels = nt, vt
                break
        ctl.end_step()
    return nodes, vels, dict(steps=ctl.steps, trials=trials, loss=ctl.loss, trace=ctl.trace, **sysm.extra)


def _lm_graph(nodes, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj, kernel, solver='torch', info=None):
    """The host-side checks of the two entry points, in this order and before any device work (the refused combinations, then
    validate_graph: any number E >= 1 of VO edges), then the _Graph."""
    if info is not None and (kernel is not None or reproj is not None):
        raise NotImplementedError('per-factor information with robust kernels or the reprojection factor is not implemented')
    if kernel is not None and reproj is not None:
        raise NotImplementedError('robust kernels on the reprojection factor are not implemented')
    if solver not in ('torch', 'hip'):
        raise ValueError("solver must be 'torch' or 'hip'")
    _validate_device_graph(nodes, edges, poses, drots, dtrans, dvels, dts)
    return _Graph(nodes, edges, poses, drots, dtrans, dvels, dts, loss_weight, info)


def run_lm_dense(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, radius=1e4, max_steps=10, patience=3,
                 decreasing=1e-3, vmin=1e-4, vmax=1e32, reproj=None, kernel=None, solver='torch', info=None):
    """In: float64 contiguous device tensors; reproj: ops.pvgo_reproj_struct or None; kernel: robust.RobustSpec or None; info: the
    packed per-factor information (PvgoInfo.packed) or None.
    solver: 'torch' (torch.linalg.cholesky_ex / cholesky_solve: a second (9N)^2 matrix per trial) or 'hip' (islam_dense_chol_factor /
    _solve, csrc/dense_chol.hip: the damped diagonal goes in as a vector and the factor lands in A's lower triangle, no second matrix).
    Returns (nodes, vels, info dict)."""
    g = _lm_graph(nodes, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj, kernel, solver, info)
    sysm = (_DenseHipSystem if solver == 'hip' else _DenseSystem)(g, vmin, vmax)
    return _run_lm(nodes, vels, g, sysm, reproj, kernel, radius, max_steps, patience, decreasing)


# ------------------------------------------------------------------------------------------ band + low-rank (PCG)
def off_band_edges(edges_host):
    """Indices of the edges that couple nodes more than one apart (the part of A outside the block-tridiagonal band)."""
    d = np.abs(edges_host[:, 1] - edges_host[:, 0])
    return np.nonzero(d > 1)[0]


class _BandTopology:
    """What the band form needs of a validated edge list, built once per graph: the CSR of the edge ends per node (_node_adjacency), the
    off-band edges, and the CSR of THEIR ends per node with entry = 2 * (position in the off-band list) + end."""

    def __init__(self, edges_host, N, dev):
        off = off_band_edges(edges_host)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
        self.K = int(off.size)
        self.off_idx = to(off)
        self.nptr, self.nadj = [to(a) for a in _node_adjacency(edges_host, N)]
        self.optr, self.oadj = [to(a) for a in _node_adjacency(edges_host[off], N)]


class _BandSystem:
    """A = B + R of one linearisation: B as (Hd, Ho) of the chain solver, R as the list of off-band 6x6 blocks (io, jo, So)."""

    def __init__(self, g, vo, lin, vmin, vmax, topo, rpt=None, c_vo=None, c_imu=None):
        Hd, Ho, rhs = g.imu_part(lin, c_imu)
        if rpt is not None:
            rpt.add_to_chain(Hd, Ho, rhs)
        self.io, self.jo, self.So = ops.pvgo_band_assemble(Hd, Ho, rhs, vo, g.edges, topo.nptr, topo.nadj, g.w[0], topo.off_idx, c_vo,
                                                           g.info_vo)                                      # the VO factors, in place
        self.Hd, self.Ho, self.b, self.topo = Hd, Ho, rhs, topo
        self.diag0 = Hd.diagonal(dim1=1, dim2=2).clamp(vmin, vmax).clone()                  # A.diagonal().clamp_(min, max)

    def set_diagonal(self, d):
        self.Hd.diagonal(dim1=1, dim2=2).copy_(d)

    def matvec(self, p):
        return ops.pvgo_band_matvec(self.Hd, self.Ho, p.contiguous(), self.topo.optr, self.topo.oadj, self.io, self.jo, self.So)


def band_columns(N, edges_host, anchor, pairs_host):
    """The columns of B_a^-1 that the band covariances need, as global DoF indices 9 * node + c: int64, in two
    parts, each ascending and without repeats.  Closure part (Rc entries): c = 0..5 of every node that is an end of an off-band edge.
    Extra part: c = 0..8 of the second node b of every requested pair (a, b) with |a - b| > 1, minus what the closure part holds.
    The pose indices of node ``anchor`` (None: no such node) are left out of both.  Returns (cols, Rc)."""
    eh = np.asarray(edges_host, dtype=np.int64).reshape(-1, 2)
    ph = np.zeros((0, 2), dtype=np.int64) if pairs_host is None else np.asarray(pairs_host, dtype=np.int64).reshape(-1, 2)
    for name, a in (('edges', eh), ('pairs', ph)):
        if a.size and (a.min() < 0 or a.max() >= N):
            raise ValueError('band_columns: %s hold a node index outside [0, %d)' % (name, N))
    dof = lambda nodes, k: (9 * nodes[:, None] + np.arange(k, dtype=np.int64)[None, :]).reshape(-1)
    free = lambda c: c if anchor is None else c[~((c // 9 == int(anchor)) & (c % 9 < 6))]
    closure = free(dof(np.unique(eh[off_band_edges(eh)].reshape(-1)), 6))
    far = np.unique(ph[np.abs(ph[:, 0] - ph[:, 1]) > 1, 1])
    extra = np.setdiff1d(free(dof(far, 9)), closure)
    return np.concatenate([closure, extra]).astype(np.int64), int(closure.size)


def _capacitance(band, off_ends, Y, cols, Rc, anchor):
    """G = (I + M Y_S)^-1 M (Rc x Rc, symmetrised) of the Woodbury form: M = R on the closure ends' pose DoF cols[:Rc] -- the block -So[t] at
    (io[t], jo[t]) and at (jo[t], io[t]), So[t] symmetric; an edge that ends at the anchor has no block -- and Y_S = Y[cols[:Rc], :Rc].
    Edge after edge in list order, so that parallel closures accumulate in a fixed order."""
    dev = Y.device
    where = {int(c): r for r, c in enumerate(cols[:Rc]) if c % 9 == 0}                   # first pose DoF of a node -> its position
    M = torch.zeros((Rc, Rc), dtype=torch.float64, device=dev)
    for t, (i, j) in enumerate(off_ends.tolist()):                        # (io[t], jo[t]) of the band, known on the host
        if i == anchor or j == anchor:
            continue
        pi, pj = where[9 * i], where[9 * j]
        M[pi:pi + 6, pj:pj + 6] -= band.So[t]
        M[pj:pj + 6, pi:pi + 6] -= band.So[t]
    YS = Y[torch.from_numpy(cols[:Rc]).to(dev), :Rc]
    # (solve_ex: no error check, so no synchronisation; a singular capacitance comes with a band that failed its own status)
    G = torch.linalg.solve_ex(torch.eye(Rc, dtype=torch.float64, device=dev) + M @ YS, M)[0]
    return (0.5 * (G + G.t())).contiguous()


def marginals_band(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj=None, anchor=0, pairs=None, info=None):
    """marginals_dense without any (9N)^2 array: the same Sigma = A^-1 from the band form A = B + R of
    _BandSystem (no clamp, the diagonal untouched), Sigma = B_a^-1 - Y_c G Y_c^T: the chain's selected inverse of B (ops.pvgo_marginals),
    the columns of B_a^-1 at the closure ends (band_columns, ops.pvgo_band_inverse_columns), the capacitance solve in torch, and the
    correction on the fp64 matrix cores (ops.pvgo_band_cov_blocks).  Memory O(N R), R <= 12 K + 9 (far pairs).  B_a is the open chain,
    far worse conditioned than A: the difference above loses digits with the length of the graph (section 3.21 has the figures).
    Arguments and return value as marginals_dense; raises IslamHipError (ISLAM_ENOTPD) when B_a is not positive definite or a variance
    comes out non-positive."""
    N, dev = nodes.shape[0], nodes.device
    if anchor is not None and not 0 <= int(anchor) < N:
        raise ValueError('anchor=%r is not a node of a graph of %d nodes' % (anchor, N))
    if info is not None and reproj is not None:
        raise NotImplementedError('per-factor information with the reprojection factor is not implemented')
    anchor = None if anchor is None else int(anchor)
    eh = _validate_device_graph(nodes, edges, poses, drots, dtrans, dvels, dts)
    ph = eh if pairs is None else np.asarray(pairs.detach().cpu() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64).reshape(-1, 2)
    cols, Rc = band_columns(N, eh, anchor, ph)
    g = _Graph(nodes, edges, poses, drots, dtrans, dvels, dts, loss_weight, info)
    vo, lin = g.linearize(nodes, vels)
    rpt = _ReprojTerms(nodes, reproj) if reproj is not None else None
    band = _BandSystem(g, vo, lin, -_NOCLAMP, _NOCLAMP, _BandTopology(eh, N, dev), rpt)
    status = torch.zeros((3,), dtype=torch.int32, device=dev)
    Sd, So = ops.pvgo_marginals(band.Hd, band.Ho, anchor=anchor, status=status[0:1])
    ws = ops.pvgo_band_inverse_workspace(N, cols.size, dev)
    Y = ops.pvgo_band_inverse_columns(band.Hd, band.Ho, cols, anchor, workspace=ws, status=status[1:2])
    G = _capacitance(band, eh[off_band_edges(eh)], Y, cols, Rc, anchor) if Rc else None
    node_cov, pair_cov = ops.pvgo_band_cov_blocks(Sd, So, Y, cols, Rc, G, anchor, ph, workspace=ws, status=status[2:3])
    bad = status.tolist()                                               # the one read-back
    if any(bad):
        what = 'the band B is not positive definite' if bad[0] or bad[1] else 'a variance is not positive'
        raise IslamHipError(-3, 'marginals_band: %s (anchored matrix not positive definite)' % what)
    return node_cov, pair_cov


PCG_FAIL_RTOL = 1e-8     # true relative residual above which a PCG solve counts as failed


def _pcg(sysm, ws, rtol=1e-13, check_every=6):
    """Solve (B + R) x = b with conjugate gradients preconditioned by B^-1 (the block-tridiagonal solver, enqueued without
    host round trips; the residual is looked at every `check_every` iterations).  Raises IslamHipError (ISLAM_ENOTPD) if B
    is not positive definite."""
    N, dev = sysm.b.shape[0], sysm.b.device
    Minv = lambda r: ops.pvgo_solve_chain_enqueue(sysm.Hd, sysm.Ho, r.contiguous(), ws)
    b = sysm.b
    x = Minv(b)
    ops.pvgo_solve_status(N, ws, dev)                      # B = L D L^T went through: positive definite
    k = int(sysm.io.numel())
    if k == 0:
        return x, 0, 0.0
    zero = torch.zeros((), dtype=b.dtype, device=dev)
    safe_div = lambda a, c: torch.where(c != 0, a / torch.where(c != 0, c, torch.ones_like(c)), zero)
    r = b - sysm.matvec(x)
    tol = rtol * float(b.norm())
    z = Minv(r)
    p = z.clone()
    rz = (r * z).sum()
    its = 0
    for its in range(1, 12 * k + 12):
        Hp = sysm.matvec(p)
        alpha = safe_div(rz, (p * Hp).sum())               # (0/0 once the residual is exactly zero)
        x = x + alpha * p
        r = r - alpha * Hp
        if its % check_every == 0 and float(r.norm()) <= tol:
            break
        z = Minv(r)
        rz_new = (r * z).sum()
        p = z + safe_div(rz_new, rz) * p
        rz = rz_new
    ops.pvgo_solve_status(N, ws, dev)
    # the TRUE residual of what is returned (the recurrence above can drift, and the loop may have hit its iteration cap)
    rel = float((b - sysm.matvec(x)).norm()) / max(float(b.norm()), 1e-300)
    return x, its, rel


class _BandPcgSystem:
    """A = B + R of one linearisation (_BandSystem), solved by _pcg on one chain-solver workspace."""

    def __init__(self, g, vmin, vmax):
        self.g, self.vmin, self.vmax = g, vmin, vmax
        self.topo = _BandTopology(g.edges.cpu().numpy(), g.N, g.dev)
        self.ws = ops.pvgo_workspace(g.N, g.dev)
        try:
            ops.pvgo_solve_status(g.N, self.ws, g.dev)     # initialises the fresh workspace's status / hand-off words
        except IslamHipError:
            pass
        self.extra = dict(pcg_iterations=0, pcg_worst_relative_residual=0.0, off_band_edges=self.topo.K)

    def assemble(self, vo, lin, rpt, c_vo, c_imu):
        self.band = _BandSystem(self.g, vo, lin, self.vmin, self.vmax, self.topo, rpt, c_vo, c_imu)
        return self.band.diag0

    def solve(self, d):
        self.band.set_diagonal(d)
        try:
            D, its, rel = _pcg(self.band, self.ws)
        except IslamHipError:
            return None
        self.extra['pcg_iterations'] += its
        self.extra['pcg_worst_relative_residual'] = max(self.extra['pcg_worst_relative_residual'], rel)
        # an unconverged step must not reach LM silently: treat it like a failed factorisation (PyPose's Cholesky would
        # have returned the exact solution or raised)
        if not bool(torch.isfinite(D).all()) or rel > PCG_FAIL_RTOL:
            return None
        return D.contiguous()


def run_lm_band_pcg(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, radius=1e4, max_steps=10, patience=3,
                    decreasing=1e-3, vmin=1e-4, vmax=1e32, reproj=None, kernel=None, info=None):
    """The LM of run_lm_dense on the band + low-rank form of the same normal equations.  In: float64 contiguous device
    tensors.  Returns (nodes, vels, info dict)."""
    g = _lm_graph(nodes, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj, kernel, info=info)
    return _run_lm(nodes, vels, g, _BandPcgSystem(g, vmin, vmax), reproj, kernel, radius, max_steps, patience, decreasing)
