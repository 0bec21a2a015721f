"""run_pvgo with the reference's call surface (reference pvgo.py:122-205) on the HIP back-end.

What runs where:
  * the LM loop (pp.optim.LM + Cholesky + TrustRegion + StopOnPlateau, pvgo.py:168-180) is ONE call into
    libislam_hip.so (islam_pvgo_run_chain): fp64, block-tridiagonal, partitioned block Cholesky;
  * vo_loss (pvgo.py:67-78) and align_to (:114-119) are HIP kernels; vo_loss is differentiable w.r.t. the VO
    motions with PyPose's gradient convention, so ``loss_bp.backward`` in train.py:280-283 works unchanged;
  * imu_loss (:95-111) is O(N) glue on the LieTensor shim (the IMU epoch carries no gradient in the
    reference release).
The information matrices of pvgo.py:125-143 are scalar multiples of the identity; they enter as four scalars (five with
the optional sparse reprojection factor ``reproj``, islam_amd/dense_ba.py).
``kernel`` (islam_amd.robust.Huber / Cauchy, one for all four factor groups or a sequence of four) puts robust kernels on the LM,
like PyPose's ``pp.optim.LM(kernel=...)``; None keeps the plain least-squares loop.
``info`` (islam_amd.information.PvgoInfo) gives every factor its own information matrix instead; None keeps
the four scalars.  ``PvgoInfo(imu=...)`` / ``PvgoInfo.from_imu_cov(..., correlated=True)`` weights the three IMU residuals of a link as
one factor with its full 9x9 information (section 3.22); nothing else about the call changes.
``marginals``: True appends the marginal covariances at the returned state (chains: section 3.9; loop-closure graphs with
general_solver='dense_hip': section 3.18); 'band' serves loop-closure graphs with every solver from the band form (section 3.21).
"""
import numpy as np
import torch

from . import lietensor as pp
from . import ops


class UnsupportedGraphError(NotImplementedError):
    pass


def _is_canonical_chain(links, n_nodes):
    l = links.detach().cpu().numpy() if isinstance(links, torch.Tensor) else np.asarray(links)
    return l.shape == (n_nodes - 1, 2) and np.array_equal(l[:, 0], np.arange(n_nodes - 1)) and \
        np.array_equal(l[:, 1], np.arange(1, n_nodes))


def _reproj_struct(reproj, loss_weight, dev):
    """The 5th residual (pvgo.py:53-61,130-143) of a SparseReprojectionLoss-like object as the library's struct (None: none)."""
    if reproj is None:
        return None
    w5 = (loss_weight[4] / reproj.N) ** 2                                                      # pvgo.py:131
    K = reproj.K.detach().cpu().double()
    return ops.pvgo_reproj_struct(reproj.point3d.detach().to(dev, torch.float64).contiguous(),
                                  reproj.target.detach().to(dev, torch.float64).contiguous(),
                                  (K[0, 0], K[1, 1], K[0, 2], K[1, 2]),
                                  pp._plain(reproj.rgb2imu_pose).detach().cpu().double().reshape(7).tolist(), w5,
                                  getattr(reproj, 'compat_first_motion', True))


_DENSE_MAX_NODES = 12000      # the dense general-topology path holds (9N)^2 doubles
_BAND_MAX_COLUMN_BYTES = 4 << 30      # the band covariances hold 9N x R doubles, the R columns of B_a^-1 (pvgo_dense.band_columns)
_GRAPH_MARGINAL_METHODS = ('dense', 'band')


def _graph_inputs(dev, *xs):
    """Every x as a contiguous float64 tensor on ``dev`` (a LieTensor as its plain tensor)."""
    return [pp._plain(torch.as_tensor(x)).detach().to(dev, torch.float64).contiguous() for x in xs]


class _Marginals:
    """node_cov (N,9,9), the gauge ``anchor``, and the pose (N,6,6) / velocity (N,3,3) blocks of node_cov as views."""

    def __init__(self, node_cov, anchor):
        self.node_cov, self.anchor = node_cov, anchor

    @property
    def pose_cov(self):
        return self.node_cov[:, :6, :6]

    @property
    def vel_cov(self):
        return self.node_cov[:, 6:, 6:]


class PvgoMarginals(_Marginals):
    """Marginal covariances of a chain's poses and velocities (float64, on the device).

    node_cov (N,9,9): Sigma_kk in the solver's per-node ordering [rho, phi, v] -- the pose part is the left perturbation
    X <- Exp([rho, phi]) X; cross (N-1,9,9): Sigma_k,k+1 (rows node k, columns node k+1); pose_cov (N,6,6) and vel_cov (N,3,3):
    the pose and velocity blocks of node_cov.  The gauge is fixed at node ``anchor`` (its pose rows / columns are zero)."""

    def __init__(self, node_cov, cross, anchor, status=None):
        super().__init__(node_cov, anchor)
        self.cross = cross
        self.status = status             # (run_pvgo: device int32 ISLAM_OK / ISLAM_ENOTPD of the stream-ordered call)


def _packed_info(info, E, M, loss_weight, dev, reproj=None, kernel=None):
    """The argument checks of ``info`` (before any device work) and its packed device form; None stays None."""
    if info is None:
        return None
    from .information import PvgoInfo
    if not isinstance(info, PvgoInfo):
        raise TypeError('info must be an islam_amd.information.PvgoInfo or None, got %s' % type(info).__name__)
    if kernel is not None:
        raise NotImplementedError('per-factor information together with a robust kernel (info with kernel) is not implemented')
    if reproj is not None:
        raise NotImplementedError('per-factor information together with the reprojection factor (info with reproj) is not implemented')
    return info.packed(E, M, loss_weight, dev)


def _marginals_at(nodes, vels, poses, drots, dtrans, dvels, dts, loss_weight, rp, anchor, seg_len=(0, 0), status=None, info=None):
    """A = J^T W J at (nodes, vels) -- undamped, unclamped, + the reprojection factor's node blocks -- and its selected inverse.
    info: the packed per-factor information (then A = sum J^T Omega J)."""
    N = nodes.shape[0]
    lin, _ = ops.pvgo_linearize(nodes, vels, poses, drots, dtrans, dvels, dts)
    w4 = [float(x) ** 2 for x in loss_weight[:4]]
    if info is not None:
        Hd, Ho, rhs = ops.pvgo_build_normal_info(lin, dts, N, info[0], info[1], vmin=-1e300, vmax=float('inf'))
    else:
        Hd, Ho, rhs = ops.pvgo_build_normal(lin, dts, N, w4, vmin=0.0, vmax=float('inf'))
    if rp is not None:
        from .pvgo_dense import _ReprojTerms
        _ReprojTerms(nodes, rp).add_to_chain(Hd, Ho, rhs)
    Sd, So = ops.pvgo_marginals(Hd, Ho, anchor=anchor, seg_len=seg_len, status=status)
    return PvgoMarginals(Sd, So, anchor, status)


def pvgo_marginals(nodes, vels, vo_motions, dts, imu_drots, imu_dtrans, imu_dvels, loss_weight=(1, 1, 1, 1), reproj=None,
                   anchor=0):
    """Marginal covariances of the poses and velocities of a canonical chain (links[k] = [k, k+1], N-1 VO motions) at the given
    state: Sigma = A^-1 with A = J^T W J the undamped Gauss-Newton matrix of run_pvgo's graph (the PyPose-compatible Jacobians,
    the reprojection factor when ``reproj`` is given), the pose DoF of node ``anchor`` held fixed (None: no gauge fix).
    (Under per-factor information: pvgo_marginals_info.)
    Returns a PvgoMarginals; raises IslamHipError (ISLAM_ENOTPD) when the anchored matrix is not positive definite."""
    return _chain_marginals(nodes, vels, vo_motions, dts, imu_drots, imu_dtrans, imu_dvels, loss_weight, reproj, anchor, None)


def pvgo_marginals_info(nodes, vels, vo_motions, dts, imu_drots, imu_dtrans, imu_dvels, info, loss_weight=(1, 1, 1, 1), anchor=0):
    """pvgo_marginals under per-factor information: A = sum J^T Omega J with ``info`` a PvgoInfo, whose None
    groups are ``loss_weight[g]**2 * I``.  With real information in every group the covariances are metric."""
    return _chain_marginals(nodes, vels, vo_motions, dts, imu_drots, imu_dtrans, imu_dvels, loss_weight, None, anchor, info)


def _chain_marginals(nodes, vels, vo_motions, dts, imu_drots, imu_dtrans, imu_dvels, loss_weight, reproj, anchor, info):
    dev = pp._plain(torch.as_tensor(nodes)).device
    if dev.type != 'cuda':
        raise RuntimeError('islam_amd.pvgo_marginals runs on the MI355X only; there is no CPU fallback')
    Nn = len(nodes)
    packed = _packed_info(info, Nn - 1, Nn - 1, loss_weight, dev, reproj)
    n64, v64, poses, drots, dtrans, dvels, dts64 = _graph_inputs(dev, nodes, vels, vo_motions, imu_drots, imu_dtrans, imu_dvels, dts)
    N = n64.shape[0]
    if poses.shape[0] != N - 1:
        raise UnsupportedGraphError('pvgo_marginals serves canonical chains: %d VO motions for %d nodes' % (poses.shape[0], N))
    return _marginals_at(n64, v64, poses, drots, dtrans, dvels, dts64.reshape(-1), loss_weight, _reproj_struct(reproj, loss_weight, dev),
                         anchor, info=packed)


class PvgoGraphMarginals(_Marginals):
    """Marginal covariances of the poses and velocities of a graph of any topology (float64, on the device).

    node_cov (N,9,9): Sigma_kk; pairs (P,2) int64 and pair_cov (P,9,9): Sigma_ab for every requested pair (a, b), rows node a, columns
    node b; pose_cov (N,6,6) and vel_cov (N,3,3): the pose and velocity blocks of node_cov.  Per-node ordering, perturbation convention
    and the meaning of ``anchor`` are those of PvgoMarginals.  method: 'dense' (section 3.18) or 'band' (section 3.21), how it was computed."""

    def __init__(self, node_cov, pairs, pair_cov, anchor, method='dense'):
        super().__init__(node_cov, anchor)
        self.pairs, self.pair_cov, self.method = pairs, pair_cov, method


def _check_band_columns(N, links_host, anchor, pairs):
    """The one size limit of method='band', checked on the host before any device work: the R columns of B_a^-1 (9N doubles each) must fit."""
    from .pvgo_dense import band_columns
    if pairs is not None:
        pairs = np.asarray(pairs.detach().cpu() if isinstance(pairs, torch.Tensor) else pairs).reshape(-1, 2)
    R = band_columns(N, links_host, anchor, links_host if pairs is None else pairs)[0].size
    if 9 * N * R * 8 > _BAND_MAX_COLUMN_BYTES:
        raise UnsupportedGraphError('band covariances hold 9N x R doubles: N = %d nodes and R = %d columns (closure ends and far pairs) '
                                    'exceed %d bytes' % (N, R, _BAND_MAX_COLUMN_BYTES))


def _graph_marginals_at(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, rp, anchor, pairs, info=None, method='dense'):
    from .pvgo_dense import marginals_band, marginals_dense
    N = nodes.shape[0]
    if method == 'dense' and N > _DENSE_MAX_NODES:
        raise UnsupportedGraphError('dense covariances are sized for N <= %d nodes, (9N)^2 doubles (got %d nodes)' % (_DENSE_MAX_NODES, N))
    if pairs is None:
        pairs = edges
    pairs = pairs.detach().cpu() if isinstance(pairs, torch.Tensor) else torch.as_tensor(np.asarray(pairs))
    pairs = pairs.to(torch.int64).reshape(-1, 2)
    fn = marginals_band if method == 'band' else marginals_dense
    node_cov, pair_cov = fn(nodes, vels, edges, poses, drots, dtrans, dvels, dts, loss_weight, reproj=rp, anchor=anchor, pairs=pairs, info=info)
    return PvgoGraphMarginals(node_cov, pairs.to(nodes.device), pair_cov, anchor, method)


def pvgo_marginals_general(nodes, vels, vo_motions, links, dts, imu_drots, imu_dtrans, imu_dvels, loss_weight=(1, 1, 1, 1), reproj=None,
                           anchor=0, pairs=None, info=None, method='dense'):
    """Marginal covariances of the poses and velocities of a graph with arbitrary ``links`` (loop closures; canonical chains too) at the
    given state: Sigma = A^-1 with A = J^T W J the undamped Gauss-Newton matrix of run_pvgo's graph, the pose DoF of node ``anchor``
    held fixed (None: no gauge fix).  method='dense': the project's Cholesky, the inverse of its factor in place and the requested blocks
    (islam_amd.pvgo_dense.marginals_dense), N <= 12000.  method='band': the chain's selected inverse of the block-tridiagonal part and a
    Woodbury correction for the off-band edges (islam_amd.pvgo_dense.marginals_band): memory O(N R) with R the
    pose DoF of the closure ends and no limit on N, but digits are lost with the length of the graph (it agrees with 'dense' to 1e-10
    at 65 nodes, 1e-6 at 200, 1e-2 at 3000, and is refused with ISLAM_ENOTPD where a variance comes out non-positive).
    pairs (P,2): the node pairs whose cross-covariance is wanted; None: ``links``.  info: a PvgoInfo (A = sum J^T Omega J; not with
    ``reproj``).
    Returns a PvgoGraphMarginals; raises IslamHipError (ISLAM_ENOTPD) when the anchored matrix is not positive definite."""
    dev = pp._plain(torch.as_tensor(nodes)).device
    if dev.type != 'cuda':
        raise RuntimeError('islam_amd.pvgo_marginals_general runs on the MI355X only; there is no CPU fallback')
    if method not in _GRAPH_MARGINAL_METHODS:
        raise ValueError("method must be 'dense' or 'band'")
    links_host = _validate_links(len(nodes), links, vo_motions, imu_drots, imu_dtrans, imu_dvels, dts)
    if method == 'band':
        _check_band_columns(len(nodes), links_host, anchor, pairs)
    packed = _packed_info(info, len(links), len(nodes) - 1, loss_weight, dev, reproj)
    n64, v64, poses, drots, dtrans, dvels, dts64 = _graph_inputs(dev, nodes, vels, vo_motions, imu_drots, imu_dtrans, imu_dvels, dts)
    edges = torch.as_tensor(links).to(dev, torch.int64).contiguous()
    return _graph_marginals_at(n64, v64, edges, poses, drots, dtrans, dvels, dts64.reshape(-1), loss_weight, _reproj_struct(reproj, loss_weight, dev),
                               anchor, pairs, info=packed, method=method)


_GENERAL_SOLVERS = ('auto', 'dense', 'dense_hip', 'band_pcg')


def _validate_links(N, links, vo_motions, imu_drots, imu_dtrans, imu_dvels, dts):
    """pvgo_dense.validate_graph on the caller's own arrays, before any of them is copied to the device."""
    from .pvgo_dense import validate_graph
    numel = lambda x: int(pp._plain(torch.as_tensor(x)).numel())
    return validate_graph(N, links, len(vo_motions), dict(imu_drots=len(imu_drots), imu_dtrans=len(imu_dtrans), imu_dvels=len(imu_dvels),
                                                          dts=numel(dts)))


def run_pvgo(init_nodes, init_vels, vo_motions, links, dts, imu_drots, imu_dtrans, imu_dvels,
             device='cuda:0', radius=1e4, loss_weight=(1, 1, 1, 1), reproj=None, target='vo', seg_len=(0, 0),
             return_info=False, general_solver='auto', marginals=False, kernel=None, info=None):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError("islam_amd.run_pvgo runs on the MI355X only (device=%r); there is no CPU fallback" % (device,))
    if not (isinstance(marginals, (bool, int)) or marginals == 'band'):
        raise ValueError("marginals must be False, True or 'band' (got %r)" % (marginals,))
    band_marginals = isinstance(marginals, str)           # 'band': covariances of a loop-closure graph from its band form (section 3.21)
    packed = _packed_info(info, len(links), len(init_nodes) - 1, loss_weight, dev, reproj, kernel)
    robust = None
    if kernel is not None:
        from .robust import parse_kernel
        robust = parse_kernel(kernel)
        if reproj is not None:
            raise NotImplementedError('run_pvgo: robust kernels on the reprojection factor (kernel with reproj) are not implemented')
        if marginals:
            raise NotImplementedError('run_pvgo: marginals under a robust kernel (kernel with marginals=True) are not implemented')
    N = len(init_nodes)
    chain = _is_canonical_chain(links, N)
    if not chain and general_solver not in _GENERAL_SOLVERS:
        raise ValueError("general_solver must be 'auto', 'dense', 'dense_hip' or 'band_pcg'")
    if marginals and not band_marginals and not chain and general_solver != 'dense_hip':
        raise UnsupportedGraphError('marginals=True serves canonical chains (links[k] = [k, k+1]) only; covariances of '
                                    "loop-closure graphs are not implemented (except with general_solver='dense_hip': the dense "
                                    'selected inverse, pvgo_marginals_general)')
    if not chain:        # any number of VO edges on the N nodes; refused before anything reaches the device
        links_host = _validate_links(N, links, vo_motions, imu_drots, imu_dtrans, imu_dvels, dts)
        if band_marginals:
            _check_band_columns(N, links_host, 0, None)
    rp = _reproj_struct(reproj, loss_weight, dev)
    out_dtype = pp._plain(init_nodes).dtype if isinstance(init_nodes, torch.Tensor) else torch.get_default_dtype()
    nodes, vels, poses, drots, dtrans, dvels, dts64 = _graph_inputs(dev, init_nodes, init_vels, vo_motions, imu_drots, imu_dtrans, imu_dvels, dts)
    edges = torch.as_tensor(links).to(dev, torch.int64).contiguous()
    nodes, vels, dts64 = nodes.clone(), vels.clone(), dts64.reshape(-1)
    target0 = nodes[0].clone()

    if chain:            # the topology train.py produces: block-tridiagonal fast path, whole LM loop in one library call
        prm = ops.pvgo_default_params(loss_weight, radius=radius, seg_len=seg_len)
        res, _ = ops.pvgo_run_chain(nodes, vels, poses, drots, dtrans, dvels, dts64, prm, reproj=rp, robust=robust, info=packed)
    else:                # loop closures / arbitrary links: dense formulation on the device (islam_amd/pvgo_dense.py)
        from .pvgo_dense import off_band_edges, run_lm_band_pcg, run_lm_dense
        k_off = len(off_band_edges(np.asarray(edges.cpu())))
        how = general_solver
        if how == 'auto':        # a long chain with a few loop closures: block-tridiagonal solver + low-rank correction (PCG)
            how = 'band_pcg' if (N > 512 and k_off <= 64) else 'dense'
        if how != 'band_pcg' and N > _DENSE_MAX_NODES:
            raise UnsupportedGraphError('dense general-topology path is sized for N <= %d nodes, (9N)^2 doubles (got %d nodes, %d off-band '
                                        'edges; general_solver="band_pcg" has no such limit)' % (_DENSE_MAX_NODES, N, k_off))
        lm_args = (nodes, vels, edges, poses, drots, dtrans, dvels, dts64, loss_weight)
        if how == 'band_pcg':
            nodes, vels, res = run_lm_band_pcg(*lm_args, radius=radius, reproj=rp, kernel=robust, info=packed)
        else:                    # 'dense_hip': the LM of 'dense' with the project's own Cholesky (csrc/dense_chol.hip)
            nodes, vels, res = run_lm_dense(*lm_args, radius=radius, reproj=rp, kernel=robust, solver='hip' if how == 'dense_hip' else 'torch',
                                            info=packed)

    if target == 'vo':
        vo = vo_motions if isinstance(vo_motions, torch.Tensor) else torch.as_tensor(vo_motions)
        vo = pp._plain(vo).to(dev)
        trans_loss, rot_loss = ops.pvgo_vo_loss(nodes, edges, vo)
    elif target == 'imu':
        n = pp.SE3(nodes.to(out_dtype))
        v = vels.to(out_dtype)
        dr = imu_drots.to(dev) if isinstance(imu_drots, pp.LieTensor) else pp.SO3(torch.as_tensor(imu_drots).to(dev))
        dv = pp._plain(torch.as_tensor(imu_dvels)).to(dev)
        adj = dv - torch.diff(v, dim=0)
        err = (dr.Inv() @ n.rotation()[:-1].Inv() @ n.rotation()[1:]).Log().tensor()
        trans_loss, rot_loss = torch.sum(adj ** 2, dim=1), torch.sum(err ** 2, dim=1)
    else:
        raise ValueError("target must be 'vo' or 'imu'")

    an, av = ops.pvgo_align(nodes, vels, target0)
    marg = None
    if marginals and not chain:     # at the aligned fp64 state, anchor 0, pairs = links (the LM's matrix is gone): the dense selected inverse
        marg = _graph_marginals_at(an, av, edges, poses, drots, dtrans, dvels, dts64, loss_weight, rp, 0, None, info=packed,      # (True, with
                                   method='band' if band_marginals else 'dense')      # general_solver='dense_hip') or the band form ('band')
    elif marginals:      # at the aligned fp64 state the caller receives; stream-ordered, its status rides on the host copy below
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        marg = _marginals_at(an, av, poses, drots, dtrans, dvels, dts64, loss_weight, rp, 0, seg_len=seg_len, status=status, info=packed)
    # ONE device -> host copy for everything the caller reads on the host: aligned poses, velocities and the two loss vectors (their
    # host values ride along as ``.host`` on the returned loss tensors, so that a caller that only wants to report the loss does not
    # pay another synchronising read: BilevelLoop.step)
    E = trans_loss.shape[0]
    parts = [an.reshape(-1), av.reshape(-1), trans_loss.detach().to(torch.float64).reshape(-1),
             rot_loss.detach().to(torch.float64).reshape(-1)]
    chain_status = marg is not None and chain
    if chain_status:
        parts.append(marg.status.to(torch.float64))
    host = torch.cat(parts).cpu()
    if chain_status and host[-1].item() != 0:
        from ._lib import IslamHipError
        raise IslamHipError(int(host[-1].item()), 'run_pvgo(marginals=True): the Gauss-Newton matrix at the solution is not '
                                                  'positive definite')
    nodes_out = pp.SE3(host[:7 * N].view(N, 7).to(out_dtype))
    vels_out = host[7 * N:10 * N].view(N, 3).to(out_dtype)
    trans_loss.host, rot_loss.host = host[10 * N:10 * N + E], host[10 * N + E:10 * N + 2 * E]
    n1 = N - 1
    covs = {'vo_rot': np.ones(len(links)) * loss_weight[0] ** 2, 'imu_rot': np.ones(n1) * loss_weight[2] ** 2,
            'vo_trans': np.ones(len(links)) * loss_weight[0] ** 2, 'imu_vel': np.ones(n1) * loss_weight[1] ** 2,
            'transvel': np.ones(n1) * loss_weight[3] ** 2}
    if info is not None:             # the keys stay; each entry is the per-factor mean of its block's diagonal
        covs = info.covs(len(links), n1, loss_weight)
    if reproj is not None:
        covs['reproj'] = np.ones(n1) * (loss_weight[4] / reproj.N) ** 2                        # pvgo.py:202-203
    out = (trans_loss, rot_loss, nodes_out, vels_out, covs) + ((res,) if return_info else ()) + ((marg,) if marginals else ())
    return out
