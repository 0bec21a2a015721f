"""Per-factor information matrices of the PVGO LM (``run_pvgo(info=PvgoInfo(...))``).

The reference hands PyPose one information matrix per factor (pvgo.py:133-162 stacks (E,6,6) and (M,3,3) tensors, :178 passes them
as ``weight=``) and only ever fills them with ``loss_weight[g]**2 * I``.  A PvgoInfo carries a real matrix per factor:
A = sum_k J_k^T Omega_k J_k, b = -sum_k J_k^T Omega_k r_k.  Factor groups, in the order of ``loss_weight``:

    g  group                  rows                        Omega
    0  vo (pgerr)             6 per edge, [rho, phi]      (E,6,6)
    1  vel                    3 per link                  (M,3,3)
    2  rot (IMU rotation)     3 per link                  (M,3,3)
    3  transvel               3 per link                  (M,3,3)

Every Omega is symmetric positive SEMI-definite: Omega_k = 0 switches factor k off (the LM's diagonal clamp keeps A positive
definite).  The accept-test loss and the trust-region term stay unweighted, as they are under scalar weights.

Groups 1-3 of a link come from the same gyro and accelerometer samples.  ``imu`` (M,9,9) replaces them by ONE factor per link on the
stacked residual [rv; er; rt] (rows in the order vel | rot | transvel), cross blocks included."""
import numpy as np
import torch

_GROUPS = (('vo', 6), ('vel', 3), ('rot', 3), ('transvel', 3))
_TRIU = {k: np.triu_indices(k) for k in (3, 6, 9)}
_IMU_BLOCKS = (('vel', 0), ('rot', 3), ('transvel', 6))       # where the three groups sit in the 9x9 of ``imu``


def _as_matrices(name, x, k, n=None):
    """(n,) scalars, (n,k) diagonals or (n,k,k) matrices -> (n,k,k) float64 numpy, symmetrised."""
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        out = a[:, None, None] * np.eye(k)
    elif a.ndim == 2 and a.shape[1] == k:
        out = np.zeros((a.shape[0], k, k))
        out[:, np.arange(k), np.arange(k)] = a
    elif a.ndim == 3 and a.shape[1:] == (k, k):
        out = 0.5 * (a + np.swapaxes(a, 1, 2))
    else:
        raise ValueError('PvgoInfo.%s: expected (n,), (n,%d) or (n,%d,%d), got shape %s' % (name, k, k, k, a.shape))
    if n is not None and out.shape[0] != n:
        raise ValueError('PvgoInfo.%s: %d factors given, the graph has %d' % (name, out.shape[0], n))
    return out


def _validate(name, m):
    bad = ~np.isfinite(m).all(axis=(1, 2))
    if bad.any():
        raise ValueError('PvgoInfo.%s: factor %d has a non-finite entry' % (name, int(np.argmax(bad))))
    if m.shape[0] == 0:
        return
    ev = np.linalg.eigvalsh(m)
    bad = ev[:, 0] < -1e-12 * np.maximum(ev[:, -1], 0.0)
    bad |= ev[:, -1] < 0.0
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError('PvgoInfo.%s: factor %d is not positive semi-definite (eigenvalues %g .. %g)' % (name, i, ev[i, 0], ev[i, -1]))


def _imu_cov_args(cov, rot):
    """cov (M,9,9) as float64 numpy and the rotation matrices (M,3,3) of ``rot`` (M,4) xyzw (None: identity), checked."""
    c = cov.detach().cpu().numpy() if isinstance(cov, torch.Tensor) else np.asarray(cov)
    c = np.asarray(c, dtype=np.float64)
    if c.ndim != 3 or c.shape[1:] != (9, 9):
        raise ValueError('from_imu_cov: cov must be (M,9,9), got %s' % (c.shape,))
    Mn = c.shape[0]
    if rot is None:
        return c, np.broadcast_to(np.eye(3), (Mn, 3, 3))
    from . import lietensor as pp
    q = pp._plain(rot) if isinstance(rot, torch.Tensor) else torch.as_tensor(np.asarray(rot))
    q = q.detach().cpu().double().numpy()
    if q.shape != (Mn, 4):
        raise ValueError('from_imu_cov: rot must be (%d,4) xyzw, got %s' % (Mn, q.shape))
    x, y, z, w = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(Mn, 3, 3)
    return c, R


class PvgoInfo:
    """One information matrix per factor.  Each of ``vo`` (6x6 per edge), ``vel``, ``rot``, ``transvel`` (3x3 per link) is None
    (``loss_weight[g]**2 * I``, filled in by run_pvgo), (n,) scalars per factor, (n,k) diagonals or (n,k,k) full matrices (symmetrised
    as (O + O^T) / 2); numpy arrays or tensors.  ``imu`` (M,9,9): one correlated information matrix per link on [rv; er; rt], in place
    of ``vel``, ``rot`` and ``transvel`` (giving it together with one of them raises ValueError).  validate: check finiteness and, on
    the host, smallest eigenvalue >= -1e-12 x largest; a violation raises ValueError naming the group and the first offending factor."""

    def __init__(self, vo=None, vel=None, rot=None, transvel=None, validate=True, imu=None):
        given = dict(vo=vo, vel=vel, rot=rot, transvel=transvel)
        self.imu = None
        if imu is not None:
            both = [name for name in ('vel', 'rot', 'transvel') if given[name] is not None]
            if both:
                raise ValueError('PvgoInfo: imu (the correlated 9x9 per link) replaces vel, rot and transvel; got imu together with %s'
                                 % ', '.join(both))
            a = imu.detach().cpu().numpy() if isinstance(imu, torch.Tensor) else np.asarray(imu)
            if a.ndim != 3 or a.shape[1:] != (9, 9):
                raise ValueError('PvgoInfo.imu: expected (n,9,9), got shape %s' % (a.shape,))
            self.imu = _as_matrices('imu', a, 9)
            if validate:
                _validate('imu', self.imu)
        for name, k in _GROUPS:
            m = None if given[name] is None else _as_matrices(name, given[name], k)
            if m is not None and validate:
                _validate(name, m)
            setattr(self, name, m)

    def matrices(self, E, M, loss_weight):
        """The four groups as (E,6,6), (M,3,3) x 3 float64 numpy arrays, None filled with loss_weight[g]**2 * I.  Under ``imu`` the
        three IMU groups are the diagonal 3x3 blocks of the 9x9 (the cross blocks: ``imu_matrices``)."""
        out = []
        imu = None if self.imu is None else self.imu_matrices(M)
        for g, (name, k) in enumerate(_GROUPS):
            n = E if g == 0 else M
            m = getattr(self, name)
            if g > 0 and imu is not None:
                lo = _IMU_BLOCKS[g - 1][1]
                m = imu[:, lo:lo + 3, lo:lo + 3]
            elif m is None:
                m = np.broadcast_to(float(loss_weight[g]) ** 2 * np.eye(k), (n, k, k))
            elif m.shape[0] != n:
                raise ValueError('PvgoInfo.%s: %d factors given, the graph has %d' % (name, m.shape[0], n))
            out.append(np.ascontiguousarray(m))
        return out

    def imu_matrices(self, M):
        """``imu`` as (M,9,9), checked against the graph's link count."""
        if self.imu is None:
            raise ValueError('PvgoInfo.imu is not set')
        if self.imu.shape[0] != M:
            raise ValueError('PvgoInfo.imu: %d factors given, the graph has %d' % (self.imu.shape[0], M))
        return self.imu

    def packed(self, E, M, loss_weight=(1, 1, 1, 1), device='cuda'):
        """The device layout of the library (include/islam_hip.h, islam_pvgo_run_chain_info), float64, component-major:
        info_vo (21,E) = the upper triangle of each 6x6 in row-major order of the triangle; info_imu (18,M) = the 6-entry upper
        triangles of [vel | rot | transvel].  With ``imu``: (info_vo, info_imu9 (45,M)), the upper triangle of each 9x9 in row-major
        order of the triangle (islam_pvgo_run_chain_info9)."""
        vo, vel, rot, tv = self.matrices(E, M, loss_weight)
        r6, c6 = _TRIU[6]
        r3, c3 = _TRIU[3]
        info_vo = np.ascontiguousarray(vo[:, r6, c6].T)
        if self.imu is not None:
            r9, c9 = _TRIU[9]
            info_imu9 = np.ascontiguousarray(self.imu_matrices(M)[:, r9, c9].T)
            return (torch.from_numpy(info_vo).to(device), torch.from_numpy(info_imu9).to(device))
        info_imu = np.ascontiguousarray(np.concatenate([m[:, r3, c3].T for m in (vel, rot, tv)], 0))
        return (torch.from_numpy(info_vo).to(device), torch.from_numpy(info_imu).to(device))

    def covs(self, E, M, loss_weight):
        """run_pvgo's ``covs`` dict under information: the per-factor mean of each block's diagonal (vo_trans rows 0-2, vo_rot 3-5)."""
        vo, vel, rot, tv = self.matrices(E, M, loss_weight)
        d = lambda m, lo, hi: np.diagonal(m, axis1=1, axis2=2)[:, lo:hi].mean(axis=1)
        return {'vo_rot': d(vo, 3, 6), 'imu_rot': d(rot, 0, 3), 'vo_trans': d(vo, 0, 3), 'imu_vel': d(vel, 0, 3), 'transvel': d(tv, 0, 3)}

    @staticmethod
    def residual_cov_from_imu_cov(cov, rot=None):
        """C (M,9,9) = S T cov T^T S^T: the covariance of the stacked IMU residual [rv; er; rt] of each link that the pre-integration
        covariance ``cov`` (M,9,9; error state [dphi, dv, dp]) implies; ``rot`` as in from_imu_cov.
        from_imu_cov(correlated=True) inverts C + floor I."""
        c, R = _imu_cov_args(cov, rot)
        c = 0.5 * (c + np.swapaxes(c, 1, 2))
        ST = np.zeros((c.shape[0], 9, 9))          # rows [rv, er, rt], columns [dphi, dv, dp]
        ST[:, 0:3, 3:6] = R                        # rv = +R dv
        ST[:, 3:6, 0:3] = -np.eye(3)               # er = -dphi
        ST[:, 6:9, 6:9] = -R                       # rt = -R dp
        C = ST @ c @ np.swapaxes(ST, 1, 2)
        return 0.5 * (C + np.swapaxes(C, 1, 2))

    @classmethod
    def from_dense_reproj(cls, H, sigma_px=1.0, floor=0.0, imu=None, vel=None, rot=None, transvel=None):
        """Information of the VO factors from the dense reprojection Hessians (DenseReprojectionLoss.normal_equations /
        ops.dense_reproj_normal): vo = H / sigma_px^2 + floor I, symmetrised and validated like every other
        group.  H (E,6,6): sum c J^T J of each edge's residual under the right perturbation motion Exp(xi); the VO residual
        Log(P^-1 X_i^-1 X_j) is -xi to first order, so H / sigma_px^2 is its information as it stands, rows [rho, phi].  sigma_px:
        standard deviation of one flow component in pixels.  ``imu`` or ``vel`` / ``rot`` / ``transvel`` are passed through.

        Flow errors of neighbouring pixels are correlated, while the sum treats every pixel as an independent measurement: the matrix
        is optimistic by about the correlation area in pixels.  ``sigma_px`` is where a user accounts for that (sigma_px^2 times the
        correlation area).  An edge with H = 0 (no valid pixel) is a factor switched off."""
        h = H.detach().cpu().numpy() if isinstance(H, torch.Tensor) else np.asarray(H)
        h = np.asarray(h, dtype=np.float64)
        if h.ndim != 3 or h.shape[1:] != (6, 6):
            raise ValueError('from_dense_reproj: H must be (E,6,6), got %s' % (h.shape,))
        sigma_px, floor = float(sigma_px), float(floor)
        if not (np.isfinite(sigma_px) and sigma_px > 0.0):
            raise ValueError('from_dense_reproj: sigma_px must be a finite positive number (got %r)' % (sigma_px,))
        if not (np.isfinite(floor) and floor >= 0.0):
            raise ValueError('from_dense_reproj: floor must be a finite non-negative number (got %r)' % (floor,))
        return cls(vo=h / sigma_px ** 2 + floor * np.eye(6), vel=vel, rot=rot, transvel=transvel, validate=True, imu=imu)

    @classmethod
    def from_imu_cov(cls, cov, rot=None, floor=0.0, vo=None, correlated=False):
        """Information of the IMU factors from the pre-integration covariances (IMUModule(prop_cov=True) / ops.imu_preint_cov in
        motion mode).  With such covariances at hand call it with ``correlated=True``: that is the
        pre-integration factor, one 9x9 per link.

        cov (M,9,9): one covariance per link, error state [dphi, dv, dp].  rot (M,4): xyzw rotation of the START node of each link,
        body -> the frame of ``imu_dvels`` / ``imu_dtrans`` (None: identity).

        correlated=True returns a PvgoInfo with ``imu = (C + floor I)^-1``, C = S T cov T^T S^T the covariance of the stacked residual
        [rv; er; rt] (``residual_cov_from_imu_cov``): T = blockdiag(I, R, R) turns dv and dp into the frame of the increments, and S
        maps [dphi, dv, dp] onto the residual rows with their signs, rv = +R dv, er = -dphi, rt = -R dp to first order (the v-r and
        v-t cross blocks change sign, r-t does not).

        correlated=False (the default) keeps the three diagonal blocks only and returns three separate factors,

            rot      = (S_phiphi + floor I)^-1
            vel      = (R S_vv R^T + floor I)^-1
            transvel = (R S_pp R^T + floor I)^-1

        which weights the three residuals of a link as if they were independent although they come from the same samples.

        Why: dphi is the right perturbation of the pre-integrated rotation dR, dR_true = dR Exp(dphi), and PVGO's rotation residual
        Log(dR^-1 R_i^-1 R_j) is exactly that perturbation to first order (with a minus sign), so S_phiphi is its covariance as it
        stands.  dv and dp live in the body frame of the link's start; the velocity and translation-velocity residuals are written in
        the frame of imu_dvels / imu_dtrans, so their covariances are rotated by R.  ``vo`` is passed through.

        A covariance (block) that is not positive definite raises ValueError naming the frame and suggesting ``floor``; a frame
        without samples has S = 0 and triggers this."""
        c, R = _imu_cov_args(cov, rot)
        Mn = c.shape[0]
        if correlated:
            C = cls.residual_cov_from_imu_cov(c, rot) + float(floor) * np.eye(9)
            ev = np.linalg.eigvalsh(C) if Mn else np.zeros((0, 9))
            bad = ~np.isfinite(ev).all(axis=1) | (ev[:, 0] <= 1e-14 * np.maximum(ev[:, -1], 0.0))
            if bad.any():
                i = int(np.argmax(bad))
                raise ValueError('from_imu_cov: the 9x9 covariance of frame %d is not positive definite (smallest eigenvalue %g; a frame '
                                 'without IMU samples has zero covariance): pass floor > 0' % (i, ev[i, 0]))
            return cls(vo=vo, validate=True, imu=np.linalg.inv(C))
        I3 = float(floor) * np.eye(3)
        out = {}
        for name, lo, rotate in (('rot', 0, False), ('vel', 3, True), ('transvel', 6, True)):
            S = c[:, lo:lo + 3, lo:lo + 3]
            S = 0.5 * (S + np.swapaxes(S, 1, 2))
            if rotate:
                S = R @ S @ np.swapaxes(R, 1, 2)
            S = S + I3
            ev = np.linalg.eigvalsh(S) if Mn else np.zeros((0, 3))
            bad = ~np.isfinite(ev).all(axis=1) | (ev[:, 0] <= 1e-14 * np.maximum(ev[:, -1], 0.0))
            if bad.any():
                i = int(np.argmax(bad))
                raise ValueError('from_imu_cov: the %s covariance of frame %d is not positive definite (smallest eigenvalue %g; a frame '
                                 'without IMU samples has zero covariance): pass floor > 0' % (name, i, ev[i, 0]))
            out[name] = np.linalg.inv(S)
        return cls(vo=vo, validate=True, **out)
