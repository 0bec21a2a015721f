"""Robust kernels for the PVGO Levenberg-Marquardt (``run_pvgo(kernel=...)``), named like PyPose's ``pp.optim.kernel``.

A kernel maps the UNWEIGHTED squared norm s = |r|^2 of one factor's residual to rho(s).  Under a kernel the LM loss (accept /
reject test, TrustRegion, StopOnPlateau) is sum rho(s) over the factors, and each factor's rows of J^T W J, J^T W r and of the
trust-region term are scaled by c = rho'(s) at the linearisation point -- r and J scaled by sqrt(c).

The factor groups are the four model outputs, in the order of ``loss_weight``: 0 VO (``pgerr``), 1 velocity (``adjvelerr``),
2 IMU rotation (``imuroterr``), 3 translation-velocity (``transvelerr``).
"""
import math

import numpy as np
import torch

NONE, HUBER, CAUCHY = 0, 1, 2         # ISLAM_ROBUST_NONE / _HUBER / _CAUCHY
GROUPS = ('vo', 'velocity', 'imu_rotation', 'translation_velocity')


def _floor(s, v):
    """max(s, v) elementwise (keeps the sqrt of the branch np.where / torch.where discards finite)."""
    return s.clamp(min=v) if isinstance(s, torch.Tensor) else np.maximum(s, v)


def _where(cond, a, b):
    return torch.where(cond, a, b) if isinstance(cond, torch.Tensor) else np.where(cond, a, b)


class _Kernel:
    kind = NONE

    def __init__(self, delta=1.0):
        delta = float(delta)
        if not (delta > 0.0 and math.isfinite(delta)):
            raise ValueError('%s: delta must be a finite positive number (got %r)' % (type(self).__name__, delta))
        self.delta = delta

    def __call__(self, s):
        """rho(s) on a torch tensor, a numpy array or a float."""
        return self.rho(s)

    def __repr__(self):
        return '%s(delta=%r)' % (type(self).__name__, self.delta)


class Huber(_Kernel):
    """rho(s) = s for s <= delta^2, 2 delta sqrt(s) - delta^2 above; rho'(s) = 1 or delta / sqrt(s)."""
    kind = HUBER

    def rho(self, s):
        d = self.delta
        d2 = d * d
        if np.isscalar(s):
            return s if s <= d2 else 2.0 * d * math.sqrt(s) - d2
        sqrt = torch.sqrt if isinstance(s, torch.Tensor) else np.sqrt
        return _where(s <= d2, s, 2.0 * d * sqrt(_floor(s, d2)) - d2)

    def weight(self, s):
        """c = rho'(s)."""
        d = self.delta
        d2 = d * d
        if np.isscalar(s):
            return 1.0 if s <= d2 else d / math.sqrt(s)
        sqrt = torch.sqrt if isinstance(s, torch.Tensor) else np.sqrt
        return _where(s <= d2, s * 0 + 1.0, d / sqrt(_floor(s, d2)))


class Cauchy(_Kernel):
    """rho(s) = delta^2 log(1 + s / delta^2); rho'(s) = 1 / (1 + s / delta^2)."""
    kind = CAUCHY

    def rho(self, s):
        d2 = self.delta * self.delta
        if np.isscalar(s):
            return d2 * math.log1p(s / d2)
        return d2 * (torch.log1p(s / d2) if isinstance(s, torch.Tensor) else np.log1p(s / d2))

    def weight(self, s):
        d2 = self.delta * self.delta
        return 1.0 / (1.0 + s / d2)


class RobustSpec:
    """The parsed ``kernel`` argument: one kernel (or None = trivial) per factor group."""

    def __init__(self, kernels):
        self.kernels = tuple(kernels)

    @property
    def kinds(self):
        return tuple(NONE if k is None else k.kind for k in self.kernels)

    @property
    def deltas(self):
        return tuple(1.0 if k is None else k.delta for k in self.kernels)

    def rho(self, g, s):
        k = self.kernels[g]
        return s if k is None else k.rho(s)

    def weight(self, g, s):
        k = self.kernels[g]
        if k is None:
            return 1.0 if np.isscalar(s) else s * 0 + 1.0
        return k.weight(s)

    def struct(self):
        """The library's islam_pvgo_robust."""
        from ._lib import PvgoRobust
        r = PvgoRobust()
        for g in range(4):
            r.kind[g], r.delta[g] = self.kinds[g], self.deltas[g]
        return r

    def __repr__(self):
        return 'RobustSpec(%r)' % (self.kernels,)


def parse_kernel(kernel):
    """``kernel`` of run_pvgo -> RobustSpec, or None when every group is trivial.  Accepts None, one kernel (applied to all four
    groups, as PyPose applies a single kernel to every output) or a sequence of four entries, None meaning trivial.  Raises
    ValueError otherwise."""
    if kernel is None:
        return None
    if isinstance(kernel, _Kernel):
        kernels = (kernel,) * 4
    elif isinstance(kernel, (list, tuple)):
        if len(kernel) != 4:
            raise ValueError('kernel: a sequence needs one entry per factor group %s (got %d)' % (GROUPS, len(kernel)))
        for k in kernel:
            if k is not None and not isinstance(k, _Kernel):
                raise ValueError('kernel: entries must be None, Huber or Cauchy (got %r)' % (k,))
        kernels = tuple(kernel)
    else:
        raise ValueError('kernel must be None, Huber(delta), Cauchy(delta) or a sequence of four of them / None (got %r)' % (kernel,))
    if all(k is None for k in kernels):
        return None
    return RobustSpec(kernels)
