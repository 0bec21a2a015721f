"""The reference's ``dense_ba`` module surface (reference dense_ba.py) on the islam_amd back-end.

  * scale_from_disp_flow (dense_ba.py:88-176): single-sample wrapper of the batched HIP reduction (TartanVO.stereo_scale);
  * SparseReprojectionLoss (dense_ba.py:276-305): holds the back-projected keypoints / flow targets that run_pvgo hands to
    the HIP LM loop as the 5th residual (islam_pvgo_run_chain_reproj); ``__call__`` evaluates the residual with LieTensor
    ops on whatever device its tensors live on (used for inspection and by the tests);
  * DenseReprojectionLoss (dense_ba.py:179-273): the per-frame mean L1 reprojection error over the masked pixels.  The
    reference cannot feed it to run_pvgo (it has no ``.N``, pvgo.py:131), so ``__call__`` is evaluation-only here as well;
    ``normal_equations`` / ``refine`` / ``information`` differentiate the same residual on the GPU (csrc/dense_reproj.hip,
    DESIGN.md section 3.23) and give run_pvgo its VO information (PvgoInfo.from_dense_reproj); ``refine(differentiable=True)``
    lets a loss on the refined pose reach the stored depth and flow (section 3.24); ``refine_joint`` and
    ``information(sigma_inv_depth=...)`` treat the stored depth as a Gaussian prior on one inverse depth per pixel and refine or
    marginalise it with the pose (csrc/dense_ba.hip, section 3.25); ``refine_joint(differentiable=True)`` lets a loss on the jointly
    refined pose, inverse depths or depth map reach the stored depth and flow (section 3.26); both take the prior's standard
    deviation per pixel as well, and ``depth_uncertainty`` returns the posterior standard deviation of every refined depth
    (section 3.27); ``propagate`` carries both into the next frame's pixel grid and fuses them with that frame's own depth map, the
    prior of the next link (csrc/depth_prop.hip, section 3.28), with ``regularize=DepthRegularizer(...)`` after occlusion removal,
    hole filling and smoothing of the propagated map (section 3.29); ``propagate(differentiable=True)`` lets a loss behind the next
    link's refinement reach this link's state, pose and measurement (section 3.31), and ``depth_uncertainty(differentiable=True)``
    lets a loss on the variance, or behind the propagation's variance input, reach the state, the pose and the flow (section 3.32);
  * pixel2point / proj / is_inside_image helpers with the reference's semantics;
  * sample_keypoints: device-side choice of ``n`` masked pixels per frame (the reference only declares
    ``--reproj-points``, arguments.py:62; no sampler ships with it).
"""
import collections

import torch

from . import lietensor as pp

DenseBAJoint = collections.namedtuple('DenseBAJoint', 'motion inv_depth S g cost l1 count sums damping accepted rejected status trace depth')
DenseBADepthUncertainty = collections.namedtuple('DenseBADepthUncertainty', 'var_inv_depth sigma_inv_depth sigma_depth status')
DenseBAPrior = collections.namedtuple('DenseBAPrior', 'depth sigma_inv_depth inv_depth var_inv_depth source flags status')


class DepthRegularizer(collections.namedtuple('DepthRegularizer', 'occl_radius occl_min fill_radius fill_min fill_inflate smooth_radius reg_gate dist_sigma',
                                              defaults=(1, 2, 1, 3, 1.0, 1, 3.0, 0.0))):
    """What ``DenseReprojectionLoss.propagate(regularize=...)`` does to the propagated map before it is fused with the next frame's
    measurement (ops.dense_ba_depth_regularize), an immutable record.  occl_radius, occl_min: a pixel with at
    least occl_min nearer, incompatible neighbours within the radius, and more of them than compatible ones, is removed (background
    seen through the holes of a magnified surface); fill_radius, fill_min, fill_inflate: a hole with at least fill_min mutually
    compatible neighbours takes their weighted mean, and fill_inflate times a neighbour's variance plus their scatter; smooth_radius:
    every value becomes the weighted mean of its compatible neighbours and keeps its variance; reg_gate: two values are compatible
    within this many standard deviations of their difference; dist_sigma (1/m per pixel, a non-negative number or a (B,) tensor): the
    expected change of the inverse depth from one pixel to the next, whose square the smoothing adds to a neighbour's variance per
    squared pixel of distance.  A radius of 0 leaves its stage out."""
    __slots__ = ()


def pixel2point(pixels, depth, intrinsics):
    """dense_ba.py:9-62: pixels (...,N,2), depth (...,N), intrinsics (...,3,3) -> camera-frame points (...,N,3)."""
    assert pixels.size(-1) == 2, "Pixels shape incorrect"
    assert depth.size(-1) == pixels.size(-2), "Depth shape does not match pixels"
    assert intrinsics.size(-1) == intrinsics.size(-2) == 3, "Intrinsics shape incorrect."
    fx, fy = intrinsics[..., 0, 0], intrinsics[..., 1, 1]
    cx, cy = intrinsics[..., 0, 2], intrinsics[..., 1, 2]
    assert not torch.any(fx == 0), "fx Cannot contain zero"
    assert not torch.any(fy == 0), "fy Cannot contain zero"
    z = depth
    return torch.stack([((pixels[..., 0] - cx) * z) / fx, ((pixels[..., 1] - cy) * z) / fy, z], dim=-1)


def is_inside_image_1D(u, width):
    return torch.logical_and(u >= 0, u <= width)


def is_inside_image(uv, width, height):
    if len(uv.shape) == 3:
        return torch.logical_and(is_inside_image_1D(uv[0, ...], width), is_inside_image_1D(uv[1, ...], height))
    return torch.logical_and(is_inside_image_1D(uv[:, 0, ...], width), is_inside_image_1D(uv[:, 1, ...], height))


def proj(x, return_mask=False):
    """dense_ba.py:71-85: normalised image coordinates; the mask keeps z > 0.1 and |x/z|, |y/z| <= 1."""
    if not return_mask:
        return x / x[..., -1]
    mask = x[..., -1:] > 0.1
    p = torch.where(mask, x / x[..., -1:], torch.zeros_like(x))
    mask = torch.where(mask, (p[..., 0:1] >= -1) & (p[..., 0:1] <= 1) & (p[..., 1:2] >= -1) & (p[..., 1:2] <= 1),
                       torch.zeros_like(mask))
    p = torch.where(mask, p, torch.zeros_like(p))
    return p, mask.squeeze()


def scale_from_disp_flow(disp, flow, motion, fx, fy, cx, cy, baseline, depth=None, mask=None, disp_th=1):
    """dense_ba.py:88-176 for ONE sample: disp (1,H,W) or (H,W), flow (2,H,W), motion SE3 (7) or se3 (6).
    Returns (s (1,), z (H,W), mask (H,W), depth_mask (H,W)); differentiable w.r.t. ``motion``."""
    from .TartanVO import stereo_scale
    dev = flow.device
    if isinstance(motion, pp.LieTensor):
        T = motion if motion.shape[-1] == 7 else motion.Exp()
    else:
        T = pp.SE3(motion) if motion.shape[-1] == 7 else pp.se3(motion).Exp()
    T = pp.SE3(T.tensor().reshape(1, 7))
    H, W = flow.shape[-2:]
    f32 = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    intr = torch.cat([f32(fx), f32(fy), f32(cx), f32(cy)]).reshape(1, 4)
    edge = None if mask is None else mask.reshape(1, H, W)
    if depth is not None:        # dense_ba.py:125-131: a depth map replaces the disparity, valid where 0 < depth <= fx*baseline
        s, z, m, dm = stereo_scale(depth.reshape(1, 1, H, W), flow.reshape(1, 2, H, W), T, intr, f32(baseline), edge, None,
                                   depth_input=True)
    else:
        s, z, m, dm = stereo_scale(disp.reshape(1, 1, H, W), flow.reshape(1, 2, H, W), T, intr, f32(baseline), edge, f32(disp_th))
    if int(m.sum()) < 500:
        print('Warning! mask contains too less points!', int(m.sum()))          # dense_ba.py:133-134
    return s.reshape(1), z[0], m[0], dm[0]


def sample_keypoints(mask, n, generator=None):
    """Choose ``n`` pixels per frame among the True entries of mask (B,H,W), uniformly without replacement (with
    replacement when a frame has fewer than n).  Returns float (B,n,2) [u, v] pixel coordinates on mask's device."""
    B, H, W = mask.shape
    flat = mask.reshape(B, -1).to(torch.float32)
    few = flat.sum(1) < n
    if bool(few.any()):
        flat = torch.where(flat.sum(1, keepdim=True) > 0, flat, torch.ones_like(flat))
    idx = torch.multinomial(flat, n, replacement=bool(few.any()), generator=generator)
    return torch.stack([(idx % W), (idx // W)], -1).to(torch.float32)


class SparseReprojectionLoss:
    def __init__(self, points2d, depth, flow, fx, fy, cx, cy, rgb2imu_pose, device='cuda:0'):
        assert len(flow.shape) == 4            # (batch, channel, height, width)
        assert len(depth.shape) == 3           # (batch, height, width)
        assert len(points2d.shape) == 3        # (batch, N, 2)
        bs, N = points2d.shape[:2]
        points2d = points2d.to(device)
        b = torch.arange(bs, device=device).view(bs, 1).expand(bs, N)
        row, col = points2d[..., 1].to(torch.int64), points2d[..., 0].to(torch.int64)        # idx = [b, y, x] (:287)
        self.K = torch.tensor([fx, 0, cx, 0, fy, cy, 0, 0, 1], dtype=torch.float32).view(3, 3).to(device)
        depth, flow = depth.to(device), flow.to(device)
        self.point3d = pixel2point(points2d, depth[b, row, col].view(bs, N), self.K)
        self.target = flow.permute(0, 2, 3, 1)[b, row, col, :].view(bs, N, 2) + points2d
        self.N = N
        self.rgb2imu_pose = rgb2imu_pose.to(device)
        self.compat_first_motion = True        # run_pvgo replicates pvgo.py:57 `motion[0] = 0.1` unless cleared

    def __call__(self, motion):
        """(bs, N, 2) = reprojerr(point3d, target, K, T^-1, reduction='none') with T = rgb2imu^-1 motion rgb2imu."""
        C = self.rgb2imu_pose
        T = C.Inv() @ motion @ C
        Tinv = T.Inv()
        dt = pp._plain(Tinv).dtype
        P = self.point3d.to(dt)
        p = pp.SE3(pp._plain(Tinv).unsqueeze(-2)).Act(P)
        K = self.K.to(dt)
        hom = p @ K.mT
        tiny = torch.finfo(dt).tiny
        den = hom[..., -1:].abs().clamp(min=tiny)
        den = torch.where(hom[..., -1:] >= 0, den, -den)
        return hom[..., :-1] / den - self.target.to(dt)


class DenseReprojectionLoss:
    def __init__(self, depth, flow, fx, fy, cx, cy, mask, rgb2imu_pose, device='cuda:0'):
        assert len(flow.shape) == 4
        assert len(depth.shape) == 3
        assert mask is None or len(mask.shape) == 3
        H, W = flow.shape[-2:]
        self.z, self.flow = depth.to(device), flow.to(device)
        self.mask = torch.ones_like(self.z, dtype=torch.bool) if mask is None else mask.to(device)
        self.rgb2imu_pose = rgb2imu_pose.to(device)
        u, v = torch.meshgrid(torch.linspace(0, W - 1, W, device=device), torch.linspace(0, H - 1, H, device=device), indexing='xy')
        self.uv = torch.stack([u, v])
        self.K4 = (float(fx), float(fy), float(cx), float(cy))

    def __call__(self, motion):
        """dense_ba.py:209-236: mean over the masked pixels of |reproj - (flow + uv)|_1 per frame -> (B,)."""
        fx, fy, cx, cy = self.K4
        C = self.rgb2imu_pose
        Tinv = (C.Inv() @ motion @ C).Inv()
        dt = pp._plain(Tinv).dtype
        u, v = self.uv[0].to(dt), self.uv[1].to(dt)
        z = self.z.to(dt)
        P = torch.stack([z * (u - cx) / fx, z * (v - cy) / fy, z], -1)                       # (B,H,W,3)
        B, H, W = z.shape
        Pt = pp.SE3(pp._plain(Tinv).view(B, 1, 7)).Act(P.view(B, H * W, 3)).view(B, H, W, 3)
        p, rmask = proj(Pt, return_mask=True)
        mask = self.mask & rmask.view(B, H, W)
        ru = fx * p[..., 0] + cx * p[..., 2] - (self.flow[:, 0].to(dt) + u)
        rv = fy * p[..., 1] + cy * p[..., 2] - (self.flow[:, 1].to(dt) + v)
        l1 = ru.abs() + rv.abs()
        return torch.stack([l1[i][mask[i]].mean() for i in range(B)])

    def _motion7(self, motion):
        """``motion`` (LieTensor or tensor, SE3 (B,7) or se3 (B,6)) as a plain (B,7) tensor, one row per stored frame pair."""
        if isinstance(motion, pp.LieTensor):
            T = motion if motion.shape[-1] == 7 else motion.Exp()
        else:
            motion = torch.as_tensor(motion)
            T = pp.SE3(motion) if motion.shape[-1] == 7 else pp.se3(motion).Exp()
        m = pp._plain(T).detach().reshape(-1, 7)
        if m.shape[0] != self.z.shape[0]:
            raise ValueError('DenseReprojectionLoss: %d motions for %d frame pairs' % (m.shape[0], self.z.shape[0]))
        return m

    def normal_equations(self, motion, kernel=None):
        """The residual of ``__call__`` differentiated: ops.dense_reproj_normal on the stored depth, flow, mask, intrinsics and
        mount.  Returns H (B,6,6), g (B,6), cost, l1, count (B) and the camera-frame sums (B,30), float64 on the device; the
        perturbation is motion Exp(xi), and l1 / count is ``__call__``'s value."""
        from . import ops
        return ops.dense_reproj_normal(self.z, self.flow, self.mask, self._motion7(motion), torch.tensor(self.K4, dtype=torch.float64),
                                       rgb2imu=self.rgb2imu_pose, kernel=kernel)

    def refine(self, motion, iters=10, kernel=None, damping=1e-4, min_count=16, trace_cap=0, differentiable=False):
        """``iters`` device-side Levenberg-Marquardt evaluations per link from ``motion`` (ops.dense_reproj_refine); the result's
        ``motion`` is the refined (B,7) and ``status`` marks the links that could not be refined.

        differentiable=True: the returned ``motion`` carries a grad_fn over the stored depth and flow (the tensors given to the
        constructor keep their graph), so a loss on the refined pose reaches the networks that made them.  The gradient is the
        implicit-function one at the optimum, not an unrolled LM: with v the loss's gradient in the right tangent of the refined pose
        and H the undamped matrix returned here, it is d(w^T g)/d(depth, flow) at w = -H^-1 v (ops.dense_reproj_ift_weights and
        ops.dense_reproj_vjp, two launches, nothing read back).  Taking H for dg/dxi is the Gauss-Newton
        approximation: exact where the residual vanishes, off by terms proportional to the residual elsewhere; it also assumes the
        refinement has converged (g = 0).  The start ``motion`` gets no gradient (the optimum does not depend on it); a link whose
        status is set, or whose H is not positive definite, gets a zero gradient."""
        from . import ops
        if differentiable:
            mount = None if self.rgb2imu_pose is None else pp._plain(self.rgb2imu_pose).detach()
            return ops.DenseReprojRefined(*ops._DenseReprojRefine.apply(
                self.z, self.flow, self.mask, self._motion7(motion), torch.tensor(self.K4, dtype=torch.float64), mount, kernel, iters,
                damping, min_count, trace_cap))
        return ops.dense_reproj_refine(self.z, self.flow, self.mask, self._motion7(motion), torch.tensor(self.K4, dtype=torch.float64),
                                       rgb2imu=self.rgb2imu_pose, kernel=kernel, iters=iters, damping=damping, min_count=min_count,
                                       trace_cap=trace_cap)

    @staticmethod
    def sigma_inv_depth_from_disparity(sigma_disp, fx, baseline):
        """The inverse-depth standard deviation of a stereo depth map whose disparity is off by ``sigma_disp`` pixels:
        depth = fx baseline / disparity, so sigma_rho = sigma_disp / (fx baseline), uniform over the image."""
        sigma_disp, fx, baseline = float(sigma_disp), float(fx), float(baseline)
        if not (sigma_disp > 0.0 and fx > 0.0 and baseline > 0.0):
            raise ValueError('sigma_inv_depth_from_disparity: sigma_disp, fx and baseline must be positive (got %r, %r, %r)' % (sigma_disp, fx, baseline))
        return sigma_disp / (fx * baseline)

    def _prior_weight(self, sigma_inv_depth, sigma_px, who):
        """(w, m): the prior weight per link and the per-pixel factor on it (None without a map).  A number or a (B,) tensor (not read
        back when it lives on the device): w = sigma_px^2 / sigma_inv_depth^2, m = None.  A (B,H,W) tensor, one standard deviation per
        pixel: w = sigma_px^2 and m = float32(1 / sigma_i^2) where sigma_i is finite and > 0, 0 elsewhere ("no prior at this pixel", not
        an error), formed with torch.where and never read back."""
        sigma_px = float(sigma_px)
        if not (sigma_px > 0.0 and sigma_px < float('inf')):
            raise ValueError('%s: sigma_px must be a finite positive number (got %r)' % (who, sigma_px))
        B = self.z.shape[0]
        if torch.is_tensor(sigma_inv_depth):
            sig = sigma_inv_depth.detach().to(torch.float64)
            if sig.dim() == 3 and tuple(sig.shape) == tuple(self.z.shape):
                ok = torch.isfinite(sig) & (sig > 0)
                m = torch.where(ok, 1.0 / torch.where(ok, sig, torch.ones_like(sig)) ** 2, torch.zeros_like(sig))
                return sigma_px ** 2, m.to(torch.float32)
            if sig.numel() != 1 and tuple(sig.shape) != (B,):
                raise ValueError('%s: sigma_inv_depth must be a positive number, a (%d,) tensor or a %s map, got shape %s' % (
                    who, B, tuple(self.z.shape), tuple(sig.shape)))
            if not sig.is_cuda and not bool(((sig > 0) & torch.isfinite(sig)).all()):
                raise ValueError('%s: sigma_inv_depth must be finite and positive (got %s)' % (who, sig.tolist()))
            return (sigma_px / sig.reshape(-1)) ** 2, None
        sig = float(sigma_inv_depth)
        if not (sig > 0.0 and sig < float('inf')):
            raise ValueError('%s: sigma_inv_depth must be a finite positive number (got %r)' % (who, sigma_inv_depth))
        return (sigma_px / sig) ** 2, None

    def refine_joint(self, motion, sigma_inv_depth, sigma_px=1.0, iters=20, kernel=None, damping=1e-4, min_count=16, trace_cap=0,
                     differentiable=False, hessian='gauss_newton'):
        """Joint two-view bundle adjustment of each link: ``iters`` device-side Levenberg-Marquardt evaluations on the pose AND one
        inverse depth per pixel, the stored depth as a Gaussian prior of standard deviation ``sigma_inv_depth`` (1/m; a positive number,
        a (B,) tensor, or a (B,H,W) map with one value per pixel, where an entry that is not finite or not positive means "no prior at
        this pixel": section 3.27; sigma_inv_depth_from_disparity gives the usual stereo value) beside flow errors of ``sigma_px`` pixels
        (ops.dense_ba_refine).  Returns DenseBAJoint: the fields of ops.DenseBARefined (motion, inv_depth, S,
        g, cost, l1, count, sums, damping, accepted, rejected, status, trace) and ``depth``: 1 / inv_depth where that is positive,
        the stored depth elsewhere.

        differentiable=False (the default): no gradient is attached.  differentiable=True: ``motion`` and ``inv_depth`` carry a grad_fn
        over the stored depth and flow (the tensors given to the constructor keep their graph), and ``depth``, formed from
        ``inv_depth`` in torch, follows by the chain rule, so a loss on the refined pose, inverse depths or depth map reaches the
        networks.  The gradient is the implicit-function one of the joint problem at the returned state, not an unrolled LM: the
        adjoint system H_full lambda = -v is solved by the forward pass's per-pixel elimination against the undamped S returned
        here, and the gradient is d(lambda^T G)/d(depth, flow) (ops.dense_ba_ift_weights and ops.dense_ba_vjp, two or three launches,
        nothing read back).  The input depth enters only through the prior, so that derivative is exact, and the
        formula assumes convergence in pose and depths.  The start ``motion`` gets no gradient (the optimum does not depend on it), nor
        does the prior weight (``sigma_inv_depth``, ``sigma_px``: out of scope); a link whose status is set, or whose matrix is not
        positive definite, gets a zero gradient.

        hessian: which matrix the adjoint system is solved with (it changes the backward pass only; the forward pass, S and the LM stay
        Gauss-Newton).  'gauss_newton' (the default): H_full is the Gauss-Newton matrix, exact where the residual vanishes and
        rho = rho0, off by terms proportional to the residuals elsewhere -- with a noisy prior the residuals at the optimum are not zero,
        and the gradient is off by 2 - 19 % on the planted scenes (section 3.26); its kernels take no per-pixel map, and
        differentiable=True with a (B,H,W) ``sigma_inv_depth`` raises NotImplementedError.  'exact' (needs differentiable=True): one half
        of the Hessian of the cost, second-order terms of the projection, the robust kernel and the pose chart included
        (ops.dense_ba_newton_weights and ops.dense_ba_newton_vjp, three launches; section 3.30); it agrees with re-refinement to 1e-6
        on those scenes and accepts a number, a (B,) tensor and a (B,H,W) map.  Any other string is a ValueError."""
        from . import ops
        if hessian not in ('gauss_newton', 'exact'):
            raise ValueError("refine_joint: hessian must be 'gauss_newton' or 'exact' (got %r)" % (hessian,))
        if hessian == 'exact' and not differentiable:
            raise ValueError("refine_joint: hessian='exact' selects the backward pass and needs differentiable=True")
        w, m = self._prior_weight(sigma_inv_depth, sigma_px, 'refine_joint')
        if differentiable and m is not None and hessian != 'exact':
            raise NotImplementedError("refine_joint: differentiable=True with the Gauss-Newton adjoint is not implemented for a per-pixel (B,H,W) "
                                      "sigma_inv_depth map; pass hessian='exact'")
        if differentiable and hessian == 'exact':
            mount = None if self.rgb2imu_pose is None else pp._plain(self.rgb2imu_pose).detach()
            out = ops.DenseBARefined(*ops._DenseBARefineNewton.apply(
                self.z, self.flow, self.mask, self._motion7(motion), torch.tensor(self.K4, dtype=torch.float64), w, m, mount, kernel, iters,
                damping, min_count, trace_cap))
        elif differentiable:
            mount = None if self.rgb2imu_pose is None else pp._plain(self.rgb2imu_pose).detach()
            out = ops.DenseBARefined(*ops._DenseBARefine.apply(
                self.z, self.flow, self.mask, self._motion7(motion), torch.tensor(self.K4, dtype=torch.float64), w, mount, kernel, iters,
                damping, min_count, trace_cap))
        else:
            out = ops.dense_ba_refine(self.z, self.flow, self.mask, self._motion7(motion), torch.tensor(self.K4, dtype=torch.float64), w,
                                      rgb2imu=self.rgb2imu_pose, kernel=kernel, iters=iters, damping=damping, min_count=min_count,
                                      trace_cap=trace_cap, **({} if m is None else {'prior_scale': m}))
        ok = out.inv_depth > 0
        depth = torch.where(ok, (1.0 / torch.where(ok, out.inv_depth, torch.ones_like(out.inv_depth))).to(self.z.dtype), self.z.detach())
        return DenseBAJoint(*out, depth)

    def depth_uncertainty(self, joint, sigma_inv_depth, sigma_px=1.0, kernel=None, marginal=True, differentiable=False):
        """The posterior uncertainty of the depths a ``refine_joint`` returned (``joint``: its result; motion, inv_depth, sums and status
        are used), in the Gauss-Newton approximation at that state (ops.dense_ba_depth_variance).
        ``sigma_inv_depth``, ``sigma_px`` and ``kernel`` must be the ones the refinement was given.  marginal=True: the pose is uncertain
        too (marginal over it); False: the pose taken as known.  Returns DenseBADepthUncertainty, (B,H,W) float64 on the device:
        var_inv_depth = sigma_px^2 v, sigma_inv_depth = its square root (a valid per-pixel prior for a next refinement), sigma_depth =
        sigma_inv_depth / inv_depth^2 (first order), all NaN where the pixel has no usable prior or the link's ``status`` (B) is set.

        differentiable=False (the default): no gradient is attached.  differentiable=True: the same launches and the same bits, and
        ``var_inv_depth`` carries a grad_fn over ``joint.inv_depth``, ``joint.motion`` and the stored flow (the tensor given to the
        constructor keeps its graph); ``sigma_inv_depth`` and ``sigma_depth`` are formed from it in torch as on the default path, so
        they carry the graph too, ``sigma_depth`` also through ``joint.inv_depth`` itself.  A loss on the uncertainty (a Gaussian
        negative log-likelihood, say) or on what ``propagate(differentiable=True)`` makes of it then reaches the refinement and the
        networks behind it (ops._DenseBADepthVariance, ops.dense_ba_depth_variance_vjp, at most four launches; DESIGN.md section
        3.32).  The gradient is the total derivative in that state: S_cam, which ``joint.sums`` holds, is taken as the function of
        the same pose, inverse depths and flow that it is, and ``joint.sums`` must be the sums at the state (``refine_joint`` returns
        them so).  Held fixed, as the forward pass found them: which pixels are valid at the state and which have a usable prior, and
        the branch of the Huber kernel.  No gradient goes to ``sigma_inv_depth`` and ``sigma_px`` (the prior weights), the intrinsics,
        the mount, the mask or the stored depth, which enters only through "has a prior".  A pixel whose variance is 1 / w_i (a prior,
        invalid at the state) or NaN gets an exactly zero gradient, the NaN that torch.sqrt's backward forms there never reaches one,
        and a link whose status is set gets zeros."""
        from . import ops
        w, m = self._prior_weight(sigma_inv_depth, sigma_px, 'depth_uncertainty')
        if differentiable:
            mount = None if self.rgb2imu_pose is None else pp._plain(self.rgb2imu_pose).detach()
            out = ops.DenseBADepthVar(*ops._DenseBADepthVariance.apply(
                self.z, self.flow, self.mask, joint.motion, torch.tensor(self.K4, dtype=torch.float64), w, joint.inv_depth, joint.sums,
                joint.status, m, mount, kernel, marginal))
            var = float(sigma_px) ** 2 * out.var
            sig = torch.sqrt(var)
            return DenseBADepthUncertainty(var, sig, sig / (joint.inv_depth * joint.inv_depth), out.status)
        out = ops.dense_ba_depth_variance(self.z, self.flow, self.mask, joint.motion, torch.tensor(self.K4, dtype=torch.float64), w,
                                          inv_depth=joint.inv_depth, sums=joint.sums, status=joint.status, prior_scale=m,
                                          rgb2imu=self.rgb2imu_pose, kernel=kernel, marginal=marginal)
        var = float(sigma_px) ** 2 * out.var
        sig = torch.sqrt(var)
        return DenseBADepthUncertainty(var, sig, sig / (joint.inv_depth * joint.inv_depth), out.status)

    def _variance_next(self, sigma, who):
        """sigma_inv_depth_next as the (B,H,W) float32 variance map of the measurement: sigma^2 where sigma is finite and > 0.  A number
        or a host-side (B,) tensor is validated here (ValueError); a device tensor is never read back, and an entry that is not finite
        or not positive becomes NaN, "no measurement at this pixel" (the rule of _prior_weight)."""
        shape, dev = tuple(self.z.shape), self.z.device
        if not torch.is_tensor(sigma):
            sigma = torch.as_tensor(float(sigma), dtype=torch.float64)
        sig = sigma.detach().to(torch.float64)
        is_map = sig.dim() == 3 and tuple(sig.shape) == shape
        if not is_map:
            if sig.numel() != 1 and tuple(sig.shape) != shape[:1]:
                raise ValueError('%s: sigma_inv_depth_next must be a positive number, a (%d,) tensor or a %s map, got shape %s' % (
                    who, shape[0], shape, tuple(sig.shape)))
            if not sig.is_cuda and not bool(((sig > 0) & torch.isfinite(sig)).all()):
                raise ValueError('%s: sigma_inv_depth_next must be finite and positive (got %s)' % (who, sig.tolist()))
            sig = sig.reshape(-1, 1, 1).expand(shape)
        sig = sig.to(dev)
        ok = torch.isfinite(sig) & (sig > 0)
        return torch.where(ok, sig * sig, torch.full_like(sig, float('nan'))).to(torch.float32).contiguous()

    @staticmethod
    def _link_sigma_squared(sigma, name):
        """A per-link standard deviation of propagate (a number or a (B,) tensor) as the variance ops takes.  A number or a host tensor
        is validated here (ValueError); a device tensor is never read back: an entry that is negative or not finite becomes NaN, which
        the kernel reports as _lib.DENSE_REPROJ_BADPRIOR on that link."""
        if torch.is_tensor(sigma):
            ps = sigma.detach().to(torch.float64)
            if not ps.is_cuda and not bool(((ps >= 0) & torch.isfinite(ps)).all()):
                raise ValueError('propagate: %s must be finite and non-negative (got %s)' % (name, ps.tolist()))
            ok = torch.isfinite(ps) & (ps >= 0)
            return torch.where(ok, ps * ps, torch.full_like(ps, float('nan')))
        ps = float(sigma)
        if not (ps >= 0.0 and ps < float('inf')):
            raise ValueError('propagate: %s must be a finite non-negative number (got %r)' % (name, sigma))
        return ps * ps

    def propagate(self, joint, uncertainty, depth_next=None, sigma_inv_depth_next=None, process_sigma=0.0, gate=3.0, regularize=None,
                  differentiable=False, regularize_grad=None):
        """The step from one link to the next: the inverse depths a ``refine_joint`` returned (``joint``) and their variances
        (``uncertainty``: the result of ``depth_uncertainty`` for it) are warped through the refined pose into the pixel grid of the
        link's second frame, the nearest surface winning where several pixels land on one, and fused there with that frame's own depth
        map (ops.dense_ba_depth_propagate).  The stored mask, intrinsics and mount are used.  depth_next
        (B,H,W) with sigma_inv_depth_next (1/m: a positive number, a (B,) tensor or a (B,H,W) map, where an entry that is not finite or
        not positive means "no measurement at this pixel"): the second frame's stereo depth and its inverse-depth standard deviation,
        both or neither (neither: pure propagation).  process_sigma (1/m, a non-negative number or (B,)): its square is added to every
        propagated variance, e.g. the discretisation noise of the nearest-pixel warp.  gate: a propagated value more than ``gate``
        standard deviations from the measurement (an occlusion, a moving object) gives way to it; 0 never gates.  Returns DenseBAPrior:
        depth (B,H,W) float32 and sigma_inv_depth (B,H,W) float64 (NaN where nothing is known), which go straight into the next
        DenseReprojectionLoss(depth=...) and refine_joint(sigma_inv_depth=...); inv_depth and var_inv_depth (float64), source (the
        pixel of the first frame that won, -1 for none), flags (1 propagated, 2 measured, 4 gated out) and status (B) int32: a link
        whose refinement or uncertainty came with a status propagates nothing and returns the measurement alone.

        regularize (a DepthRegularizer or None): the propagated map is regularised before the fusion -- the
        pure propagation, then ops.dense_ba_depth_regularize with the measurement and ``gate``: background seen through the holes of a
        magnified surface is removed, holes are filled from their neighbours, every value is smoothed over its compatible neighbours.
        flags then also carries 8 (filled) and 16 (removed), its 1 means "a propagated or filled value is present", and source is -1
        at filled and removed pixels.  None: the single call above, unchanged.

        differentiable=False (the default): every input is detached and no gradient is attached.  differentiable=True: the same
        launches and the same bits, and ``inv_depth`` and ``var_inv_depth`` carry a grad_fn over ``joint.inv_depth``,
        ``joint.motion``, ``uncertainty.var_inv_depth`` and ``depth_next`` (which keeps its graph on this path), with ``depth`` and
        ``sigma_inv_depth`` formed from them in torch, so a loss on the next link's refinement reaches this link's refinement and the
        networks behind both (ops._DenseBAPropagate, ops.dense_ba_depth_propagate_vjp, two launches).  The
        gradient is that of the piece the forward pass chose: the target pixel, the z-buffer winner and the gate decision are held
        fixed.  ``sigma_inv_depth_next``, ``process_sigma`` and ``gate`` get no gradient; a link with a status gets a zero gradient on
        its state and pose.  With ``regularize`` it raises NotImplementedError unless ``regularize_grad`` says how the non-smooth
        stencil is differentiated.

        regularize_grad=None, or 'piecewise' (with differentiable=True and a DepthRegularizer only; anything else is a ValueError): the
        pure propagation goes through ops._DenseBAPropagate and the regularisation through ops._DenseBARegularize (its backward:
        ops.dense_ba_depth_regularize_vjp, at most three launches), the same launches and the same bits as
        the ``differentiable=False`` regularised call.  The gradient is again that of the piece the forward pass chose: every
        compatibility decision, the removed and filled sets, each hole's cluster, each pixel's smoothing set and the gate decision are
        held fixed, and a pixel that stage 1 did not keep gets an exactly zero gradient.  ``dist_sigma`` and the stage parameters get
        no gradient."""
        from . import ops
        if regularize_grad is not None and regularize_grad != 'piecewise':
            raise ValueError("propagate: regularize_grad must be None or 'piecewise' (got %r)" % (regularize_grad,))
        if regularize_grad is not None and not (differentiable and regularize is not None):
            raise ValueError("propagate: regularize_grad='piecewise' needs differentiable=True and a DepthRegularizer in regularize")
        if differentiable and regularize is not None and regularize_grad is None:
            raise NotImplementedError("propagate: differentiable=True with regularize needs regularize_grad='piecewise', the gradient of the "
                                      'piece the regularisation chose (the stencil is not smooth)')
        if (depth_next is None) != (sigma_inv_depth_next is None):
            raise ValueError('propagate: depth_next and sigma_inv_depth_next come together or not at all')
        var_next = None
        if depth_next is not None:
            if tuple(depth_next.shape) != tuple(self.z.shape):
                raise ValueError('propagate: depth_next must be %s, got %s' % (tuple(self.z.shape), tuple(depth_next.shape)))
            var_next = self._variance_next(sigma_inv_depth_next, 'propagate')
            depth_next = (depth_next if differentiable else depth_next.detach()).to(self.z.device)
        process_var = self._link_sigma_squared(process_sigma, 'process_sigma')
        link = (joint.inv_depth, uncertainty.var_inv_depth, joint.motion, torch.tensor(self.K4, dtype=torch.float64))
        link_kw = dict(mask=self.mask, status=uncertainty.status, rgb2imu=self.rgb2imu_pose, process_var=process_var)
        if differentiable:
            mount = None if self.rgb2imu_pose is None else pp._plain(self.rgb2imu_pose).detach()
            if regularize is None:
                out = ops.DenseBAPropagated(*ops._DenseBAPropagate.apply(*link, self.mask, uncertainty.status, mount, process_var, depth_next,
                                                                         var_next, gate))
            else:
                if not isinstance(regularize, DepthRegularizer):
                    raise ValueError('propagate: regularize must be a DepthRegularizer or None (got %r)' % (regularize,))
                stages = regularize._asdict()
                dist_var = self._link_sigma_squared(stages.pop('dist_sigma'), 'dist_sigma')
                pure = ops.DenseBAPropagated(*ops._DenseBAPropagate.apply(*link, self.mask, uncertainty.status, mount, process_var, None, None, 0.0))
                out = ops.DenseBARegularized(*ops._DenseBARegularize.apply(pure.inv_depth, pure.var_inv_depth, pure.source, pure.status, dist_var,
                                                                           depth_next, var_next, gate, stages))
            ok = out.inv_depth > 0          # the kernel's out_depth, with its graph: the float32 of 1 / rho_f, else the bits it stored
            depth = torch.where(ok, (1.0 / torch.where(ok, out.inv_depth, torch.ones_like(out.inv_depth))).to(torch.float32), out.depth)
            return DenseBAPrior(depth, torch.sqrt(out.var_inv_depth), out.inv_depth, out.var_inv_depth, out.source, out.flags, out.status)
        if regularize is None:
            out = ops.dense_ba_depth_propagate(*link, **link_kw, depth_next=depth_next, var_next=var_next, gate=gate)
        else:
            if not isinstance(regularize, DepthRegularizer):
                raise ValueError('propagate: regularize must be a DepthRegularizer or None (got %r)' % (regularize,))
            stages = regularize._asdict()
            dist_var = self._link_sigma_squared(stages.pop('dist_sigma'), 'dist_sigma')
            pure = ops.dense_ba_depth_propagate(*link, **link_kw, depth_next=None, var_next=None, gate=0.0)
            out = ops.dense_ba_depth_regularize(pure.inv_depth, pure.var_inv_depth, source=pure.source, status=pure.status, dist_var=dist_var,
                                                depth_next=depth_next, var_next=var_next, gate=gate, **stages)
        return DenseBAPrior(out.depth, torch.sqrt(out.var_inv_depth), out.inv_depth, out.var_inv_depth, out.source, out.flags, out.status)

    def information(self, motion, sigma_px=1.0, kernel=None, sigma_inv_depth=None):
        """H / sigma_px^2 (B,6,6) float64: the information of each link's VO residual in the frame and row order of PvgoInfo.vo, for
        flow errors of ``sigma_px`` pixels per component (PvgoInfo.from_dense_reproj).  sigma_px='residual' estimates the variance per
        link from the fit itself, sigma^2 = cost / (2 count - 6); a link with 2 count <= 6 gives the zero matrix.

        sigma_inv_depth (a positive number, a (B,) tensor or a (B,H,W) map as in refine_joint; None: the depth is taken as exact, the
        path above): the stored depth is
        a Gaussian prior of that standard deviation in inverse depth, and the result is S / sigma_px^2 with S the Schur complement of
        the joint (pose, inverse depth) problem onto the pose, at the prior depths (ops.dense_ba_normal): the
        depth-marginalised information, never larger than H / sigma_px^2.  With sigma_px='residual' the prior weight is formed with
        sigma_px = 1 and the variance comes from the joint cost, again over 2 count - 6 degrees of freedom (the n depth unknowns are
        matched by their n prior rows)."""
        if sigma_inv_depth is None:
            ne = self.normal_equations(motion, kernel=kernel)
            Hm = ne.H
        else:
            from . import ops
            residual = isinstance(sigma_px, str)
            w, m = self._prior_weight(sigma_inv_depth, 1.0 if residual else sigma_px, 'information')
            ne = ops.dense_ba_normal(self.z, self.flow, self.mask, self._motion7(motion), torch.tensor(self.K4, dtype=torch.float64), w,
                                     rgb2imu=self.rgb2imu_pose, kernel=kernel, **({} if m is None else {'prior_scale': m}))
            Hm = ne.S
        if isinstance(sigma_px, str):
            if sigma_px != 'residual':
                raise ValueError("information: sigma_px must be a positive number or 'residual' (got %r)" % (sigma_px,))
            dof = 2.0 * ne.count - 6.0
            ok = dof > 0
            var = torch.where(ok, ne.cost / torch.where(ok, dof, torch.ones_like(dof)), torch.ones_like(dof))
            return torch.where(ok.view(-1, 1, 1), Hm / var.view(-1, 1, 1), torch.zeros_like(Hm))
        sigma_px = float(sigma_px)
        if not (sigma_px > 0.0 and sigma_px < float('inf')):
            raise ValueError('information: sigma_px must be a finite positive number (got %r)' % (sigma_px,))
        return Hm / sigma_px ** 2
