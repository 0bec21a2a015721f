"""Thin tensor-level wrappers over the C ABI (one function per entry point of include/islam_hip.h).

PyTorch is used for device memory and the current HIP stream only.  All functions raise when given
CPU tensors: the product path has no CPU fallback.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import c_double, c_float, c_int, c_int64, c_size_t, c_void_p, check, lib, ptr, require_cuda, stream_ptr


def _f32c(t):
    return t.contiguous().float() if (t.dtype != torch.float32 or not t.is_contiguous()) else t


# --------------------------------------------------------------------------- correlation / warp
def corr81_forward(first, second):
    """Network/PWC/correlation.py:281-331.  (B,C,H,W) x2 float32 -> (B,81,H,W)."""
    require_cuda(first, second)
    assert first.is_contiguous() and second.is_contiguous(), 'inputs must be contiguous NCHW (correlation.py:287-288)'
    assert first.dtype == torch.float32 and second.dtype == torch.float32 and first.shape == second.shape
    B, C, H, W = first.shape
    out = torch.empty((B, 81, H, W), dtype=torch.float32, device=first.device)
    nbytes = lib().islam_corr81_scratch_bytes(B, C, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=first.device) if nbytes else None
    check(lib().islam_corr81_fwd(ptr(first), ptr(second), ptr(out), B, C, H, W, ptr(scratch), stream_ptr(first.device)))
    return out


def corr81_act(first, second, out, coff, slope=0.1):
    """LeakyReLU_slope(corr81(first, second)) written into channels [coff, coff + 81) of ``out`` (B, Ctot, H, W) fp32 -- the head of
    PWC-Net's DenseNet concatenation without the activation and copy passes (islam_corr81_fwd_act).  Inference only."""
    require_cuda(first, second, out)
    assert first.is_contiguous() and second.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32
    assert first.dtype == torch.float32 and second.dtype == torch.float32 and first.shape == second.shape
    B, C, H, W = first.shape
    assert out.shape[0] == B and tuple(out.shape[2:]) == (H, W)
    nbytes = lib().islam_corr81_scratch_bytes(B, C, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=first.device) if nbytes else None
    check(lib().islam_corr81_fwd_act(ptr(first), ptr(second), ptr(out), int(out.shape[1]), int(coff), float(slope), B, C, H, W, ptr(scratch),
                                     stream_ptr(first.device)))
    return out


def corr81_backward(first, second, grad_out, need_first=True, need_second=True):
    """Network/PWC/correlation.py:334-383."""
    require_cuda(first, second, grad_out)
    assert grad_out.is_contiguous(), 'gradOutput must be contiguous (correlation.py:337)'
    B, C, H, W = first.shape
    g1 = torch.empty_like(first) if need_first else None
    g2 = torch.empty_like(second) if need_second else None
    check(lib().islam_corr81_bwd(ptr(first), ptr(second), ptr(grad_out), ptr(g1), ptr(g2), B, C, H, W,
                                 stream_ptr(first.device)))
    return g1, g2


class _Correlation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, first, second):
        ctx.save_for_backward(first, second)
        return corr81_forward(first, second)

    @staticmethod
    def backward(ctx, grad_out):
        first, second = ctx.saved_tensors
        return corr81_backward(first, second, grad_out.contiguous(), ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def FunctionCorrelation(tenFirst, tenSecond):
    """Drop-in for Network.PWC.correlation.FunctionCorrelation (correlation.py:386-388)."""
    return _Correlation.apply(tenFirst, tenSecond)


class _WarpMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow, scale):
        ctx.save_for_backward(x, flow)
        ctx.scale = float(scale)
        return warp_mask(x, flow, scale)

    @staticmethod
    def backward(ctx, g):
        x, flow = ctx.saved_tensors
        x, flow, g = _f32c(x), _f32c(flow), _f32c(g)
        B, C, H, W = x.shape
        gx, gflow = torch.zeros_like(x), torch.zeros_like(flow)
        check(lib().islam_warp_mask_bwd(ptr(x), ptr(flow), c_float(ctx.scale), ptr(g), ptr(gx), ptr(gflow), B, C, H, W,
                                        stream_ptr(x.device)))
        return gx, gflow, None


def warp(x, flow, scale=1.0):
    """Differentiable PWCDCNet.warp(x, flow*scale) (Network/PWC/PWCNet.py:170-206)."""
    return _WarpMask.apply(x, flow, scale)


def warp_mask(x, flow, scale=1.0):
    """PWCDCNet.warp(x, flow*scale) (Network/PWC/PWCNet.py:170-206), forward value only."""
    require_cuda(x, flow)
    x, flow = _f32c(x), _f32c(flow)
    B, C, H, W = x.shape
    assert flow.shape == (B, 2, H, W)
    out = torch.empty_like(x)
    check(lib().islam_warp_mask(ptr(x), ptr(flow), c_float(scale), ptr(out), B, C, H, W, stream_ptr(x.device)))
    return out


# --------------------------------------------------------------------------- edge mask
def edge_mask(img0, downscale=True, low=50, high=100):
    """TartanVO.py:145-155 (uint8 conversion, 1/4 resize, Canny(50, 100), 5x5 dilate) in one launch.
    (B,3,H,W) float32 in [0,1] -> (B,H/4,W/4) bool."""
    require_cuda(img0)
    assert img0.dim() == 4 and img0.shape[1] == 3, 'expects (B,3,H,W) images'
    img0 = _f32c(img0)
    B, _, H, W = img0.shape
    h, w = (H // 4, W // 4) if downscale else (H, W)
    out = torch.empty((B, h, w), dtype=torch.bool, device=img0.device)
    check(lib().islam_edge_mask(ptr(img0), ptr(out), B, H, W, int(bool(downscale)), int(low), int(high), stream_ptr(img0.device)))
    return out


# --------------------------------------------------------------------------- scale recovery
def scale_ls(disp, flow, pose7, intr4, baseline, edge, disp_th, depth_input=False):
    """Batched dense_ba.scale_from_disp_flow (dense_ba.py:88-176).  Returns scale (B), z (B,H,W),
    mask, depth_mask (B,H,W) bool, sums (B,18) float64.  depth_input: ``disp`` holds a depth map (the ``depth=`` branch,
    dense_ba.py:125-131; disp_th unused)."""
    require_cuda(disp, flow, pose7)
    dev = disp.device
    disp, flow = _f32c(disp), _f32c(flow)
    B, _, H, W = flow.shape
    pose7 = _f32c(pose7.detach())
    intr4 = _f32c(intr4.to(dev))
    baseline = _f32c(baseline.to(dev))
    disp_th = None if depth_input else _f32c(disp_th.to(dev))
    if edge is not None:
        edge = edge.to(dev).to(torch.uint8).contiguous()
    scale = torch.empty(B, dtype=torch.float32, device=dev)
    z = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    dmask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    sums = torch.empty((B, _lib.SCALE_NSUM), dtype=torch.float64, device=dev)
    partial = torch.empty((B, _lib.SCALE_NBLK, _lib.SCALE_NSUM), dtype=torch.float64, device=dev)
    if depth_input:
        check(lib().islam_scale_ls_depth(ptr(disp), ptr(flow), ptr(pose7), ptr(intr4), ptr(baseline), ptr(edge), ptr(scale),
                                         ptr(z), ptr(mask), ptr(dmask), ptr(sums), ptr(partial), B, H, W, stream_ptr(dev)))
    else:
        check(lib().islam_scale_ls(ptr(disp), ptr(flow), ptr(pose7), ptr(intr4), ptr(baseline), ptr(edge), ptr(disp_th),
                                   ptr(scale), ptr(z), ptr(mask), ptr(dmask), ptr(sums), ptr(partial), B, H, W,
                                   stream_ptr(dev)))
    return scale, z, mask.bool(), dmask.bool(), sums


# --------------------------------------------------------------------------- dense reprojection
DenseReprojNormal = collections.namedtuple('DenseReprojNormal', 'H g cost l1 count sums')
DenseReprojRefined = collections.namedtuple('DenseReprojRefined', 'motion H g cost l1 count sums damping accepted rejected status trace')


class _DenseArgs(collections.namedtuple('_DenseArgs', 'dev B H W depth flow mask motion intr rgb2imu kind delta')):
    """What _dense_reproj_args prepared: the device tensors and scalars every entry point of the family takes."""

    def head(self):
        """The six pointers every entry point starts with."""
        return ptr(self.depth), ptr(self.flow), ptr(self.mask), ptr(self.motion), ptr(self.rgb2imu), ptr(self.intr)


def _dense_link_args(who, dev, B, H, W, mask, motion, intr, rgb2imu):
    """What every entry point of the family takes per link, checked and on the device: mask (B,H,W) uint8 or None, motion (B,7) and intr
    (B,4) float64, rgb2imu (7) float64 or None."""
    from . import lietensor as pp
    if mask is not None:
        if tuple(mask.shape) != (B, H, W):
            raise ValueError('%s: mask must be (%d,%d,%d), got %s' % (who, B, H, W, tuple(mask.shape)))
        mask = (mask.to(dev) != 0).to(torch.uint8).contiguous()
    f64 = lambda t: pp._plain(torch.as_tensor(t)).detach().to(dev, torch.float64).contiguous()
    motion = f64(motion)
    if tuple(motion.shape) != (B, 7):
        raise ValueError('%s: motion must be (%d,7) [t, q xyzw], got %s' % (who, B, tuple(motion.shape)))
    intr = f64(intr)
    if intr.numel() == 4:
        intr = intr.reshape(1, 4).expand(B, 4).contiguous()
    if tuple(intr.shape) != (B, 4):
        raise ValueError('%s: intr must be (4) or (%d,4) = fx, fy, cx, cy, got %s' % (who, B, tuple(intr.shape)))
    if rgb2imu is not None:
        rgb2imu = f64(rgb2imu).reshape(-1)
        if rgb2imu.numel() != 7:
            raise ValueError('%s: rgb2imu must be one SE3 (7), got %d values' % (who, rgb2imu.numel()))
    return mask, motion, intr, rgb2imu


def _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel):
    """The device tensors and scalars every entry point takes (include/islam_hip.h, "dense reprojection"), as one _DenseArgs."""
    from .robust import NONE, _Kernel
    require_cuda(depth, flow)
    dev = depth.device
    if flow.dim() != 4 or flow.shape[1] != 2 or depth.dim() != 3 or (depth.shape[0],) + tuple(depth.shape[1:]) != (flow.shape[0],) + tuple(flow.shape[2:]):
        raise ValueError('dense_reproj: depth must be (B,H,W) and flow (B,2,H,W), got %s and %s' % (tuple(depth.shape), tuple(flow.shape)))
    B, H, W = depth.shape
    depth, flow = _f32c(depth), _f32c(flow)
    mask, motion, intr, rgb2imu = _dense_link_args('dense_reproj', dev, B, H, W, mask, motion, intr, rgb2imu)
    if kernel is not None and not isinstance(kernel, _Kernel):
        raise ValueError('dense_reproj: kernel must be None, Huber(delta) or Cauchy(delta) (got %r)' % (kernel,))
    kind, delta = (NONE, 1.0) if kernel is None else (kernel.kind, kernel.delta)
    return _DenseArgs(dev, B, H, W, depth, flow, mask, motion, intr, rgb2imu, kind, delta)


def _dense_reproj_outputs(B, dev):
    e = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    return DenseReprojNormal(e(B, 6, 6), e(B, 6), e(B), e(B), e(B), e(B, _lib.DENSE_REPROJ_NSUM))


def _dense_lm_outputs(B, dev, trace_cap):
    """What a refinement returns beside the normal equations: pose (B,7), lambda (B), accepted, rejected, status (B) int32 and the
    NaN-filled trace (trace_cap,B) (None for trace_cap = 0)."""
    pose = torch.empty((B, 7), dtype=torch.float64, device=dev)
    lam = torch.empty(B, dtype=torch.float64, device=dev)
    acc, rej, status = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    trace = torch.full((trace_cap, B), float('nan'), dtype=torch.float64, device=dev) if trace_cap > 0 else None
    return pose, lam, acc, rej, status, trace


def _dense_grad_outputs(a):
    """What a VJP entry point fills: (grad_depth (B,H,W), grad_flow (B,2,H,W)), float32."""
    return (torch.empty((a.B, a.H, a.W), dtype=torch.float32, device=a.dev), torch.empty((a.B, 2, a.H, a.W), dtype=torch.float32, device=a.dev))


def _dense_ift_outputs(B, dev):
    """What an ift_weights entry point fills: (the link's row of six (B,6) float64, status (B) int32)."""
    return torch.empty((B, 6), dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)


def dense_reproj_normal(depth, flow, mask, motion, intr, rgb2imu=None, kernel=None):
    """Gauss-Newton normal equations of the dense reprojection residual per link (include/islam_hip.h, "dense reprojection";
    DESIGN.md section 3.23).  depth (B,H,W), flow (B,2,H,W), mask (B,H,W) or None, motion (B,7) SE3 [t, q], intr (4) or (B,4) =
    fx, fy, cx, cy, rgb2imu (7) or None, kernel None / robust.Huber / robust.Cauchy.  Returns DenseReprojNormal(H (B,6,6), g (B,6),
    cost, l1, count (B), sums (B,30)), float64 on the device; nothing is read back."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    out = _dense_reproj_outputs(a.B, a.dev)
    scratch = torch.empty(lib().islam_dense_reproj_scratch_bytes(a.B, 0), dtype=torch.uint8, device=a.dev)
    check(lib().islam_dense_reproj_normal(*a.head(), a.kind, a.delta, ptr(out.H), ptr(out.g), ptr(out.cost), ptr(out.l1), ptr(out.count),
                                          ptr(out.sums), ptr(scratch), a.B, a.H, a.W, stream_ptr(a.dev)))
    return out


def dense_reproj_refine(depth, flow, mask, motion, intr, rgb2imu=None, kernel=None, iters=10, damping=1e-4, min_count=16, trace_cap=0):
    """``iters`` Levenberg-Marquardt evaluations on the dense reprojection cost of each link, all on the device (accept rule and
    schedule: include/islam_hip.h, islam_dense_reproj_refine).  Arguments as dense_reproj_normal; damping: the initial lambda;
    min_count: fewest valid pixels a pose may have.  Returns DenseReprojRefined: motion (B,7) and H, g, cost, l1, count, sums at it,
    damping (B), accepted, rejected, status (B) int32 (0, or _lib.DENSE_REPROJ_FEW / _NOTPD: that link's pose came back as it
    stood) and trace (trace_cap,B) = the mean cost of each evaluation (None for trace_cap = 0)."""
    return _dense_reproj_refine_launch(_dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel), iters, damping, min_count, trace_cap)


def _dense_reproj_refine_launch(a, iters, damping, min_count, trace_cap):
    """islam_dense_reproj_refine on what _dense_reproj_args prepared."""
    iters, trace_cap = int(iters), int(trace_cap)
    out = _dense_reproj_outputs(a.B, a.dev)
    pose, lam, acc, rej, status, trace = _dense_lm_outputs(a.B, a.dev, trace_cap)
    scratch = torch.empty(lib().islam_dense_reproj_scratch_bytes(a.B, max(iters, 1)), dtype=torch.uint8, device=a.dev)
    check(lib().islam_dense_reproj_refine(*a.head(), a.kind, a.delta, iters, float(damping), float(min_count), ptr(pose), ptr(out.H),
                                          ptr(out.g), ptr(out.cost), ptr(out.l1), ptr(out.count), ptr(out.sums), ptr(lam), ptr(acc), ptr(rej),
                                          ptr(status), ptr(trace), trace_cap, ptr(scratch), a.B, a.H, a.W, stream_ptr(a.dev)))
    return DenseReprojRefined(pose, *out, lam, acc, rej, status, trace)


DenseBANormal = collections.namedtuple('DenseBANormal', 'S g cost l1 count sums')
DenseBARefined = collections.namedtuple('DenseBARefined', 'motion inv_depth S g cost l1 count sums damping accepted rejected status trace')


def _dense_ba_prior_weight(prior_weight, B, dev):
    """prior_weight as a (B,) float64 device tensor.  A host-side number is validated here; a device tensor is not read back (a
    non-positive entry marks its link with _lib.DENSE_REPROJ_BADPRIOR on the device)."""
    if not torch.is_tensor(prior_weight):
        prior_weight = torch.as_tensor(prior_weight, dtype=torch.float64)
    if not prior_weight.is_cuda and not bool(((prior_weight > 0) & torch.isfinite(prior_weight)).all()):
        raise ValueError('dense_ba: prior_weight must be finite and positive (got %s)' % (prior_weight.tolist(),))
    w = prior_weight.detach().to(dev, torch.float64)
    if w.numel() == 1:
        w = w.reshape(1).expand(B)
    if tuple(w.shape) != (B,):
        raise ValueError('dense_ba: prior_weight must be a number or (%d,), got %s' % (B, tuple(w.shape)))
    return w.contiguous()


def _dense_ba_prior_scale(prior_scale, a, who):
    """prior_scale (B,H,W) as a contiguous float32 device tensor (None stays None); nothing is read back."""
    if prior_scale is None:
        return None
    require_cuda(prior_scale)
    if tuple(prior_scale.shape) != (a.B, a.H, a.W):
        raise ValueError('%s: prior_scale must be (%d,%d,%d), got %s' % (who, a.B, a.H, a.W, tuple(prior_scale.shape)))
    return _f32c(prior_scale.detach().to(a.dev))


def dense_ba_normal(depth, flow, mask, motion, intr, prior_weight, inv_depth=None, rgb2imu=None, kernel=None, prior_scale=None):
    """The depth-marginalised normal equations of the joint (pose, inverse depth) dense reprojection problem per link
    (include/islam_hip.h, islam_dense_ba_normal).  Arguments as dense_reproj_normal, plus prior_weight (a
    positive number or (B,)) = sigma_px^2 / sigma_inv_depth^2 and inv_depth (B,H,W) float64, the state's inverse depths (None: the
    prior 1/depth).  prior_scale (B,H,W) on the device or None: a per-pixel factor m on the prior weight, w_i = prior_weight[b] m_i
    (float32; a pixel whose m is not finite or is <= 0 has no prior; islam_dense_ba_normal_map, section 3.27).  Returns
    DenseBANormal(S (B,6,6), g (B,6), cost, l1, count (B), sums (B,30)), float64 on the device; nothing is read back."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
    m = _dense_ba_prior_scale(prior_scale, a, 'dense_ba_normal')
    if inv_depth is not None:
        require_cuda(inv_depth)
        inv_depth = _dense_ba_state(inv_depth, a, 'dense_ba')
    out = DenseBANormal(*_dense_reproj_outputs(a.B, a.dev))
    scratch = torch.empty(lib().islam_dense_ba_scratch_bytes(a.B, a.H, a.W, 0), dtype=torch.uint8, device=a.dev)
    tail = (ptr(inv_depth), a.kind, a.delta, ptr(out.S), ptr(out.g), ptr(out.cost), ptr(out.l1), ptr(out.count), ptr(out.sums), ptr(scratch),
            a.B, a.H, a.W, stream_ptr(a.dev))
    if m is None:
        check(lib().islam_dense_ba_normal(*a.head(), ptr(w), *tail))
    else:
        check(lib().islam_dense_ba_normal_map(*a.head(), ptr(w), ptr(m), *tail))
    return out


def dense_ba_refine(depth, flow, mask, motion, intr, prior_weight, rgb2imu=None, kernel=None, iters=20, damping=1e-4, min_count=16,
                    trace_cap=0, prior_scale=None):
    """``iters`` Levenberg-Marquardt evaluations on the joint (pose, inverse depth) problem of each link, all on the device
    (include/islam_hip.h, islam_dense_ba_refine).  Arguments as dense_reproj_refine plus prior_weight and prior_scale (see
    dense_ba_normal; with a map the launch is islam_dense_ba_refine_map).  Returns
    DenseBARefined: motion (B,7), inv_depth (B,H,W) float64 (0 where the depth gives no prior) and S, g, cost, l1, count, sums at
    them, damping, accepted, rejected, status (B) int32 (0, or _lib.DENSE_REPROJ_FEW / _NOTPD / _BADPRIOR) and trace."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    return _dense_ba_refine_launch(a, _dense_ba_prior_weight(prior_weight, a.B, a.dev), iters, damping, min_count, trace_cap,
                                   _dense_ba_prior_scale(prior_scale, a, 'dense_ba_refine'))


def _dense_ba_refine_launch(a, w, iters, damping, min_count, trace_cap, m=None):
    """islam_dense_ba_refine (m (B,H,W) float32: islam_dense_ba_refine_map) on what _dense_reproj_args and _dense_ba_prior_weight prepared."""
    iters, trace_cap = int(iters), int(trace_cap)
    out = _dense_reproj_outputs(a.B, a.dev)
    pose, lam, acc, rej, status, trace = _dense_lm_outputs(a.B, a.dev, trace_cap)
    rho = torch.empty((a.B, a.H, a.W), dtype=torch.float64, device=a.dev)
    scratch = torch.empty(lib().islam_dense_ba_scratch_bytes(a.B, a.H, a.W, max(iters, 1)), dtype=torch.uint8, device=a.dev)
    tail = (a.kind, a.delta, iters, float(damping), float(min_count), ptr(pose), ptr(rho), ptr(out.H), ptr(out.g), ptr(out.cost), ptr(out.l1),
            ptr(out.count), ptr(out.sums), ptr(lam), ptr(acc), ptr(rej), ptr(status), ptr(trace), trace_cap, ptr(scratch), a.B, a.H, a.W,
            stream_ptr(a.dev))
    if m is None:
        check(lib().islam_dense_ba_refine(*a.head(), ptr(w), *tail))
    else:
        check(lib().islam_dense_ba_refine_map(*a.head(), ptr(w), ptr(m), *tail))
    return DenseBARefined(pose, rho, *out, lam, acc, rej, status, trace)


DenseBADepthVar = collections.namedtuple('DenseBADepthVar', 'var status')


def dense_ba_depth_variance(depth, flow, mask, motion, intr, prior_weight, inv_depth=None, sums=None, status=None, prior_scale=None,
                            rgb2imu=None, kernel=None, marginal=True):
    """The posterior variance of every pixel's inverse depth at the state (motion, inv_depth; None: the prior 1/depth), in units of
    sigma_px^2 (include/islam_hip.h, islam_dense_ba_depth_var): v = 1/h_dd + h_cam^T S_cam^-1 h_cam / h_dd^2
    marginal over the pose, 1/h_dd conditional on it (marginal=False), 1/w_i at a pixel with a prior that is invalid at the state, NaN
    at one without a usable prior.  sums (B,30): the camera-frame sums dense_ba_normal / dense_ba_refine returned at this state (None:
    dense_ba_normal is called here); status (B) int or None: the refinement's status; other arguments as dense_ba_normal.  Returns
    DenseBADepthVar(var (B,H,W) float64, status (B) int32: the incoming status, _lib.DENSE_REPROJ_BADPRIOR, or _NOTPD for sums that
    are not finite or an S_cam that is not positive definite; such a link's map is all NaN).  Two launches, nothing is read back."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
    m = _dense_ba_prior_scale(prior_scale, a, 'dense_ba_depth_variance')
    if inv_depth is not None:
        require_cuda(inv_depth)
        inv_depth = _dense_ba_state(inv_depth, a, 'dense_ba_depth_variance')
    if sums is None:
        sums = dense_ba_normal(a.depth, a.flow, a.mask, a.motion, a.intr, w, inv_depth=inv_depth, rgb2imu=a.rgb2imu, kernel=kernel,
                               prior_scale=m).sums
    sums = torch.as_tensor(sums).detach().to(a.dev, torch.float64).contiguous()
    if tuple(sums.shape) != (a.B, _lib.DENSE_REPROJ_NSUM):
        raise ValueError('dense_ba_depth_variance: sums must be (%d,%d), got %s' % (a.B, _lib.DENSE_REPROJ_NSUM, tuple(sums.shape)))
    status = _dense_reproj_status(status, a.B, a.dev)
    var = torch.empty((a.B, a.H, a.W), dtype=torch.float64, device=a.dev)
    out = torch.empty(a.B, dtype=torch.int32, device=a.dev)
    scratch = torch.empty(lib().islam_dense_ba_depth_var_scratch_bytes(a.B), dtype=torch.uint8, device=a.dev)
    check(lib().islam_dense_ba_depth_var(*a.head(), ptr(w), ptr(m), ptr(inv_depth), ptr(sums), ptr(status), a.kind, a.delta,
                                         0 if marginal else 1, ptr(var), ptr(out), ptr(scratch), a.B, a.H, a.W, stream_ptr(a.dev)))
    return DenseBADepthVar(var, out)


DenseBADepthVarGrad = collections.namedtuple('DenseBADepthVarGrad', 'grad_inv_depth grad_flow grad_motion status')


def dense_ba_depth_variance_vjp(depth, flow, mask, motion, intr, prior_weight, inv_depth, sums, grad_var, status=None, prior_scale=None,
                                rgb2imu=None, kernel=None, marginal=True):
    """The vector-Jacobian product of dense_ba_depth_variance: the total derivative of v in the state (inv_depth, motion, flow), S_cam
    being a function of that same state (include/islam_hip.h, islam_dense_ba_depth_var_vjp).  Arguments as the
    forward call was given them, with inv_depth (B,H,W) and sums (B,30) (the sums at the state) required; grad_var (B,H,W): the
    cotangent of var, read only at the pixels that are valid at the state (it may be NaN where var is NaN).  The valid set and the
    branch of the Huber kernel are held fixed; prior_weight, prior_scale, intr, rgb2imu, the mask and the stored depth get no
    gradient.  Returns DenseBADepthVarGrad(grad_inv_depth (B,H,W) float64, grad_flow (B,2,H,W) float32, grad_motion (B,7) float64 on the
    plain components [t, q xyzw] (the convention of dense_ba_depth_propagate_vjp), status (B) int32 as the forward call forms it).  A
    pixel whose var is 1/w_i or NaN gets exact zeros, and so does every output of a link whose status is not 0.  At most four launches,
    nothing is read back."""
    who = 'dense_ba_depth_variance_vjp'
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
    m = _dense_ba_prior_scale(prior_scale, a, who)
    if inv_depth is None or sums is None or grad_var is None:
        raise ValueError('%s: inv_depth, sums and grad_var are required' % who)
    require_cuda(inv_depth, grad_var)
    inv_depth = _dense_ba_state(inv_depth, a, who)
    grad_var = _dense_ba_state(grad_var, a, who, 'grad_var')
    sums = torch.as_tensor(sums).detach().to(a.dev, torch.float64).contiguous()
    if tuple(sums.shape) != (a.B, _lib.DENSE_REPROJ_NSUM):
        raise ValueError('%s: sums must be (%d,%d), got %s' % (who, a.B, _lib.DENSE_REPROJ_NSUM, tuple(sums.shape)))
    status = _dense_reproj_status(status, a.B, a.dev)
    e = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=a.dev)
    out = DenseBADepthVarGrad(e(torch.float64, a.B, a.H, a.W), e(torch.float32, a.B, 2, a.H, a.W), e(torch.float64, a.B, 7), e(torch.int32, a.B))
    scratch = torch.empty(lib().islam_dense_ba_depth_var_vjp_scratch_bytes(a.B), dtype=torch.uint8, device=a.dev)
    check(lib().islam_dense_ba_depth_var_vjp(*a.head(), ptr(w), ptr(m), ptr(inv_depth), ptr(sums), ptr(status), a.kind, a.delta,
                                             0 if marginal else 1, ptr(grad_var), ptr(out.grad_inv_depth), ptr(out.grad_flow),
                                             ptr(out.grad_motion), ptr(out.status), ptr(scratch), a.B, a.H, a.W, stream_ptr(a.dev)))
    return out


class _DenseBADepthVariance(torch.autograd.Function):
    """dense_ba_depth_variance whose var output carries the total derivative of the variance in flow, motion and inv_depth (DESIGN.md
    section 3.32): forward is that call (the same launches, the same bits), backward is dense_ba_depth_variance_vjp on the same tensors,
    and nothing else.  sums is the state's own function and gets no gradient of its own; depth, the mask, the intrinsics, the prior
    weight and map and the mount get none either."""

    @staticmethod
    def forward(ctx, depth, flow, mask, motion, intr, prior_weight, inv_depth, sums, status, prior_scale, rgb2imu, kernel, marginal):
        out = dense_ba_depth_variance(depth, flow, mask, motion, intr, prior_weight, inv_depth=inv_depth, sums=sums, status=status,
                                      prior_scale=prior_scale, rgb2imu=rgb2imu, kernel=kernel, marginal=marginal)
        ctx.save_for_backward(depth, flow, mask, motion, intr, inv_depth, sums, status, prior_scale, rgb2imu,
                              prior_weight if torch.is_tensor(prior_weight) else None)
        ctx.prior_weight = None if torch.is_tensor(prior_weight) else prior_weight
        ctx.kernel, ctx.marginal = kernel, marginal
        ctx.dtypes = (flow.dtype, motion.dtype, inv_depth.dtype)
        ctx.mark_non_differentiable(out.status)
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_var, *unused):
        need = ctx.needs_input_grad
        if grad_var is None or not (need[1] or need[3] or need[6]):
            return (None,) * 13
        depth, flow, mask, motion, intr, inv_depth, sums, status, prior_scale, rgb2imu, w = ctx.saved_tensors
        g = dense_ba_depth_variance_vjp(depth, flow, mask, motion, intr, ctx.prior_weight if w is None else w, inv_depth, sums, grad_var,
                                        status=status, prior_scale=prior_scale, rgb2imu=rgb2imu, kernel=ctx.kernel, marginal=ctx.marginal)
        d = ctx.dtypes
        return (None, g.grad_flow.to(d[0]) if need[1] else None, None, g.grad_motion.to(d[1]) if need[3] else None, None, None,
                g.grad_inv_depth.to(d[2]) if need[6] else None, None, None, None, None, None, None)


def _dense_reproj_status(status, B, dev):
    if status is None:
        return None
    status = torch.as_tensor(status).to(dev, torch.int32).contiguous()
    if tuple(status.shape) != (B,):
        raise ValueError('dense_reproj: status must be (%d), got %s' % (B, tuple(status.shape)))
    return status


def _link_variance(who, name, value, B, dev):
    """A variance per link (process_var, dist_var) as a contiguous (B,) float64 device tensor.  A number or a host tensor is checked
    here (finite, non-negative); a device tensor is not read back: its bad entries are marked on the device."""
    if not torch.is_tensor(value):
        value = torch.as_tensor(value, dtype=torch.float64)
    if not value.is_cuda and not bool(((value >= 0) & torch.isfinite(value)).all()):
        raise ValueError('%s: %s must be finite and non-negative (got %s)' % (who, name, value.tolist()))
    v = value.detach().to(dev, torch.float64)
    if v.numel() == 1:
        v = v.reshape(1).expand(B)
    if tuple(v.shape) != (B,):
        raise ValueError('%s: %s must be a number or (%d,), got %s' % (who, name, B, tuple(v.shape)))
    return v.contiguous()


def _next_measurement(who, depth_next, var_next, gate, B, H, W, dev):
    """The second frame's measurement as the fusion takes it: depth_next and var_next (B,H,W) contiguous float32 on dev, or both None,
    and gate as a finite non-negative float."""
    if (depth_next is None) != (var_next is None):
        raise ValueError('%s: depth_next and var_next come together or not at all' % who)
    if depth_next is not None:
        if tuple(depth_next.shape) != (B, H, W) or tuple(var_next.shape) != (B, H, W):
            raise ValueError('%s: depth_next and var_next must be (%d,%d,%d), got %s and %s' % (
                who, B, H, W, tuple(depth_next.shape), tuple(var_next.shape)))
        depth_next, var_next = _f32c(depth_next.detach().to(dev)), _f32c(var_next.detach().to(dev))
    gate = float(gate)
    if not (gate >= 0.0 and gate < float('inf')):
        raise ValueError('%s: gate must be finite and non-negative (got %r)' % (who, gate))
    return depth_next, var_next, gate


DenseBAPropagated = collections.namedtuple('DenseBAPropagated', 'inv_depth var_inv_depth depth source flags status')


def dense_ba_depth_propagate(inv_depth, var_inv_depth, motion, intr, mask=None, status=None, rgb2imu=None, process_var=0.0, depth_next=None,
                             var_next=None, gate=0.0):
    """The inverse depths and variances of the first frame of each link carried into the pixel grid of its second frame and fused
    there with that frame's own measurement (include/islam_hip.h, islam_depth_propagate).  inv_depth,
    var_inv_depth (B,H,W): the state a joint refinement returned and its variance in 1/m^2 (sigma_px^2 v of dense_ba_depth_variance; a
    pixel whose variance is NaN, or not > 0, is not carried over); motion (B,7) SE3 [t, q]; intr (4) or (B,4); mask (B,H,W) or None;
    status (B) int or None: a link whose status is not 0 propagates nothing; rgb2imu (7) or None; process_var: a non-negative number
    or (B,), added to every propagated variance (a device tensor is not read back: a negative or non-finite entry marks its link with
    _lib.DENSE_REPROJ_BADPRIOR on the device); depth_next, var_next (B,H,W) on the device or both None: the second frame's depth and
    the variance of its inverse depth; gate >= 0: a propagated value further than gate standard deviations from the measurement gives
    way to it (0: never).  Returns DenseBAPropagated(inv_depth, var_inv_depth (B,H,W) float64: 0 and NaN where nothing is known, depth
    (B,H,W) float32, source (B,H,W) int32: the source pixel that won the z-buffer or -1, flags (B,H,W) uint8: 1 propagated, 2 measured,
    4 gated out, status (B) int32).  One memset and two launches, nothing is read back."""
    dev = inv_depth.device
    if inv_depth.dim() != 3 or tuple(var_inv_depth.shape) != tuple(inv_depth.shape):
        raise ValueError('dense_ba_depth_propagate: inv_depth and var_inv_depth must be (B,H,W), got %s and %s' % (
            tuple(inv_depth.shape), tuple(var_inv_depth.shape)))
    B, H, W = inv_depth.shape
    rho, var = (t.detach().to(dev, torch.float64).contiguous() for t in (inv_depth, var_inv_depth))
    mask, motion, intr, rgb2imu = _dense_link_args('dense_ba_depth_propagate', dev, B, H, W, mask, motion, intr, rgb2imu)
    pv = _link_variance('dense_ba_depth_propagate', 'process_var', process_var, B, dev)
    depth_next, var_next, gate = _next_measurement('dense_ba_depth_propagate', depth_next, var_next, gate, B, H, W, dev)
    status = _dense_reproj_status(status, B, dev)
    require_cuda(inv_depth, var_inv_depth, depth_next, var_next)      # after the argument rules, which need no device
    e = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    out = DenseBAPropagated(e(torch.float64, B, H, W), e(torch.float64, B, H, W), e(torch.float32, B, H, W), e(torch.int32, B, H, W),
                            e(torch.uint8, B, H, W), e(torch.int32, B))
    scratch = torch.empty(lib().islam_depth_propagate_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    check(lib().islam_depth_propagate(ptr(rho), ptr(var), ptr(mask), ptr(motion), ptr(rgb2imu), ptr(intr), ptr(status), ptr(pv),
                                      ptr(depth_next), ptr(var_next), gate, ptr(out.inv_depth), ptr(out.var_inv_depth), ptr(out.depth),
                                      ptr(out.source), ptr(out.flags), ptr(out.status), ptr(scratch), B, H, W, stream_ptr(dev)))
    return out


DenseBAPropagateGrad = collections.namedtuple('DenseBAPropagateGrad', 'grad_inv_depth grad_var_inv_depth grad_motion grad_depth_next grad_var_next')


def dense_ba_depth_propagate_vjp(inv_depth, var_inv_depth, motion, intr, source, flags, status, grad_inv_depth=None, grad_var_inv_depth=None,
                                 rgb2imu=None, process_var=0.0, depth_next=None, var_next=None):
    """The vector-Jacobian product of dense_ba_depth_propagate on the piece its forward pass chose (include/islam_hip.h,
    islam_depth_propagate_vjp).  inv_depth, var_inv_depth, motion, intr, rgb2imu, process_var, depth_next,
    var_next: what the forward call was given (the mask is not needed); source, flags (B,H,W) and status (B): what it returned;
    grad_inv_depth, grad_var_inv_depth (B,H,W) or None (zero): the cotangents of its inv_depth and var_inv_depth outputs, read only
    where flags is not 0 (they may be NaN where nothing is known).  The target pixel, the z-buffer winner and the row of the fusion
    table are held fixed.  Returns DenseBAPropagateGrad(grad_inv_depth, grad_var_inv_depth (B,H,W) float64: exactly 0 at a source pixel
    that did not win its target, grad_motion (B,7) float64 on the plain components [t, q xyzw] (what dense_ba_newton_weights and
    dense_ba_ift_weights take as grad_motion), grad_depth_next, grad_var_next (B,H,W) float32, None without a measurement).  A link
    whose status is not 0 gets zeros on its state and motion; its measurement still gets its gradient.  Two launches, nothing is read
    back."""
    who = 'dense_ba_depth_propagate_vjp'
    dev = inv_depth.device
    if inv_depth.dim() != 3 or tuple(var_inv_depth.shape) != tuple(inv_depth.shape):
        raise ValueError('%s: inv_depth and var_inv_depth must be (B,H,W), got %s and %s' % (who, tuple(inv_depth.shape), tuple(var_inv_depth.shape)))
    B, H, W = inv_depth.shape
    rho, var = (t.detach().to(dev, torch.float64).contiguous() for t in (inv_depth, var_inv_depth))
    _, motion, intr, rgb2imu = _dense_link_args(who, dev, B, H, W, None, motion, intr, rgb2imu)
    pv = _link_variance(who, 'process_var', process_var, B, dev)
    depth_next, var_next, _ = _next_measurement(who, depth_next, var_next, 0.0, B, H, W, dev)
    if tuple(source.shape) != (B, H, W) or tuple(flags.shape) != (B, H, W):
        raise ValueError('%s: source and flags must be (%d,%d,%d), got %s and %s' % (who, B, H, W, tuple(source.shape), tuple(flags.shape)))
    source, flags = source.to(dev, torch.int32).contiguous(), flags.to(dev, torch.uint8).contiguous()
    if status is None:
        raise ValueError('%s: status must be the (%d,) status the forward call returned' % (who, B))
    status = _dense_reproj_status(status, B, dev)
    cots = []
    for name, g in (('grad_inv_depth', grad_inv_depth), ('grad_var_inv_depth', grad_var_inv_depth)):
        if g is not None:
            if tuple(g.shape) != (B, H, W):
                raise ValueError('%s: %s must be (%d,%d,%d), got %s' % (who, name, B, H, W, tuple(g.shape)))
            g = g.detach().to(dev, torch.float64).contiguous()
        cots.append(g)
    require_cuda(inv_depth, var_inv_depth, depth_next, var_next)      # after the argument rules, which need no device
    e = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    meas = depth_next is not None
    out = DenseBAPropagateGrad(e(torch.float64, B, H, W), e(torch.float64, B, H, W), e(torch.float64, B, 7),
                               e(torch.float32, B, H, W) if meas else None, e(torch.float32, B, H, W) if meas else None)
    scratch = torch.empty(lib().islam_depth_propagate_vjp_scratch_bytes(B), dtype=torch.uint8, device=dev)
    check(lib().islam_depth_propagate_vjp(ptr(rho), ptr(var), ptr(motion), ptr(rgb2imu), ptr(intr), ptr(pv), ptr(depth_next), ptr(var_next),
                                          ptr(source), ptr(flags), ptr(status), ptr(cots[0]), ptr(cots[1]), ptr(out.grad_inv_depth),
                                          ptr(out.grad_var_inv_depth), ptr(out.grad_motion), ptr(out.grad_depth_next),
                                          ptr(out.grad_var_next), ptr(scratch), B, H, W, stream_ptr(dev)))
    return out


class _DenseBAPropagate(torch.autograd.Function):
    """dense_ba_depth_propagate whose inv_depth and var_inv_depth outputs carry the gradient of the piece the forward pass chose in
    inv_depth, var_inv_depth, motion, depth_next and var_next: forward is that call, backward is
    dense_ba_depth_propagate_vjp on the same tensors with the source, flags and status forward returned, and nothing else.  The mask,
    the intrinsics, the mount, process_var and the gate get no gradient."""

    @staticmethod
    def forward(ctx, inv_depth, var_inv_depth, motion, intr, mask, status, rgb2imu, process_var, depth_next, var_next, gate):
        out = dense_ba_depth_propagate(inv_depth, var_inv_depth, motion, intr, mask=mask, status=status, rgb2imu=rgb2imu, process_var=process_var,
                                       depth_next=depth_next, var_next=var_next, gate=gate)
        ctx.save_for_backward(inv_depth, var_inv_depth, motion, intr, rgb2imu, depth_next, var_next, out.source, out.flags, out.status)
        ctx.process_var = process_var.detach() if torch.is_tensor(process_var) else process_var
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (inv_depth, var_inv_depth, motion, depth_next, var_next))
        ctx.mark_non_differentiable(out.depth, out.source, out.flags, out.status)
        ctx.set_materialize_grads(False)          # a cotangent the loss does not give arrives as None: the kernel takes NULL for zero
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_inv_depth, grad_var_inv_depth, *unused):
        none = (None,) * 11
        need = ctx.needs_input_grad
        if not (need[0] or need[1] or need[2] or need[8] or need[9]):
            return none
        rho, var, motion, intr, rgb2imu, depth_next, var_next, source, flags, status = ctx.saved_tensors
        pv = ctx.process_var
        g = dense_ba_depth_propagate_vjp(rho, var, motion, intr, source, flags, status, grad_inv_depth=grad_inv_depth,
                                         grad_var_inv_depth=grad_var_inv_depth, rgb2imu=rgb2imu, process_var=pv, depth_next=depth_next,
                                         var_next=var_next)
        d = ctx.dtypes
        return (g.grad_inv_depth.to(d[0]) if need[0] else None, g.grad_var_inv_depth.to(d[1]) if need[1] else None,
                g.grad_motion.to(d[2]) if need[2] else None, None, None, None, None, None,
                g.grad_depth_next.to(d[3]) if need[8] else None, g.grad_var_next.to(d[4]) if need[9] else None, None)


def _regularize_stage_args(who, occl_radius, occl_min, fill_radius, fill_min, fill_inflate, smooth_radius, reg_gate):
    """The stage arguments of the regularisation as the library takes them: ([occl_radius, fill_radius, smooth_radius] as ints,
    fill_inflate, reg_gate as floats), ValueError for what islam_depth_regularize would refuse."""
    radii = [int(r) for r in (occl_radius, fill_radius, smooth_radius)]
    if any(r not in (0, 1, 2) or r != x for r, x in zip(radii, (occl_radius, fill_radius, smooth_radius))):
        raise ValueError('%s: occl_radius, fill_radius and smooth_radius must be 0, 1 or 2 (got %r, %r, %r)' % (
            who, occl_radius, fill_radius, smooth_radius))
    if int(occl_min) != occl_min or int(fill_min) != fill_min or occl_min < 1 or fill_min < 1:
        raise ValueError('%s: occl_min and fill_min must be integers >= 1 (got %r, %r)' % (who, occl_min, fill_min))
    fill_inflate, reg_gate = float(fill_inflate), float(reg_gate)
    if not (fill_inflate >= 1.0 and fill_inflate < float('inf')):
        raise ValueError('%s: fill_inflate must be finite and at least 1 (got %r)' % (who, fill_inflate))
    if not (reg_gate > 0.0 and reg_gate < float('inf')):
        raise ValueError('%s: reg_gate must be finite and positive (got %r)' % (who, reg_gate))
    return radii, fill_inflate, reg_gate


DenseBARegularized = collections.namedtuple('DenseBARegularized', 'inv_depth var_inv_depth depth source flags status')


def dense_ba_depth_regularize(inv_depth, var_inv_depth, source=None, status=None, dist_var=0.0, depth_next=None, var_next=None, gate=0.0,
                              occl_radius=1, occl_min=2, fill_radius=1, fill_min=3, fill_inflate=1.0, smooth_radius=1, reg_gate=3.0):
    """Occlusion removal, hole filling and smoothing of a propagated inverse-depth map, then the fusion with the second frame's own
    measurement (include/islam_hip.h, islam_depth_regularize).  inv_depth, var_inv_depth (B,H,W): what
    dense_ba_depth_propagate returned without a measurement (a pixel whose values are not finite and > 0 is a hole); source (B,H,W)
    int or None and status (B) int or None: that call's source map and status (a link whose status is not 0 gets the measurement
    alone); dist_var: a non-negative number or (B,), the variance a neighbour's value gains per squared pixel of distance in the
    smoothing (a device tensor is not read back: a negative or non-finite entry marks its link with _lib.DENSE_REPROJ_BADPRIOR on the
    device); depth_next, var_next, gate as in dense_ba_depth_propagate.  The stages: a pixel with at least occl_min nearer neighbours
    that are incompatible with it at reg_gate standard deviations within occl_radius, and more of them than compatible ones, is
    removed; a hole with at least fill_min mutually compatible neighbours around its nearest one within fill_radius takes their
    weighted mean, and fill_inflate >= 1 times the variance of one of them plus their scatter; every value becomes the weighted mean
    of its compatible neighbours within smooth_radius and keeps its variance.  A radius is 0 (the stage is left out), 1 or 2.  Returns
    DenseBARegularized(inv_depth, var_inv_depth (B,H,W) float64, depth (B,H,W) float32, source (B,H,W) int32: -1 at filled and removed
    pixels, flags (B,H,W) uint8: 1 a value is present, 2 measured, 4 gated out, 8 filled, 16 removed, status (B) int32).  One launch,
    nothing is read back."""
    who = 'dense_ba_depth_regularize'
    dev = inv_depth.device
    if inv_depth.dim() != 3 or tuple(var_inv_depth.shape) != tuple(inv_depth.shape):
        raise ValueError('%s: inv_depth and var_inv_depth must be (B,H,W), got %s and %s' % (who, tuple(inv_depth.shape), tuple(var_inv_depth.shape)))
    B, H, W = inv_depth.shape
    rho, var = (t.detach().to(dev, torch.float64).contiguous() for t in (inv_depth, var_inv_depth))
    if source is not None:
        if tuple(source.shape) != (B, H, W):
            raise ValueError('%s: source must be (%d,%d,%d), got %s' % (who, B, H, W, tuple(source.shape)))
        source = source.to(dev, torch.int32).contiguous()
    dv = _link_variance(who, 'dist_var', dist_var, B, dev)
    depth_next, var_next, gate = _next_measurement(who, depth_next, var_next, gate, B, H, W, dev)
    radii, fill_inflate, reg_gate = _regularize_stage_args(who, occl_radius, occl_min, fill_radius, fill_min, fill_inflate, smooth_radius, reg_gate)
    status = _dense_reproj_status(status, B, dev)
    require_cuda(inv_depth, var_inv_depth, depth_next, var_next)      # after the argument rules, which need no device
    e = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    out = DenseBARegularized(e(torch.float64, B, H, W), e(torch.float64, B, H, W), e(torch.float32, B, H, W), e(torch.int32, B, H, W),
                             e(torch.uint8, B, H, W), e(torch.int32, B))
    nbytes = lib().islam_depth_regularize_scratch_bytes(B, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    check(lib().islam_depth_regularize(ptr(rho), ptr(var), ptr(source), ptr(status), ptr(dv), ptr(depth_next), ptr(var_next), gate, radii[0],
                                       int(occl_min), radii[1], int(fill_min), fill_inflate, radii[2], reg_gate, ptr(out.inv_depth),
                                       ptr(out.var_inv_depth), ptr(out.depth), ptr(out.source), ptr(out.flags), ptr(out.status),
                                       ptr(scratch), B, H, W, stream_ptr(dev)))
    return out


DenseBARegularizeGrad = collections.namedtuple('DenseBARegularizeGrad', 'grad_inv_depth grad_var_inv_depth grad_depth_next grad_var_next')


def dense_ba_depth_regularize_vjp(inv_depth, var_inv_depth, flags, status=None, grad_inv_depth=None, grad_var_inv_depth=None, dist_var=0.0,
                                  depth_next=None, var_next=None, gate=0.0, occl_radius=1, occl_min=2, fill_radius=1, fill_min=3,
                                  fill_inflate=1.0, smooth_radius=1, reg_gate=3.0):
    """The vector-Jacobian product of dense_ba_depth_regularize on the piece its forward pass chose (include/islam_hip.h,
    islam_depth_regularize_vjp).  inv_depth, var_inv_depth, dist_var, depth_next, var_next, gate and the stage
    arguments: what the forward call was given (the source map is not needed); flags (B,H,W): what it returned; status (B) or None: the
    status it returned (or the one it was given: dist_var marks its links again on the device); grad_inv_depth, grad_var_inv_depth
    (B,H,W) or None (zero): the cotangents of its inv_depth and var_inv_depth outputs, read only where flags & 3 is not 0 (they may be
    NaN where nothing is known).  Every compat decision, the removed and filled sets, each hole's anchor and cluster, each pixel's
    smoothing set and the row of the fusion table are held fixed.  Returns DenseBARegularizeGrad(grad_inv_depth, grad_var_inv_depth
    (B,H,W) float64: exactly 0 at every pixel that stage 1 did not keep, grad_depth_next, grad_var_next (B,H,W) float32, None without a
    measurement).  A link with a status gets zeros on its state; its measurement still gets its gradient.  dist_var, gate and the
    stage arguments get no gradient.  At most three launches, nothing is read back."""
    who = 'dense_ba_depth_regularize_vjp'
    dev = inv_depth.device
    if inv_depth.dim() != 3 or tuple(var_inv_depth.shape) != tuple(inv_depth.shape):
        raise ValueError('%s: inv_depth and var_inv_depth must be (B,H,W), got %s and %s' % (who, tuple(inv_depth.shape), tuple(var_inv_depth.shape)))
    B, H, W = inv_depth.shape
    rho, var = (t.detach().to(dev, torch.float64).contiguous() for t in (inv_depth, var_inv_depth))
    if flags is None or tuple(flags.shape) != (B, H, W):
        raise ValueError('%s: flags must be the (%d,%d,%d) flags the forward call returned, got %s' % (
            who, B, H, W, None if flags is None else tuple(flags.shape)))
    flags = flags.to(dev, torch.uint8).contiguous()
    dv = _link_variance(who, 'dist_var', dist_var, B, dev)
    depth_next, var_next, gate = _next_measurement(who, depth_next, var_next, gate, B, H, W, dev)
    radii, fill_inflate, reg_gate = _regularize_stage_args(who, occl_radius, occl_min, fill_radius, fill_min, fill_inflate, smooth_radius, reg_gate)
    status = _dense_reproj_status(status, B, dev)
    cots = []
    for name, g in (('grad_inv_depth', grad_inv_depth), ('grad_var_inv_depth', grad_var_inv_depth)):
        if g is not None:
            if tuple(g.shape) != (B, H, W):
                raise ValueError('%s: %s must be (%d,%d,%d), got %s' % (who, name, B, H, W, tuple(g.shape)))
            g = g.detach().to(dev, torch.float64).contiguous()
        cots.append(g)
    require_cuda(inv_depth, var_inv_depth, depth_next, var_next)      # after the argument rules, which need no device
    e = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    meas = depth_next is not None
    out = DenseBARegularizeGrad(e(torch.float64, B, H, W), e(torch.float64, B, H, W), e(torch.float32, B, H, W) if meas else None,
                                e(torch.float32, B, H, W) if meas else None)
    scratch = torch.empty(lib().islam_depth_regularize_vjp_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    check(lib().islam_depth_regularize_vjp(ptr(rho), ptr(var), ptr(status), ptr(dv), ptr(depth_next), ptr(var_next), gate, radii[0], int(occl_min),
                                           radii[1], int(fill_min), fill_inflate, radii[2], reg_gate, ptr(flags), ptr(cots[0]), ptr(cots[1]),
                                           ptr(out.grad_inv_depth), ptr(out.grad_var_inv_depth), ptr(out.grad_depth_next),
                                           ptr(out.grad_var_next), ptr(scratch), B, H, W, stream_ptr(dev)))
    return out


class _DenseBARegularize(torch.autograd.Function):
    """dense_ba_depth_regularize whose inv_depth and var_inv_depth outputs carry the gradient of the piece the forward pass chose in
    inv_depth, var_inv_depth, depth_next and var_next: forward is that call, backward is
    dense_ba_depth_regularize_vjp on the same tensors with the flags and status forward returned, and nothing else.  The source map,
    the status, dist_var, the gate and ``stages`` (a dict of the stage arguments) get no gradient."""

    @staticmethod
    def forward(ctx, inv_depth, var_inv_depth, source, status, dist_var, depth_next, var_next, gate, stages):
        out = dense_ba_depth_regularize(inv_depth, var_inv_depth, source=source, status=status, dist_var=dist_var, depth_next=depth_next,
                                        var_next=var_next, gate=gate, **stages)
        ctx.save_for_backward(inv_depth, var_inv_depth, depth_next, var_next, out.flags, out.status)
        ctx.dist_var = dist_var.detach() if torch.is_tensor(dist_var) else dist_var
        ctx.gate, ctx.stages = gate, dict(stages)
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (inv_depth, var_inv_depth, depth_next, var_next))
        ctx.mark_non_differentiable(out.depth, out.source, out.flags, out.status)
        ctx.set_materialize_grads(False)          # a cotangent the loss does not give arrives as None: the kernel takes NULL for zero
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_inv_depth, grad_var_inv_depth, *unused):
        need = ctx.needs_input_grad
        if not (need[0] or need[1] or need[5] or need[6]):
            return (None,) * 9
        rho, var, depth_next, var_next, flags, status = ctx.saved_tensors
        g = dense_ba_depth_regularize_vjp(rho, var, flags, status=status, grad_inv_depth=grad_inv_depth, grad_var_inv_depth=grad_var_inv_depth,
                                          dist_var=ctx.dist_var, depth_next=depth_next, var_next=var_next, gate=ctx.gate, **ctx.stages)
        d = ctx.dtypes
        return (g.grad_inv_depth.to(d[0]) if need[0] else None, g.grad_var_inv_depth.to(d[1]) if need[1] else None, None, None, None,
                g.grad_depth_next.to(d[2]) if need[5] else None, g.grad_var_next.to(d[3]) if need[6] else None, None, None)


def dense_reproj_vjp(depth, flow, mask, motion, intr, w, rgb2imu=None, kernel=None, status=None):
    """The derivative of w^T g in depth and flow, g as dense_reproj_normal returns it at ``motion``, with the pose and the valid set
    held fixed (include/islam_hip.h, islam_dense_reproj_vjp).  Arguments as dense_reproj_normal; w (B,6)
    body frame [rho, phi]; status (B) int or None: a link whose status is not 0 gets zeros.  Returns (grad_depth (B,H,W),
    grad_flow (B,2,H,W)), float32 on the device, exactly 0 at every invalid pixel; one launch, nothing is read back."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    w = torch.as_tensor(w).detach().to(a.dev, torch.float64).contiguous()
    if tuple(w.shape) != (a.B, 6):
        raise ValueError('dense_reproj_vjp: w must be (%d,6) [rho, phi], got %s' % (a.B, tuple(w.shape)))
    return _dense_reproj_vjp_launch(a, w, _dense_reproj_status(status, a.B, a.dev))


def _dense_reproj_vjp_launch(a, w, status):
    """islam_dense_reproj_vjp on what _dense_reproj_args prepared."""
    grad_depth, grad_flow = _dense_grad_outputs(a)
    check(lib().islam_dense_reproj_vjp(*a.head(), a.B, a.H, a.W, a.kind, a.delta, ptr(w), ptr(status), ptr(grad_depth), ptr(grad_flow),
                                       stream_ptr(a.dev)))
    return grad_depth, grad_flow


def dense_reproj_ift_weights(H, motion, grad_motion, status=None):
    """w = -H^-1 v per link (include/islam_hip.h, islam_dense_reproj_ift_weights): H (B,6,6) the undamped matrix of a refinement,
    motion (B,7) the pose it ended at, grad_motion (B,7) a loss's gradient on [t, q xyzw] there (v: the same gradient in the right
    tangent of the pose), status (B) int or None the refinement's status.  Returns (w (B,6) float64, status (B) int32): a link with
    an incoming status, or whose H is not positive definite (_lib.DENSE_REPROJ_NOTPD), has w = 0.  One launch, nothing is read back."""
    require_cuda(H)
    dev = H.device
    f64 = lambda t: torch.as_tensor(t).detach().to(dev, torch.float64).contiguous()
    H, motion, grad_motion = f64(H), f64(motion), f64(grad_motion)
    if H.dim() != 3 or tuple(H.shape[1:]) != (6, 6):
        raise ValueError('dense_reproj_ift_weights: H must be (B,6,6), got %s' % (tuple(H.shape),))
    B = H.shape[0]
    if tuple(motion.shape) != (B, 7) or tuple(grad_motion.shape) != (B, 7):
        raise ValueError('dense_reproj_ift_weights: motion and grad_motion must be (%d,7), got %s and %s' % (
            B, tuple(motion.shape), tuple(grad_motion.shape)))
    return _dense_reproj_ift_launch(H, motion, grad_motion, _dense_reproj_status(status, B, dev))


def _dense_reproj_ift_launch(H, motion, grad_motion, status):
    """islam_dense_reproj_ift_weights on contiguous float64 device tensors."""
    B, dev = H.shape[0], H.device
    w, out = _dense_ift_outputs(B, dev)
    check(lib().islam_dense_reproj_ift_weights(ptr(H), ptr(motion), ptr(grad_motion), ptr(status), B, ptr(w), ptr(out), stream_ptr(dev)))
    return w, out


class _DenseReprojRefine(torch.autograd.Function):
    """dense_reproj_refine whose refined motion carries the implicit-function gradient in depth and flow:
    backward is islam_dense_reproj_ift_weights and islam_dense_reproj_vjp at the refined pose on the tensors forward prepared, two
    launches and nothing else.  The start pose gets no gradient: the optimum does not depend on it."""

    @staticmethod
    def forward(ctx, depth, flow, mask, motion, intr, rgb2imu, kernel, iters, damping, min_count, trace_cap):
        a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
        out = _dense_reproj_refine_launch(a, iters, damping, min_count, trace_cap)
        ctx.save_for_backward(a.depth, a.flow, a.mask, out.motion, out.H, out.status, a.intr, a.rgb2imu)
        ctx.kind, ctx.delta, ctx.dtypes = a.kind, a.delta, (depth.dtype, flow.dtype)
        ctx.mark_non_differentiable(*(t for t in out[1:] if t is not None))
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_motion, *unused):
        depth, flow, mask, motion, H, status, intr, rgb2imu = ctx.saved_tensors
        a = _DenseArgs(depth.device, *depth.shape, depth, flow, mask, motion, intr, rgb2imu, ctx.kind, ctx.delta)      # at the refined pose
        w, status = _dense_reproj_ift_launch(H, motion, grad_motion.to(torch.float64).contiguous(), status)
        grad_depth, grad_flow = _dense_reproj_vjp_launch(a, w, status)
        return (grad_depth.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None, grad_flow.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None, None, None, None)


def _dense_ba_state(inv_depth, a, who, name='inv_depth'):
    if tuple(inv_depth.shape) != (a.B, a.H, a.W):
        raise ValueError('%s: %s must be (%d,%d,%d), got %s' % (who, name, a.B, a.H, a.W, tuple(inv_depth.shape)))
    return inv_depth.detach().to(a.dev, torch.float64).contiguous()


def dense_ba_ift_weights(depth, flow, mask, motion, intr, prior_weight, inv_depth, S, grad_motion, grad_inv_depth=None, rgb2imu=None,
                         kernel=None, status=None):
    """lambda_p (B,6) of the joint refinement's implicit gradient (include/islam_hip.h, islam_dense_ba_ift_weights; DESIGN.md section
    3.26): S lambda_p = -(v_p - A^T u_cam) at the state (motion (B,7), inv_depth (B,H,W)) a dense_ba_refine returned with the undamped
    S (B,6,6), for a loss with gradient grad_motion (B,7) on [t, q xyzw] and grad_inv_depth (B,H,W) or None on inv_depth (None skips
    the reduction of u_cam).  Other arguments as dense_ba_normal; status (B) int or None: the refinement's status.  Returns
    (lambda_p float64, status (B) int32): a link with an incoming status, a prior weight that is not > 0 (_lib.DENSE_REPROJ_BADPRIOR)
    or an S that is not positive definite (_NOTPD) has lambda_p = 0.  One or two launches, nothing is read back."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
    rho = _dense_ba_state(inv_depth, a, 'dense_ba_ift_weights')
    f64 = lambda t: torch.as_tensor(t).detach().to(a.dev, torch.float64).contiguous()
    S, grad_motion = f64(S), f64(grad_motion)
    if tuple(S.shape) != (a.B, 6, 6) or tuple(grad_motion.shape) != (a.B, 7):
        raise ValueError('dense_ba_ift_weights: S must be (%d,6,6) and grad_motion (%d,7), got %s and %s' % (
            a.B, a.B, tuple(S.shape), tuple(grad_motion.shape)))
    if grad_inv_depth is not None:
        grad_inv_depth = _dense_ba_state(grad_inv_depth, a, 'dense_ba_ift_weights', 'grad_inv_depth')
    return _dense_ba_ift_launch(a, w, rho, S, grad_motion, grad_inv_depth, _dense_reproj_status(status, a.B, a.dev))


def _dense_ba_ift_launch(a, w, rho, S, grad_motion, grad_rho, status):
    """islam_dense_ba_ift_weights on what _dense_reproj_args prepared."""
    lam, out = _dense_ift_outputs(a.B, a.dev)
    scratch = torch.empty(lib().islam_dense_ba_adjoint_scratch_bytes(a.B), dtype=torch.uint8, device=a.dev)
    check(lib().islam_dense_ba_ift_weights(*a.head(), ptr(w), ptr(rho), a.kind, a.delta, ptr(S), ptr(grad_motion), ptr(grad_rho),
                                           ptr(status), ptr(scratch), a.B, a.H, a.W, ptr(lam), ptr(out), stream_ptr(a.dev)))
    return lam, out


def dense_ba_vjp(depth, flow, mask, motion, intr, prior_weight, inv_depth, lambda_p, grad_inv_depth=None, rgb2imu=None, kernel=None,
                 status=None):
    """The gradient of a loss on a joint refinement's outputs in depth and flow, from lambda_p (B,6) (dense_ba_ift_weights) and the
    loss's gradient grad_inv_depth (B,H,W) or None on inv_depth (include/islam_hip.h, islam_dense_ba_vjp):
    per pixel lambda_d, then dL/dflow = -(c q + 2 c' (q.r) r) and dL/ddepth = w lambda_d / depth^2.  Other arguments as
    dense_ba_normal; status (B) int or None: a link whose status is not 0 gets zeros.  Returns (grad_depth (B,H,W), grad_flow
    (B,2,H,W)), float32 on the device; one launch, nothing is read back."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
    rho = _dense_ba_state(inv_depth, a, 'dense_ba_vjp')
    lambda_p = torch.as_tensor(lambda_p).detach().to(a.dev, torch.float64).contiguous()
    if tuple(lambda_p.shape) != (a.B, 6):
        raise ValueError('dense_ba_vjp: lambda_p must be (%d,6) [rho, phi], got %s' % (a.B, tuple(lambda_p.shape)))
    if grad_inv_depth is not None:
        grad_inv_depth = _dense_ba_state(grad_inv_depth, a, 'dense_ba_vjp', 'grad_inv_depth')
    return _dense_ba_vjp_launch(a, w, rho, lambda_p, grad_inv_depth, _dense_reproj_status(status, a.B, a.dev))


def _dense_ba_vjp_launch(a, w, rho, lambda_p, grad_rho, status):
    """islam_dense_ba_vjp on what _dense_reproj_args prepared."""
    grad_depth, grad_flow = _dense_grad_outputs(a)
    check(lib().islam_dense_ba_vjp(*a.head(), ptr(w), ptr(rho), a.kind, a.delta, ptr(lambda_p), ptr(grad_rho), ptr(status),
                                   ptr(grad_depth), ptr(grad_flow), a.B, a.H, a.W, stream_ptr(a.dev)))
    return grad_depth, grad_flow


class _DenseBARefine(torch.autograd.Function):
    """dense_ba_refine whose refined motion and inv_depth carry the implicit-function gradient in depth and flow (DESIGN.md section
    3.26): backward is islam_dense_ba_ift_weights (two launches, one when no gradient arrives on inv_depth) and islam_dense_ba_vjp at
    the refined state on the tensors forward prepared, and nothing else.  The start pose and the prior weight get no gradient."""

    @staticmethod
    def forward(ctx, depth, flow, mask, motion, intr, prior_weight, rgb2imu, kernel, iters, damping, min_count, trace_cap):
        a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
        w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
        out = _dense_ba_refine_launch(a, w, iters, damping, min_count, trace_cap)
        ctx.save_for_backward(a.depth, a.flow, a.mask, out.motion, out.inv_depth, out.S, out.status, a.intr, a.rgb2imu, w)
        ctx.kind, ctx.delta, ctx.dtypes = a.kind, a.delta, (depth.dtype, flow.dtype)
        ctx.mark_non_differentiable(*(t for t in out[2:] if t is not None))
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None: no reduction for it
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_motion, grad_inv_depth, *unused):
        none = (None,) * 12
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return none
        depth, flow, mask, motion, rho, S, status, intr, rgb2imu, w = ctx.saved_tensors
        a = _DenseArgs(depth.device, *depth.shape, depth, flow, mask, motion, intr, rgb2imu, ctx.kind, ctx.delta)      # at the refined state
        grad_motion = torch.zeros_like(motion) if grad_motion is None else grad_motion.to(torch.float64).contiguous()
        if grad_inv_depth is not None:
            grad_inv_depth = grad_inv_depth.to(torch.float64).contiguous()
        lam, status = _dense_ba_ift_launch(a, w, rho, S, grad_motion, grad_inv_depth, status)
        grad_depth, grad_flow = _dense_ba_vjp_launch(a, w, rho, lam, grad_inv_depth, status)
        return (grad_depth.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None,
                grad_flow.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None) + none[2:]


DenseBANewton = collections.namedtuple('DenseBANewton', 'lambda_p S fallback status')


def _dense_ba_newton_state(who, depth, flow, mask, motion, intr, prior_weight, inv_depth, grad_inv_depth, rgb2imu, kernel, prior_scale):
    """What both Newton ops prepare alike: (_DenseArgs, w (B,), m (B,H,W) float32 or None, rho, grad_inv_depth or None)."""
    a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
    w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
    m = _dense_ba_prior_scale(prior_scale, a, who)
    rho = _dense_ba_state(inv_depth, a, who)
    if grad_inv_depth is not None:
        grad_inv_depth = _dense_ba_state(grad_inv_depth, a, who, 'grad_inv_depth')
    return a, w, m, rho, grad_inv_depth


def dense_ba_newton_weights(depth, flow, mask, motion, intr, prior_weight, inv_depth, grad_motion, grad_inv_depth=None, rgb2imu=None,
                            kernel=None, status=None, prior_scale=None):
    """lambda_p (B,6) of the joint refinement's implicit gradient with the exact (Newton) Hessian (include/islam_hip.h,
    islam_dense_ba_newton_weights): S_N lambda_p = -(v_p - A^T u_cam) at the state (motion (B,7), inv_depth
    (B,H,W)) a dense_ba_refine returned, S_N the pose block of one half of the cost's Hessian with the depths eliminated pixel by
    pixel, for a loss with gradient grad_motion (B,7) on [t, q xyzw] and grad_inv_depth (B,H,W) or None on inv_depth.  prior_scale
    (B,H,W) or None: the per-pixel factor on the prior weight the refinement was given; other arguments as dense_ba_ift_weights.
    Returns DenseBANewton(lambda_p (B,6), S (B,6,6) = S_N, body frame, float64; fallback (B) int32: the valid pixels whose exact n_dd
    was not > 0 and that took their Gauss-Newton blocks; status (B) int32: the incoming status, _lib.DENSE_REPROJ_BADPRIOR for a prior
    weight that is not > 0, _NOTPD for an S_N that is not positive definite; lambda_p = 0 for such a link).  Two launches, nothing is
    read back."""
    a, w, m, rho, grad_inv_depth = _dense_ba_newton_state('dense_ba_newton_weights', depth, flow, mask, motion, intr, prior_weight, inv_depth,
                                                          grad_inv_depth, rgb2imu, kernel, prior_scale)
    grad_motion = torch.as_tensor(grad_motion).detach().to(a.dev, torch.float64).contiguous()
    if tuple(grad_motion.shape) != (a.B, 7):
        raise ValueError('dense_ba_newton_weights: grad_motion must be (%d,7), got %s' % (a.B, tuple(grad_motion.shape)))
    return _dense_ba_newton_launch(a, w, m, rho, grad_motion, grad_inv_depth, _dense_reproj_status(status, a.B, a.dev))


def _dense_ba_newton_launch(a, w, m, rho, grad_motion, grad_rho, status):
    """islam_dense_ba_newton_weights on what _dense_ba_newton_state prepared."""
    lam, out = _dense_ift_outputs(a.B, a.dev)
    S = torch.empty((a.B, 6, 6), dtype=torch.float64, device=a.dev)
    fallback = torch.empty(a.B, dtype=torch.int32, device=a.dev)
    scratch = torch.empty(lib().islam_dense_ba_newton_scratch_bytes(a.B), dtype=torch.uint8, device=a.dev)
    check(lib().islam_dense_ba_newton_weights(*a.head(), ptr(w), ptr(m), ptr(rho), a.kind, a.delta, ptr(grad_motion), ptr(grad_rho), ptr(status),
                                              ptr(scratch), a.B, a.H, a.W, ptr(lam), ptr(S), ptr(fallback), ptr(out), stream_ptr(a.dev)))
    return DenseBANewton(lam, S, fallback, out)


def dense_ba_newton_vjp(depth, flow, mask, motion, intr, prior_weight, inv_depth, lambda_p, grad_inv_depth=None, rgb2imu=None, kernel=None,
                        status=None, prior_scale=None):
    """The gradient of a loss on a joint refinement's outputs in depth and flow with the exact Hessian, from lambda_p (B,6)
    (dense_ba_newton_weights) and the loss's gradient grad_inv_depth (B,H,W) or None on inv_depth (include/islam_hip.h,
    islam_dense_ba_newton_vjp): dense_ba_vjp's data gradient with lambda_d from the exact n_pd and n_dd, and
    w_i = prior_weight prior_scale_i under a map.  Returns (grad_depth (B,H,W), grad_flow (B,2,H,W)), float32 on the device; one
    launch, nothing is read back."""
    a, w, m, rho, grad_inv_depth = _dense_ba_newton_state('dense_ba_newton_vjp', depth, flow, mask, motion, intr, prior_weight, inv_depth,
                                                          grad_inv_depth, rgb2imu, kernel, prior_scale)
    lambda_p = torch.as_tensor(lambda_p).detach().to(a.dev, torch.float64).contiguous()
    if tuple(lambda_p.shape) != (a.B, 6):
        raise ValueError('dense_ba_newton_vjp: lambda_p must be (%d,6) [rho, phi], got %s' % (a.B, tuple(lambda_p.shape)))
    return _dense_ba_newton_vjp_launch(a, w, m, rho, lambda_p, grad_inv_depth, _dense_reproj_status(status, a.B, a.dev))


def _dense_ba_newton_vjp_launch(a, w, m, rho, lambda_p, grad_rho, status):
    """islam_dense_ba_newton_vjp on what _dense_ba_newton_state prepared."""
    grad_depth, grad_flow = _dense_grad_outputs(a)
    check(lib().islam_dense_ba_newton_vjp(*a.head(), ptr(w), ptr(m), ptr(rho), a.kind, a.delta, ptr(lambda_p), ptr(grad_rho), ptr(status),
                                          ptr(grad_depth), ptr(grad_flow), a.B, a.H, a.W, stream_ptr(a.dev)))
    return grad_depth, grad_flow


class _DenseBARefineNewton(torch.autograd.Function):
    """dense_ba_refine (with prior_scale when given) whose refined motion and inv_depth carry the implicit-function gradient in depth and
    flow with the exact Hessian: backward is islam_dense_ba_newton_weights (two launches) and
    islam_dense_ba_newton_vjp at the refined state on the tensors forward prepared, and nothing else.  The start pose, the prior weight
    and the prior scale get no gradient."""

    @staticmethod
    def forward(ctx, depth, flow, mask, motion, intr, prior_weight, prior_scale, rgb2imu, kernel, iters, damping, min_count, trace_cap):
        a = _dense_reproj_args(depth, flow, mask, motion, intr, rgb2imu, kernel)
        w = _dense_ba_prior_weight(prior_weight, a.B, a.dev)
        m = _dense_ba_prior_scale(prior_scale, a, 'dense_ba_refine')
        out = _dense_ba_refine_launch(a, w, iters, damping, min_count, trace_cap, m)
        ctx.save_for_backward(a.depth, a.flow, a.mask, out.motion, out.inv_depth, out.status, a.intr, a.rgb2imu, w, m)
        ctx.kind, ctx.delta, ctx.dtypes = a.kind, a.delta, (depth.dtype, flow.dtype)
        ctx.mark_non_differentiable(*(t for t in out[2:] if t is not None))
        ctx.set_materialize_grads(False)          # an output the loss does not use arrives as None: no sums of u_cam for it
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_motion, grad_inv_depth, *unused):
        none = (None,) * 13
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return none
        depth, flow, mask, motion, rho, status, intr, rgb2imu, w, m = ctx.saved_tensors
        a = _DenseArgs(depth.device, *depth.shape, depth, flow, mask, motion, intr, rgb2imu, ctx.kind, ctx.delta)      # at the refined state
        grad_motion = torch.zeros_like(motion) if grad_motion is None else grad_motion.to(torch.float64).contiguous()
        if grad_inv_depth is not None:
            grad_inv_depth = grad_inv_depth.to(torch.float64).contiguous()
        nw = _dense_ba_newton_launch(a, w, m, rho, grad_motion, grad_inv_depth, status)
        grad_depth, grad_flow = _dense_ba_newton_vjp_launch(a, w, m, rho, nw.lambda_p, grad_inv_depth, nw.status)
        return (grad_depth.to(ctx.dtypes[0]) if ctx.needs_input_grad[0] else None,
                grad_flow.to(ctx.dtypes[1]) if ctx.needs_input_grad[1] else None) + none[2:]


# --------------------------------------------------------------------------- 3x3 convolution on the matrix cores
def deconv_to2(x, weight, bias, out=None, coff=0):
    """nn.ConvTranspose2d(C, 2, 4, 2, 1)(x) for fp32 NCHW tensors on islam_deconv4x4s2_to2_f32 (PWC-Net's deconv / upfeat layers), written
    into channels [coff, coff + 2) of ``out`` (B, ytot, 2H, 2W) (allocated with two channels when None)."""
    require_cuda(x, weight)
    B, C, H, W = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(weight.shape) == (C, 2, 4, 4) and weight.dtype == torch.float32
    if out is None:
        out = torch.empty((B, 2, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B and tuple(out.shape[2:]) == (2 * H, 2 * W)
    check(lib().islam_deconv4x4s2_to2_f32(ptr(x), ptr(weight.contiguous()), ptr(bias), ptr(out), int(out.shape[1]), int(coff), B, C, H, W,
                                          stream_ptr(x.device)))
    return out


def flow_head_up(x, wf, bf, wu=None, bu=None, up_out=None, up_coff=0):
    """(Conv2d(C, 2, 3, 1, 1)(x), ConvTranspose2d(C, 2, 4, 2, 1)(x)) -- PWC-Net's predict_flow and upfeat of one level -- in one pass over
    x (islam_flow_head_up_f32).  wf: the Conv2d weight re-laid out as [C][2][3][3] (``weight.permute(1, 0, 2, 3).contiguous()``);
    wu / bu: the ConvTranspose2d's weight (C,2,4,4) / bias, or None for the head alone (returns (flow, None))."""
    require_cuda(x, wf)
    B, C, H, W = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(wf.shape) == (C, 2, 3, 3) and wf.is_contiguous() and wf.dtype == torch.float32
    flow = torch.empty((B, 2, H, W), dtype=torch.float32, device=x.device)
    up = None
    if wu is not None:
        assert tuple(wu.shape) == (C, 2, 4, 4) and wu.dtype == torch.float32 and wu.is_contiguous()
        if up_out is not None:              # into channels [up_coff, up_coff + 2) of a larger (B, Ctot, 2H, 2W) tensor
            assert up_out.dtype == torch.float32 and up_out.is_contiguous() and up_out.shape[0] == B and tuple(up_out.shape[2:]) == (2 * H, 2 * W)
            up = up_out
        else:
            up, up_coff = torch.empty((B, 2, 2 * H, 2 * W), dtype=torch.float32, device=x.device), 0
    check(lib().islam_flow_head_up_f32(ptr(x), ptr(wf), ptr(bf), ptr(flow), ptr(wu), ptr(bu), ptr(up), int(up.shape[1]) if up is not None else 0,
                                       int(up_coff), B, C, H, W, stream_ptr(x.device)))
    return flow, up


def pack_pyramid_weight(w):
    """(Cout, Cin, 3, 3) fp32 -> bf16 [Cout][ceil(9 * SC / 32) * 32] with K index = (ky * 3 + kx) * SC + c, SC = 4 for Cin <= 4 else Cin,
    zero padded: the layout islam_flow_pyramid_level holds in registers (include/islam_hip.h)."""
    Cout, Cin = int(w.shape[0]), int(w.shape[1])
    assert tuple(w.shape[2:]) == (3, 3)
    SC = 4 if Cin <= 4 else Cin
    K = (9 * SC + 31) // 32 * 32
    p = torch.zeros((Cout, K), dtype=torch.bfloat16, device=w.device)
    t = torch.zeros((Cout, 9, SC), dtype=torch.bfloat16, device=w.device)
    t[:, :, :Cin] = w.detach().permute(0, 2, 3, 1).reshape(Cout, 9, Cin).to(torch.bfloat16)
    p[:, :9 * SC] = t.reshape(Cout, 9 * SC)
    assert p.numel() == lib().islam_pyramid_packed_elems(Cin, Cout)
    return p.contiguous()


def flow_pyramid_level(x, packed, biases, slope=0.1):
    """conv(k3, s2) + conv(k3) + conv(k3), each + bias + LeakyReLU(slope), of one pyramid level in one launch (fp32 NCHW in and out, bf16
    operands).  packed / biases: the three layers' pack_pyramid_weight tensors / fp32 biases.  Inference only."""
    require_cuda(x, *packed)
    B, Cin, H, W = x.shape
    C = int(biases[0].numel())
    assert x.dtype == torch.float32 and x.is_contiguous() and len(packed) == 3 and len(biases) == 3
    y = torch.empty((B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    check(lib().islam_flow_pyramid_level(ptr(x), ptr(packed[0]), ptr(biases[0]), ptr(packed[1]), ptr(biases[1]), ptr(packed[2]), ptr(biases[2]),
                                         ptr(y), B, Cin, H, W, C, float(slope), stream_ptr(x.device)))
    return y


def flow_pyramid_level_pair(x, packed, biases, slope=0.1):
    """flow_pyramid_level (level 1: 3 -> 16 channels) on the two frames of a pair tensor x (B, 6, H, W) fp32: the result for
    torch.cat((x[:, :3], x[:, 3:]), 0) -- (2 B, 16, H/2, W/2), first frames first -- without that copy."""
    require_cuda(x, *packed)
    B, C6, H, W = x.shape
    assert C6 == 6 and x.dtype == torch.float32 and x.is_contiguous() and len(packed) == 3 and int(biases[0].numel()) == 16
    y = torch.empty((2 * B, 16, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    check(lib().islam_flow_pyramid_level_pair(ptr(x), ptr(packed[0]), ptr(biases[0]), ptr(packed[1]), ptr(biases[1]), ptr(packed[2]),
                                              ptr(biases[2]), ptr(y), B, H, W, float(slope), stream_ptr(x.device)))
    return y


def pack_conv3x3_weight(w):
    """(Cout, Cin, 3, 3) fp32 -> bf16 [9][CoutP][CinP] (tap-major, zero padded), the layout islam_conv3x3_mfma stages.
    The kernel walks the input channels in chunks of 16; when Cin > 16 is not a multiple of 16 its last chunk reads the LAST
    16 channels of the tensor (all exist), so that chunk's 16 weight slots hold channels Cin-16 .. Cin-1, zero for the ones
    the previous chunk already covered (include/islam_hip.h, islam_conv3x3_mfma)."""
    Cout, Cin = int(w.shape[0]), int(w.shape[1])
    assert tuple(w.shape[2:]) == (3, 3)
    CinP, CoutP = (Cin + 15) // 16 * 16, (Cout + 63) // 64 * 64
    p = torch.zeros((9, CoutP, CinP), dtype=torch.bfloat16, device=w.device)
    wt = w.detach().permute(2, 3, 0, 1).reshape(9, Cout, Cin).to(torch.bfloat16)
    full = Cin // 16 * 16
    if Cin == full or Cin < 16:
        p[:, :Cout, :Cin] = wt
    else:
        p[:, :Cout, :full] = wt[:, :, :full]
        p[:, :Cout, CinP - (Cin - full):] = wt[:, :, full:]
    assert p.numel() == lib().islam_conv3x3_packed_elems(Cin, Cout)
    return p.contiguous()


def conv3x3_mfma(x, packed, bias, cout, stride=1, dilation=1, slope=0.1, out=None, coff=0, xoff=0, cin=None):
    """y = LeakyReLU_slope(conv3x3(x[:, xoff:xoff+cin]) + bias) with padding = dilation (slope=1.0: linear).
    ``out`` (B, Ctot, Ho, Wo) fp32: the result goes to channels [coff, coff+cout); with ``xoff`` the input is a channel slice
    of a larger buffer -- together a DenseNet block needs no torch.cat.  Inference only (no autograd)."""
    require_cuda(x, packed)
    assert x.dtype == torch.float32 and x.is_contiguous()
    B, xtot, H, W = x.shape
    cin = xtot - xoff if cin is None else cin
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] == B and tuple(out.shape[2:]) == (Ho, Wo)
    check(lib().islam_conv3x3_mfma(ptr(x), ptr(packed), ptr(bias), ptr(out), B, int(cin), H, W, int(cout), int(stride), int(dilation),
                                   int(xoff), int(xtot), int(coff), int(out.shape[1]), ctypes.c_float(slope), stream_ptr(x.device)))
    return out


def pack_conv_nhwc_weight(w):
    """(Cout, Cin, k, k) -> bf16 [k*k][CoutP][CinP] (tap-major, zero padded; CoutP = Cout up to 64s, CinP = Cin up to 32s), the
    layout islam_conv_nhwc_bf16 stages."""
    Cout, Cin, k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    assert w.shape[2] == w.shape[3] and k in (1, 2, 3)
    CinP, CoutP = (Cin + 31) // 32 * 32, (Cout + 63) // 64 * 64
    p = torch.zeros((k * k, CoutP, CinP), dtype=torch.bfloat16, device=w.device)
    p[:, :Cout, :Cin] = w.detach().permute(2, 3, 0, 1).reshape(k * k, Cout, Cin).to(torch.bfloat16)
    assert p.numel() == lib().islam_conv_nhwc_packed_elems(Cin, Cout, k)
    return p.contiguous()


def conv_nhwc(x, packed, cout, ksize, in_affine=None, bias=None, res=None, relu=False, stats=False, in_relu=False):
    """Channels-last bf16 convolution (k = 1 or 3, stride 1, "same" padding) on islam_conv_nhwc_bf16.  x: (B,Cin,H,W) bf16
    channels_last.  in_affine (2*Cin fp32): the producer's BatchNorm scale | shift, applied with a ReLU while x is staged.
    stats=True: returns (y, folded) with folded = the [256][2][cout] partial sums of the raw output for bn_finalize.
    in_relu: ReLU of the input while it is staged (no separate pass over x)."""
    require_cuda(x, packed)
    B, Cin, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    y = torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    st = None
    if stats:
        st = torch.empty(lib().islam_conv_nhwc_stats_floats(B, H, W, cout), dtype=torch.float32, device=x.device)
    if res is not None:
        assert res.shape == y.shape and res.dtype == torch.bfloat16 and res.is_contiguous(memory_format=torch.channels_last)
    check(lib().islam_conv_nhwc_bf16(ptr(x), ptr(packed), ptr(in_affine), ptr(bias), ptr(res), ptr(y), ptr(st), B, Cin, H, W, int(cout),
                                     int(ksize), int(bool(relu)) | (2 if in_relu else 0), stream_ptr(x.device)))
    if stats:
        return y, st[st.numel() - 256 * 2 * cout:]
    return y


def conv_nhwc_s2(x, packed, cout, ksize, in_affine=None, bias=None, res=None, relu=False, stats=False, in_relu=False, out_hw=None, x2=None):
    """conv_nhwc at stride 2 with padding ksize // 2 (islam_conv_nhwc_bf16_s2; ksize 1, 2 or 3).  out_hw: fewer output rows / columns than
    the convolution has (the quarter-resolution tail keeps (H/2, W/2) of (H/2 + 1, W/2 + 1)).  x2 (ksize 2, bias / ReLU only): the input is
    torch.cat((x, x2), 1) read from the two tensors where they lie (islam_conv_nhwc_bf16_s2_cat; x.shape[1] % 16 == 0)."""
    require_cuda(x, packed, x2)
    B, Cin, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    P = ksize // 2
    Ho, Wo = ((H + 2 * P - ksize) // 2 + 1, (W + 2 * P - ksize) // 2 + 1) if out_hw is None else out_hw
    y = torch.empty((B, cout, Ho, Wo), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    if x2 is not None:
        assert in_affine is None and res is None and not stats and ksize == 2
        assert x2.dtype == torch.bfloat16 and x2.is_contiguous(memory_format=torch.channels_last) and x2.shape[0] == B and tuple(x2.shape[2:]) == (H, W)
        check(lib().islam_conv_nhwc_bf16_s2_cat(ptr(x), Cin, ptr(x2), int(x2.shape[1]), ptr(packed), ptr(bias), ptr(y), B, H, W, int(cout), Ho, Wo,
                                                int(ksize), int(bool(relu)) | (2 if in_relu else 0), stream_ptr(x.device)))
        return y
    st = None
    if stats:
        st = torch.empty(lib().islam_conv_nhwc_s2_stats_floats(B, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    if res is not None:
        assert res.shape == y.shape and res.dtype == torch.bfloat16 and res.is_contiguous(memory_format=torch.channels_last)
    check(lib().islam_conv_nhwc_bf16_s2(ptr(x), ptr(packed), ptr(in_affine), ptr(bias), ptr(res), ptr(y), ptr(st), B, Cin, H, W, int(cout), Ho, Wo,
                                        int(ksize), int(bool(relu)) | (2 if in_relu else 0), stream_ptr(x.device)))
    if stats:
        return y, st[st.numel() - 256 * 2 * cout:]
    return y


def conv_nhwc_into(x, packed, cout, ksize, out, yoff, in_affine=None, bias=None, relu=False, in_relu=False):
    """conv_nhwc with the result written into out[:, yoff:yoff+cout] of a larger channels-last bf16 tensor (a concatenation under
    construction; islam_conv_nhwc_bf16_into).  Returns ``out``."""
    require_cuda(x, packed, out)
    B, Cin, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    assert out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last) and out.shape[0] == B
    assert tuple(out.shape[2:]) == (H, W)
    check(lib().islam_conv_nhwc_bf16_into(ptr(x), ptr(packed), ptr(in_affine), ptr(bias), ptr(out), int(out.shape[1]), int(yoff), B, Cin, H, W,
                                          int(cout), int(ksize), int(bool(relu)) | (2 if in_relu else 0), stream_ptr(x.device)))
    return out


_BN_COUNTERS = {}


def _bn_counter(device):
    """A zero-initialised int32 slot for islam_conv_nhwc_bf16_bn's ticket (one ring of 256 per device: two launches that could run at
    the same time -- two streams, two nodes of a captured graph -- never share a slot; the kernel leaves its slot at zero)."""
    key = (device.type, device.index)
    hit = _BN_COUNTERS.get(key)
    if hit is None:
        hit = _BN_COUNTERS[key] = [torch.zeros(256 * 32, dtype=torch.int32, device=device), 0]      # one 128-byte line per slot
    hit[1] = (hit[1] + 1) % 256
    return hit[0][hit[1] * 32:]


def conv_nhwc_bn(x, packed, cout, ksize, bn, in_affine=None, in_relu=False):
    """conv_nhwc(..., stats=True) followed by bn_finalize as two launches instead of three (islam_conv_nhwc_bf16_bn): returns
    (raw output, [scale | shift] of the train-mode BatchNorm ``bn``, whose running statistics are updated).  Same bits."""
    require_cuda(x, packed)
    B, Cin, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last) and bn.num_features == cout
    y = torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    st = torch.empty(lib().islam_conv_nhwc_stats_floats(B, H, W, cout), dtype=torch.float32, device=x.device)
    out = torch.empty(2 * cout, dtype=torch.float32, device=x.device)
    track = bn.track_running_stats and bn.running_mean is not None
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    check(lib().islam_conv_nhwc_bf16_bn(ptr(x), ptr(packed), ptr(in_affine), ptr(y), ptr(st), B, Cin, H, W, int(cout), int(ksize),
                                        int(bool(in_relu)), ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean) if track else None,
                                        ptr(bn.running_var) if track else None, ptr(bn.num_batches_tracked) if track else None,
                                        c_double(mom), c_double(float(bn.eps)), ptr(out), ptr(_bn_counter(x.device)),
                                        stream_ptr(x.device)))
    return y, out


def pack_hg_residual(w1, w2, w3):
    """Weights of one hourglass Residual (hourglass.py:28-40: conv1 (h,Cin,1,1), conv2 (h,h,3,3), conv3 (Cout,h,1,1)) as the MFMA A
    fragments islam_hg_residual_nhwc_bf16 loads (1 KiB each: 64 lanes x 8 bf16), in the order its waves consume them
    (csrc/hourglass.hip)."""
    h, Cin, Cout = int(w1.shape[0]), int(w1.shape[1]), int(w3.shape[0])
    assert tuple(w2.shape) == (h, h, 3, 3) and int(w3.shape[1]) == h and Cout == 2 * h and h % 32 == 0 and Cin % 64 == 0
    MT = h // 32
    dev = w1.device
    bf = torch.bfloat16
    W1, W3 = w1.detach().reshape(h, Cin), w3.detach().reshape(Cout, h)
    W2 = w2.detach()
    # one MFMA A fragment = [64 lanes][8] bf16: lane (li = lane & 31, kg = lane >> 5) holds row r0 + li, columns k0 + 8 kg ... + 8
    li = torch.arange(64, device=dev) & 31
    kk = (torch.arange(64, device=dev) >> 5)[:, None] * 8 + torch.arange(8, device=dev)[None, :]      # (64, 8): 8 kg + j
    frag = lambda M, r0, k0: M[(r0 + li)[:, None], k0 + kk]
    if Cin == 64 and Cout == 64:
        # hg_residual64_kernel keeps the module's weights in registers: 26 fragments
        fr = [frag(W1, 0, 16 * ks) for ks in range(4)]
        fr += [frag(W2[:, :, t // 3, t % 3], 0, 16 * ks) for t in range(9) for ks in range(2)]
        fr += [frag(W3, 32 * a, 16 * ks) for a in range(2) for ks in range(2)]
    else:
        # hg_residual_kernel: every wave streams the fragments of ITS output-channel tile in consumption order
        fr = [frag(W1, 32 * mg, 16 * ks) for mg in range(MT) for ks in range(Cin // 16)]
        fr += [frag(W2[:, :, t // 3, t % 3], 32 * mg, 32 * c + 16 * ks) for mg in range(MT) for c in range(MT) for t in range(9) for ks in range(2)]
        fr += [frag(W3, 32 * m3, 16 * ks) for m3 in range(2 * MT) for ks in range(h // 16)]
    packed = torch.stack(fr).to(bf).reshape(-1).contiguous()
    assert packed.numel() == lib().islam_hg_residual_packed_elems(Cin, Cout), (packed.numel(), Cin, Cout)
    return packed


def hg_residual(x, packed, bias32, cout, res=None):
    """conv3(relu(conv2(relu(conv1(relu(x)))))) + res of a channels-last bf16 tensor in one launch (islam_hg_residual_nhwc_bf16);
    res = x when None (needs Cin == cout).  bias32 = cat(b1, b2, b3) fp32."""
    require_cuda(x, packed)
    B, Cin, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last) and bias32.dtype == torch.float32
    assert bias32.numel() == 2 * cout
    if res is None:
        assert Cin == cout
        res = x
    y = torch.empty((B, cout, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    assert res.shape == y.shape and res.dtype == torch.bfloat16 and res.is_contiguous(memory_format=torch.channels_last)
    check(lib().islam_hg_residual_nhwc_bf16(ptr(x), ptr(res), ptr(y), ptr(packed), ptr(bias32), B, Cin, H, W, int(cout), stream_ptr(x.device)))
    return y


def pack_deconv_nhwc_weight(w):
    """ConvTranspose2d weight (Cin, Cout, 4, 4) -> bf16 [4 classes][4 taps][CoutP][CinP] for islam_deconv4x4s2_nhwc_bf16: output parity
    class (a, c), tap (r, s) of its 2x2 convolution = W[:, :, 3 - 2r - a, 3 - 2s - c] (stride 2, padding 1)."""
    Cin, Cout = int(w.shape[0]), int(w.shape[1])
    assert tuple(w.shape[2:]) == (4, 4)
    CinP, CoutP = (Cin + 31) // 32 * 32, (Cout + 63) // 64 * 64
    p = torch.zeros((4, 4, CoutP, CinP), dtype=torch.bfloat16, device=w.device)
    wt = w.detach().permute(2, 3, 1, 0).to(torch.bfloat16)            # (ky, kx, Cout, Cin)
    for a in range(2):
        for c in range(2):
            for r in range(2):
                for s_ in range(2):
                    p[a * 2 + c, r * 2 + s_, :Cout, :Cin] = wt[3 - 2 * r - a, 3 - 2 * s_ - c]
    assert p.numel() == lib().islam_deconv_nhwc_packed_elems(Cin, Cout)
    return p.contiguous()


def deconv_nhwc(x, packed, bias32, cout, out=None, yoff=0, relu=False, x2=None):
    """act(ConvTranspose2d(k=4, s=2, p=1)(x) + bias) of a channels-last bf16 tensor on islam_deconv4x4s2_nhwc_bf16, written into
    channels [yoff, yoff + cout) of ``out`` (B, ytot, 2H, 2W) channels_last bf16 (allocated dense when None).  x2: the layer's input is
    torch.cat((x, x2), 1), read from the two tensors where they lie (islam_deconv4x4s2_nhwc_bf16_cat; x.shape[1] % 32 == 0)."""
    require_cuda(x, packed, x2)
    B, Cin, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last) and bias32.dtype == torch.float32
    if out is None:
        out = torch.empty((B, cout, 2 * H, 2 * W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    assert out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last)
    assert out.shape[0] == B and tuple(out.shape[2:]) == (2 * H, 2 * W)
    if x2 is not None:
        assert x2.dtype == torch.bfloat16 and x2.is_contiguous(memory_format=torch.channels_last) and x2.shape[0] == B and tuple(x2.shape[2:]) == (H, W)
        check(lib().islam_deconv4x4s2_nhwc_bf16_cat(ptr(x), Cin, ptr(x2), int(x2.shape[1]), ptr(packed), ptr(bias32), ptr(out), int(out.shape[1]),
                                                    int(yoff), B, H, W, int(cout), int(bool(relu)), stream_ptr(x.device)))
        return out
    check(lib().islam_deconv4x4s2_nhwc_bf16(ptr(x), ptr(packed), ptr(bias32), ptr(out), int(out.shape[1]), int(yoff), B, Cin, H, W, int(cout),
                                            int(bool(relu)), stream_ptr(x.device)))
    return out


def bn_finalize(folded, bn, count):
    """[256][2][C] partial sums -> (2*C) fp32 [scale | shift] of a train-mode nn.BatchNorm2d; its running statistics are
    updated like nn.BatchNorm2d would (islam_bn_finalize)."""
    C = bn.num_features
    out = torch.empty(2 * C, dtype=torch.float32, device=folded.device)
    track = bn.track_running_stats and bn.running_mean is not None
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    check(lib().islam_bn_finalize(ptr(folded), c_double(float(count)), ptr(bn.weight), ptr(bn.bias),
                                  ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None,
                                  ptr(bn.num_batches_tracked) if track else None, c_double(mom), c_double(float(bn.eps)), C, ptr(out),
                                  stream_ptr(folded.device)))
    return out


def bn_apply_(x, scale_shift, relu=False, res=None):
    """In place on a channels-last bf16 tensor: x <- act(bf16(x*scale[c] + shift[c]) [+ res]) (islam_bn_apply_nhwc_bf16)."""
    B, C, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    if res is not None:
        assert res.shape == x.shape and res.dtype == torch.bfloat16 and res.is_contiguous(memory_format=torch.channels_last)
    check(lib().islam_bn_apply_nhwc_bf16(ptr(x), ptr(x), ptr(res), ptr(scale_shift), int(bool(relu)), ctypes.c_longlong(B * H * W), C,
                                         stream_ptr(x.device)))
    return x


def resize_bilinear(x, size, align_corners=False):
    """F.interpolate(x, size, mode='bilinear', align_corners=...) -- on the HIP kernel for channels-last bf16 inference
    tensors (the frozen stereo net's execution copy), through torch otherwise."""
    Ho, Wo = int(size[0]), int(size[1])
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] % 8 == 0 and not x.requires_grad
            and x.is_contiguous(memory_format=torch.channels_last)):
        B, C, Hi, Wi = x.shape
        y = torch.empty((B, C, Ho, Wo), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
        check(lib().islam_resize_bilinear_nhwc_bf16(ptr(x), ptr(y), B, C, Hi, Wi, Ho, Wo, int(bool(align_corners)),
                                                    stream_ptr(x.device)))
        return y
    return torch.nn.functional.interpolate(x, [Ho, Wo], mode='bilinear', align_corners=align_corners)


def resize_bilinear_into(x, out, coff, align_corners=False):
    """Bilinear resize of a channels-last bf16 tensor to out's spatial size, written into out[:, coff:coff+C] (out: channels-last
    bf16 with a multiple of 8 channels; coff a multiple of 8).  islam_resize_bilinear_nhwc_bf16_into."""
    B, C, Hi, Wi = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    assert out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last) and out.shape[0] == B
    check(lib().islam_resize_bilinear_nhwc_bf16_into(ptr(x), ptr(out), B, C, Hi, Wi, int(out.shape[2]), int(out.shape[3]),
                                                     int(bool(align_corners)), int(out.shape[1]), int(coff), stream_ptr(x.device)))
    return out


def stack_pair_pad8(x):
    """(B, 2c, H, W) channels-last bf16 stereo pair -> (2B, 8, H, W): left images, then right images, channels [c, 8) zero
    (islam_stack_pair_pad8_nhwc_bf16)."""
    B, C2, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last) and C2 % 2 == 0 and C2 <= 16
    y = torch.empty((2 * B, 8, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    check(lib().islam_stack_pair_pad8_nhwc_bf16(ptr(x), ptr(y), B, C2, H, W, stream_ptr(x.device)))
    return y


def stereo_pair_prepare(left, right):
    """The stereo pair (two fp32 (B,c,H,W) tensors, c <= 4) as the frozen stereo net's execution copy reads it, in one pass
    (islam_stereo_pair_prepare_f32): (x6, xs) with x6 = torch.cat((left, right), 1).to(bfloat16) channels-last and xs = stack_pair_pad8(x6)."""
    require_cuda(left, right)
    B, c, H, W = left.shape
    assert left.dtype == torch.float32 and right.dtype == torch.float32 and left.shape == right.shape and c <= 4
    assert left.is_contiguous() and right.is_contiguous()
    x6 = torch.empty((B, 2 * c, H, W), dtype=torch.bfloat16, device=left.device, memory_format=torch.channels_last)
    xs = torch.empty((2 * B, 8, H, W), dtype=torch.bfloat16, device=left.device, memory_format=torch.channels_last)
    check(lib().islam_stereo_pair_prepare_f32(ptr(left), ptr(right), ptr(x6), ptr(xs), B, c, H, W, stream_ptr(left.device)))
    return x6, xs


def upsample_cat(pieces, size, tail=None, align_corners=False):
    """torch.cat([F.interpolate(p, size, mode='bilinear') for p in pieces] + [tail], 1) for channels-last bf16 pieces of one shape
    (B, C_k, Hi, Wi), C_k multiples of 8, at most 8 of them; tail: (B, C_t, *size) or None.  One launch
    (islam_upsample_cat_nhwc_bf16); every value is the one resize_bilinear produces."""
    import ctypes
    B, _, Hi, Wi = pieces[0].shape
    Ho, Wo = int(size[0]), int(size[1])
    for t in pieces:
        assert t.dtype == torch.bfloat16 and t.is_contiguous(memory_format=torch.channels_last) and t.shape[0] == B and tuple(t.shape[2:]) == (Hi, Wi)
        assert t.shape[1] % 8 == 0
    ct = 0
    if tail is not None:
        assert tail.dtype == torch.bfloat16 and tail.is_contiguous(memory_format=torch.channels_last) and tuple(tail.shape[2:]) == (Ho, Wo)
        assert tail.shape[0] == B and tail.shape[1] % 8 == 0
        ct = int(tail.shape[1])
    n = len(pieces)
    assert 1 <= n <= 8
    out = torch.empty((B, sum(int(t.shape[1]) for t in pieces) + ct, Ho, Wo), dtype=torch.bfloat16, device=pieces[0].device,
                      memory_format=torch.channels_last)
    srcs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in pieces])
    chans = (ctypes.c_int * n)(*[int(t.shape[1]) for t in pieces])
    check(lib().islam_upsample_cat_nhwc_bf16(srcs, chans, n, ptr(tail) if tail is not None else None, ct, ptr(out), B, Hi, Wi, Ho, Wo,
                                             int(bool(align_corners)), stream_ptr(out.device)))
    return out


def nchw_to_nhwc_mirror(src, soff, C, dst, doff):
    """fp32 NCHW channels [soff, soff+C) of ``src`` -> bf16 channels [doff, doff+C) of the channels-last tensor ``dst`` (a
    (B, Ctot, H, W) bf16 tensor in torch.channels_last memory format); the channels up to the next multiple of 8 are zeroed."""
    B, stot, H, W = src.shape
    assert src.dtype == torch.float32 and src.is_contiguous() and dst.dtype == torch.bfloat16
    assert dst.is_contiguous(memory_format=torch.channels_last) and dst.shape[0] == B and tuple(dst.shape[2:]) == (H, W)
    check(lib().islam_nchw_f32_to_nhwc_bf16(ptr(src), stot, int(soff), ptr(dst), int(dst.shape[1]), int(doff), B, int(C), H, W,
                                            stream_ptr(src.device)))
    return dst


def conv_nhwc_flow(xm, xoff, cin, packed, bias, y32, coff, cout, slope, ymir=None, moff=0, dilation=1):
    """islam_conv_nhwc_flow: act(conv3x3(xm[:, xoff:xoff+cin], dilation) + bias) -> y32[:, coff:coff+cout] (fp32 NCHW, may be None)
    and / or ymir[:, moff:moff+cout] (bf16 channels-last mirror).  xm / ymir: bf16 tensors in torch.channels_last memory format."""
    B, xtot, H, W = xm.shape
    assert xm.dtype == torch.bfloat16 and xm.is_contiguous(memory_format=torch.channels_last)
    assert y32 is not None or ymir is not None
    if y32 is not None:
        assert y32.dtype == torch.float32 and y32.is_contiguous() and tuple(y32.shape[2:]) == (H, W) and y32.shape[0] == B
    assert packed.dtype == torch.bfloat16 and packed.numel() == lib().islam_conv_nhwc_packed_elems(int(cin), int(cout), 3)
    if ymir is not None:
        assert ymir.dtype == torch.bfloat16 and ymir.is_contiguous(memory_format=torch.channels_last) and ymir.shape[0] == B
        assert tuple(ymir.shape[2:]) == (H, W)
    check(lib().islam_conv_nhwc_flow(ptr(xm), int(xtot), int(xoff), int(cin), ptr(packed), ptr(bias), ptr(y32),
                                     int(y32.shape[1]) if y32 is not None else 0, int(coff), ptr(ymir),
                                     int(ymir.shape[1]) if ymir is not None else 0, int(moff), B, H, W, int(cout), int(dilation),
                                     c_float(slope), stream_ptr(xm.device)))
    return y32 if y32 is not None else ymir


def resize_bilinear_add(x, add, align_corners=False, out=None, coff=0):
    """add + F.interpolate(x, add's size, mode='bilinear') in one pass over channels-last bf16 tensors
    (islam_resize_bilinear_add_nhwc_bf16: the hourglass's `up1 + up2(low)`).  ``out``: write into out[:, coff:coff+C] of a larger
    channels-last bf16 tensor (a concatenation under construction) and return ``out``."""
    B, C, Hi, Wi = x.shape
    assert fusable_nhwc_bf16(x, C) and fusable_nhwc_bf16(add, C) and add.shape[:2] == x.shape[:2]
    if out is not None:
        assert out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last) and out.shape[0] == B
        assert tuple(out.shape[2:]) == tuple(add.shape[2:])
        check(lib().islam_resize_bilinear_add_nhwc_bf16_into(ptr(x), ptr(add), ptr(out), B, C, Hi, Wi, int(add.shape[2]), int(add.shape[3]),
                                                             int(bool(align_corners)), int(out.shape[1]), int(coff), stream_ptr(x.device)))
        return out
    y = torch.empty_like(add)
    check(lib().islam_resize_bilinear_add_nhwc_bf16(ptr(x), ptr(add), ptr(y), B, C, Hi, Wi, int(add.shape[2]), int(add.shape[3]),
                                                    int(bool(align_corners)), stream_ptr(x.device)))
    return y


def half_image_into(x, out, yoff):
    """F.interpolate(x, scale_factor=0.5, mode='bilinear') of a channels-last bf16 image with at most 8 channels, written (zero padded to
    8 channels) into out[:, yoff:yoff+8] of a larger channels-last bf16 tensor (islam_half_image_into_nhwc_bf16).  Returns ``out``."""
    require_cuda(x, out)
    B, C, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    assert out.dtype == torch.bfloat16 and out.is_contiguous(memory_format=torch.channels_last)
    assert tuple(out.shape[2:]) == (H // 2, W // 2) and out.shape[0] == B
    check(lib().islam_half_image_into_nhwc_bf16(ptr(x), ptr(out), int(out.shape[1]), int(yoff), B, C, H, W, stream_ptr(x.device)))
    return out


def maxpool2(x, relu=False):
    """F.max_pool2d([relu](x), 2): islam_maxpool2_nhwc_bf16 for channels-last bf16 inference tensors, torch otherwise."""
    if fusable_nhwc_bf16(x, x.shape[1]) and x.shape[2] >= 2 and x.shape[3] >= 2:
        B, C, H, W = x.shape
        y = torch.empty((B, C, H // 2, W // 2), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
        check(lib().islam_maxpool2_nhwc_bf16(ptr(x), ptr(y), B, C, H, W, int(bool(relu)), stream_ptr(x.device)))
        return y
    return torch.nn.functional.max_pool2d(torch.relu(x) if relu else x, kernel_size=2)


def avgpool(x, k):
    """AvgPool2d((k, k), stride=(k, k)) of a channels-last bf16 inference tensor (islam_avgpool_nhwc_bf16)."""
    B, C, H, W = x.shape
    assert fusable_nhwc_bf16(x, C) and H >= k and W >= k
    y = torch.empty((B, C, H // k, W // k), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
    check(lib().islam_avgpool_nhwc_bf16(ptr(x), ptr(y), B, C, H, W, int(k), stream_ptr(x.device)))
    return y


def fusable_nhwc_bf16(x, channels):
    """True for the tensors the channels-last bf16 epilogue / resize kernels take (frozen execution copies, no autograd)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and channels % 8 == 0 and not x.requires_grad
            and x.is_contiguous(memory_format=torch.channels_last))


def bias_act_add_(y, bias32, res=None, relu=False):
    """In place on a channels-last bf16 conv output: y <- act(bf16(y + bias) [+ res]) (islam_bias_act_add_nhwc_bf16)."""
    B, C, H, W = y.shape
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last) and bias32.dtype == torch.float32
    if res is not None:
        assert res.shape == y.shape and res.dtype == torch.bfloat16 and res.is_contiguous(memory_format=torch.channels_last)
    check(lib().islam_bias_act_add_nhwc_bf16(ptr(y), ptr(bias32), ptr(res), ctypes.c_longlong(B * H * W), C, int(bool(relu)),
                                             stream_ptr(y.device)))
    return y


class _BiasActF32(torch.autograd.Function):
    """y = act(x + bias[c] (+ res)) on fp32 channels-last conv outputs, one launch each way (islam_bias_act_f32_nhwc /
    islam_bias_act_bwd_f32_nhwc): the elementwise tail of the trainable pose head's convolutions (Network/VOFlowNet.py:42-157)."""

    @staticmethod
    def forward(ctx, x, bias, res, relu):
        B, C, H, W = x.shape
        y = torch.empty_like(x, memory_format=torch.channels_last)
        check(lib().islam_bias_act_f32_nhwc(ptr(x), ptr(bias), ptr(res), ptr(y), ctypes.c_longlong(B * H * W), C, int(bool(relu)),
                                            stream_ptr(x.device)))
        ctx.relu, ctx.has_res = bool(relu), res is not None
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        B, C, H, W = y.shape
        gy = gy.contiguous(memory_format=torch.channels_last)
        gx = torch.empty_like(gy, memory_format=torch.channels_last)
        gb = torch.empty(C, dtype=torch.float32, device=y.device)
        npix = B * H * W
        scratch = torch.empty(int(lib().islam_bias_act_bwd_scratch_floats(ctypes.c_longlong(npix), C)), dtype=torch.float32, device=y.device)
        check(lib().islam_bias_act_bwd_f32_nhwc(ptr(gy), ptr(y), ptr(gx), ptr(gb), ptr(scratch), ptr(_ticket(y.device)),
                                                ctypes.c_longlong(npix), C, int(ctx.relu), stream_ptr(y.device)))
        return gx, gb, (gx if ctx.has_res else None), None


_TICKETS = {}


def _ticket(device):
    """One zero-initialised word per device for the kernels that fold partial sums in their last workgroup (they leave it at zero;
    launches on one stream are ordered, so they can share it)."""
    t = _TICKETS.get(device)
    if t is None:
        t = _TICKETS[device] = torch.zeros(4, dtype=torch.int32, device=device)
    return t


def bias_act(x, bias, res=None, relu=True):
    """act(x + bias[c] (+ res)) for an fp32 channels-last conv output, differentiable w.r.t. x, bias and res."""
    assert x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and x.shape[1] % 4 == 0
    if res is not None:
        assert res.shape == x.shape and res.dtype == torch.float32 and res.is_contiguous(memory_format=torch.channels_last)
    return _BiasActF32.apply(x, bias, res, relu)


def bn_train_(x, bn, relu=False, res=None):
    """nn.BatchNorm2d in training mode on a channels-last bf16 conv output, IN PLACE, with the ReLU and / or residual add
    that follows it folded in (islam_bn_train_nhwc_bf16).  ``bn``: the fp32 BatchNorm2d module (weight, bias, running
    statistics, momentum, eps); its buffers are updated like nn.BatchNorm2d would."""
    B, C, H, W = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
    if res is not None:
        assert res.shape == x.shape and res.dtype == torch.bfloat16 and res.is_contiguous(memory_format=torch.channels_last)
    scratch = torch.empty(lib().islam_bn_scratch_floats(C), dtype=torch.float32, device=x.device)
    track = bn.track_running_stats and bn.running_mean is not None
    mom = 0.1 if bn.momentum is None else float(bn.momentum)
    check(lib().islam_bn_train_nhwc_bf16(ptr(x), ptr(x), ptr(res), ptr(bn.weight), ptr(bn.bias),
                                         ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None,
                                         ptr(bn.num_batches_tracked) if track else None, c_double(mom), c_double(bn.eps),
                                         int(bool(relu)), ctypes.c_longlong(B * H * W), C, ptr(scratch), stream_ptr(x.device)))
    return x


# --------------------------------------------------------------------------- IMU
def _dtype_code(dtype):
    """ISLAM_F32 / ISLAM_F64 of include/islam_hip.h; KeyError for any other dtype"""
    return {torch.float32: 0, torch.float64: 1}[dtype]


def _imu_preint_raw(dt, gyro, acc, seg, seg_host, init_pos, init_rot, init_vel, gravity, motion_mode):
    require_cuda(dt, gyro, acc, seg)
    dtype = dt.dtype
    code = _dtype_code(dtype)
    dev = dt.device
    nframes = int(seg_host.shape[0]) - 1
    S = int(dt.shape[0])
    maxF = int(np.max(np.diff(seg_host))) if nframes > 0 else 0
    rows = nframes if motion_mode else nframes + 1
    pos = torch.empty((rows, 3), dtype=dtype, device=dev)
    rot = torch.empty((rows, 4), dtype=dtype, device=dev)
    vel = torch.empty((rows, 3), dtype=dtype, device=dev)
    nbytes = lib().islam_imu_scratch_bytes(S, nframes, code)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().islam_imu_preint(ptr(dt), ptr(gyro), ptr(acc), ptr(seg), nframes, S, maxF, ptr(init_pos), ptr(init_rot),
                                 ptr(init_vel), c_double(gravity), 1 if motion_mode else 0, ptr(pos), ptr(rot), ptr(vel),
                                 ptr(scratch), code, stream_ptr(dev)))
    return pos, rot, vel, scratch


def imu_preint_both(dt, gyro, acc, seg, seg_host, init_pos, init_rot, init_vel, gravity):
    """World-mode and motion-mode outputs of one frame range from ONE pass (islam_imu_preint_both): ((pos, rot, vel) with
    nframes + 1 rows, (pos, rot, vel) with nframes rows), bit-identical to two imu_preint calls.  Forward values only."""
    require_cuda(dt, gyro, acc, seg)
    dtype = dt.dtype
    code = _dtype_code(dtype)
    dev = dt.device
    nframes = int(seg_host.shape[0]) - 1
    S = int(dt.shape[0])
    maxF = int(np.max(np.diff(seg_host))) if nframes > 0 else 0
    # one allocation for the six outputs: [world pos | rot | vel | motion pos | rot | vel], 10 columns per row
    out = torch.empty((2 * nframes + 1) * 10, dtype=dtype, device=dev)
    w, m = nframes + 1, nframes
    views, o = [], 0
    for rows, cols in ((w, 3), (w, 4), (w, 3), (m, 3), (m, 4), (m, 3)):
        views.append(out[o:o + rows * cols].view(rows, cols))
        o += rows * cols
    nbytes = lib().islam_imu_scratch_bytes(S, nframes, code)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(lib().islam_imu_preint_both(ptr(dt), ptr(gyro), ptr(acc), ptr(seg), nframes, S, maxF, ptr(init_pos), ptr(init_rot),
                                      ptr(init_vel), c_double(gravity), *[ptr(v) for v in views], ptr(scratch), code, stream_ptr(dev)))
    return tuple(views[:3]), tuple(views[3:]), out


class _ImuPreint(torch.autograd.Function):
    """islam_imu_preint with islam_imu_preint_bwd: gradients w.r.t. the gyro / accelerometer samples (the denoiser's outputs
    in the IMU-target epoch).  The gradient of the quaternion output is read in PyPose's convention (left tangent, padded)."""

    @staticmethod
    def forward(ctx, gyro, acc, dt, seg, seg_host, init_pos, init_rot, init_vel, gravity, motion_mode):
        pos, rot, vel, scratch = _imu_preint_raw(dt, gyro, acc, seg, seg_host, init_pos, init_rot, init_vel, gravity, motion_mode)
        ctx.save_for_backward(gyro, acc, dt, seg, scratch)
        ctx.meta = (int(seg_host.shape[0]) - 1, float(gravity), bool(motion_mode))
        return pos, rot, vel

    @staticmethod
    def backward(ctx, g_pos, g_rot, g_vel):
        gyro, acc, dt, seg, scratch = ctx.saved_tensors
        nframes, gravity, motion = ctx.meta
        code = _dtype_code(dt.dtype)
        c = lambda g: None if g is None else g.to(dt.dtype).contiguous()
        g_pos, g_rot, g_vel = c(g_pos), c(g_rot), c(g_vel)
        g_gyro, g_acc = torch.zeros_like(gyro), torch.zeros_like(acc)
        ws = torch.empty(lib().islam_imu_preint_bwd_scratch_bytes(nframes), dtype=torch.uint8, device=dt.device)
        check(lib().islam_imu_preint_bwd(ptr(dt), ptr(gyro), ptr(acc), ptr(seg), nframes, int(dt.shape[0]), c_double(gravity),
                                         1 if motion else 0, ptr(scratch), ptr(g_pos), ptr(g_rot), ptr(g_vel), ptr(g_gyro), ptr(g_acc),
                                         ptr(ws), code, stream_ptr(dt.device)))
        return g_gyro, g_acc, None, None, None, None, None, None, None, None


def imu_preint(dt, gyro, acc, seg, seg_host, init_pos, init_rot, init_vel, gravity, motion_mode):
    """One IMUModule.integrate frame loop (imu_integrator.py:116-158).  dt (S), gyro/acc (S,3) on device,
    float32 or float64; seg int64 device tensor (nframes+1), seg_host the same on the host.  Differentiable w.r.t. gyro / acc
    when either requires grad."""
    if torch.is_grad_enabled() and (gyro.requires_grad or acc.requires_grad):
        return _ImuPreint.apply(gyro, acc, dt, seg, seg_host, init_pos, init_rot, init_vel, gravity, motion_mode)
    return _imu_preint_raw(dt, gyro, acc, seg, seg_host, init_pos, init_rot, init_vel, gravity, motion_mode)[:3]


def _variance3(v, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError('%s: one variance or three, got %d values' % (name, a.size))
    return (ctypes.c_double * 3)(*a)


def imu_preint_cov(dt, gyro, acc, seg, seg_host, gyro_cov, acc_cov, motion_mode, init_cov=None, gyro_cov_s=None, acc_cov_s=None):
    """Covariance of the pre-integration over the frames of ``seg`` (islam_imu_preint_cov; definition in include/islam_hip.h):
    (rows, 9, 9) float64 on the device, error state [dphi, dv, dp]; rows = nframes in motion mode, nframes + 1 in world mode
    (row 0 = ``init_cov``, a 9x9 tensor or None = zero).  gyro_cov / acc_cov: a per-sample variance or three of them;
    gyro_cov_s / acc_cov_s: optional (S, 3) device tensors of per-sample variances in dt's dtype.  Forward values only."""
    require_cuda(dt, gyro, acc, seg, init_cov, gyro_cov_s, acc_cov_s)
    dtype = dt.dtype
    code = _dtype_code(dtype)
    dev = dt.device
    nframes = int(seg_host.shape[0]) - 1
    S = int(dt.shape[0])
    maxF = int(np.max(np.diff(seg_host))) if nframes > 0 else 0
    for v, name in ((gyro_cov_s, 'gyro_cov_s'), (acc_cov_s, 'acc_cov_s')):
        if v is not None and (tuple(v.shape) != (S, 3) or v.dtype != dtype or not v.is_contiguous()):
            raise ValueError('%s: a contiguous (%d, 3) tensor of %s expected' % (name, S, dtype))
    if init_cov is not None:
        if tuple(init_cov.shape) != (9, 9):
            raise ValueError('init_cov: a 9x9 tensor expected, got %s' % (tuple(init_cov.shape),))
        init_cov = init_cov.to(torch.float64).contiguous()
    rows = nframes if motion_mode else nframes + 1
    out = torch.empty((rows, 9, 9), dtype=torch.float64, device=dev)
    scratch = None
    if not motion_mode and nframes > 0:
        scratch = torch.empty(lib().islam_imu_preint_cov_scratch_bytes(S, nframes), dtype=torch.uint8, device=dev)
    check(lib().islam_imu_preint_cov(ptr(dt), ptr(gyro), ptr(acc), ptr(seg), nframes, S, maxF, _variance3(gyro_cov, 'gyro_cov'),
                                     _variance3(acc_cov, 'acc_cov'), ptr(gyro_cov_s), ptr(acc_cov_s), ptr(init_cov),
                                     1 if motion_mode else 0, ptr(out), ptr(scratch), code, stream_ptr(dev)))
    return out


def imu_preint_bias_jac(dt, gyro, acc, seg, seg_host, motion_mode, init_jac=None):
    """Bias Jacobians of the pre-integration over the frames of ``seg`` (islam_imu_preint_bias_jac; definition in
    include/islam_hip.h): (rows, 9, 6) float64 on the device, rows [dphi, dv, dp], columns [b_g | b_a]; rows = nframes in motion
    mode, nframes + 1 in world mode (row 0 = ``init_jac``, a 9x6 tensor or None = zero).  Forward values only."""
    require_cuda(dt, gyro, acc, seg, init_jac)
    code = _dtype_code(dt.dtype)
    dev = dt.device
    nframes = int(seg_host.shape[0]) - 1
    S = int(dt.shape[0])
    maxF = int(np.max(np.diff(seg_host))) if nframes > 0 else 0
    if init_jac is not None:
        if tuple(init_jac.shape) != (9, 6):
            raise ValueError('init_jac: a 9x6 tensor expected, got %s' % (tuple(init_jac.shape),))
        init_jac = init_jac.to(torch.float64).contiguous()
    rows = nframes if motion_mode else nframes + 1
    with torch.no_grad():
        out = torch.empty((rows, 9, 6), dtype=torch.float64, device=dev)
        scratch = None
        if not motion_mode and nframes > 0:
            scratch = torch.empty(lib().islam_imu_preint_bias_jac_scratch_bytes(S, nframes), dtype=torch.uint8, device=dev)
        check(lib().islam_imu_preint_bias_jac(ptr(dt), ptr(gyro), ptr(acc), ptr(seg), nframes, S, maxF,
                                              None if motion_mode else ptr(init_jac), 1 if motion_mode else 0, ptr(out), ptr(scratch),
                                              code, stream_ptr(dev)))
    return out


def _rows_of(jac, rot):
    rows = int(jac.shape[0])
    if tuple(jac.shape) != (rows, 9, 6) or jac.dtype != torch.float64 or not jac.is_contiguous():
        raise ValueError('jac: a contiguous (rows, 9, 6) float64 tensor expected, got %s %s' % (tuple(jac.shape), jac.dtype))
    if tuple(rot.shape) != (rows, 4):
        raise ValueError('rotations: (%d, 4) expected, got %s' % (rows, tuple(rot.shape)))
    return rows


def _imu_arg(t, dtype, shape, name, got=True):
    """``t`` detached, in ``dtype`` and contiguous for the IMU entry points; None passes through; ValueError unless its shape is ``shape``"""
    if t is None:
        return None
    t = (t if t.dtype == dtype else t.to(dtype)).detach().contiguous()
    if tuple(t.shape) != shape:
        raise ValueError('%s: %s expected' % (name, shape) + (', got %s' % (tuple(t.shape),) if got else ''))
    return t


def imu_bias_correct(jac, rot, vel, pos, dbg, dba):
    """First-order correction of pre-integrated increments in their start-body frame for a further bias (dbg, dba: three values
    each) subtracted from the samples (islam_imu_bias_correct; include/islam_hip.h says how motion rows of a non-identity start
    rotation must be rotated first).  jac (rows, 9, 6) float64; rot (rows, 4) xyzw, vel, pos (rows, 3) in float32 or float64.
    Returns new (rot, vel, pos).  Forward values only."""
    require_cuda(jac, rot, vel, pos)
    rows = _rows_of(jac, rot)
    dtype = rot.dtype
    code = _dtype_code(dtype)
    with torch.no_grad():
        rot = _imu_arg(rot, dtype, (rows, 4), 'rotations')
        vel, pos = (_imu_arg(t, dtype, (rows, 3), 'vel / pos', got=False) for t in (vel, pos))
        out = [torch.empty_like(t) for t in (rot, vel, pos)]
        g3 = (ctypes.c_double * 3)(*np.asarray(torch.as_tensor(dbg).detach().cpu(), dtype=np.float64).reshape(3))
        a3 = (ctypes.c_double * 3)(*np.asarray(torch.as_tensor(dba).detach().cpu(), dtype=np.float64).reshape(3))
        check(lib().islam_imu_bias_correct(ptr(jac), ptr(rot), ptr(vel), ptr(pos), rows, g3, a3, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                           code, stream_ptr(rot.device)))
    return tuple(out)


def _imu_solve(symbol, rows, dtype, dev, args, mid, sizes):
    """The call of a closed-form IMU solve.  args: (tensor or None, dtype, shape, name) in the order of the entry point, made detached,
    contiguous and shape-checked by _imu_arg; mid: the values between rows and the outputs; sizes: the float64 outputs, carved in this
    order from one device buffer; the scratch is sized by `symbol`_scratch_bytes(rows).  A negative return code raises IslamHipError.
    Returns (the outputs as flat views of the buffer, the number of excluded rows)."""
    code = _dtype_code(dtype)
    with torch.no_grad():
        args = [_imu_arg(*a) for a in args]
        out = torch.empty(sum(sizes), dtype=torch.float64, device=dev)
        outs, o = [], 0
        for n in sizes:
            outs.append(out[o:o + n])
            o += n
        scratch = torch.empty(getattr(lib(), symbol + '_scratch_bytes')(rows), dtype=torch.uint8, device=dev)
        rc = getattr(lib(), symbol)(*[ptr(t) for t in args], rows, *mid, *[ptr(o) for o in outs], ptr(scratch), code, stream_ptr(dev))
    if rc < 0:
        check(rc)
    return outs, int(rc)


def imu_gyro_bias_solve(jac, rot_imu, rot_ref, weight=None):
    """Closed-form gyro-bias step (islam_imu_gyro_bias_solve): dbg minimises sum_i w_i |Log(rot_imu_i^T rot_ref_i) - J_phig,i dbg|^2.
    Returns (dbg (3) float64, H (3, 3) float64, number of rows excluded for a non-finite residual); the bias to subtract from the
    gyro samples becomes bias + dbg.  Raises IslamHipError (code ISLAM_ENOTPD) when H is singular.  Synchronises the stream."""
    require_cuda(jac, rot_imu, rot_ref, weight)
    rows = _rows_of(jac, rot_imu)
    dtype = rot_imu.dtype
    (dbg, H), bad = _imu_solve('islam_imu_gyro_bias_solve', rows, dtype, jac.device, (
        (jac, torch.float64, (rows, 9, 6), 'jac'), (rot_imu, dtype, (rows, 4), 'rotations'), (rot_ref, dtype, (rows, 4), 'rot_ref'),
        (weight, torch.float64, (rows,), 'weight')), (), (3, 9))
    return dbg, H.view(3, 3), bad


def _imu_alignment_solve(symbol, nx, names, rot, pos, dts, dvel, dpos, jac, cov, weight, flags, gravity_norm):
    """What imu_gravity_bias_solve (nx = 6) and imu_lever_scale_solve (nx = 10) share: the arguments of `symbol` (flags: the ints between
    rows and gravity_norm).  Returns (x (nx), H (nx, nx), vel (rows + 1, 3), number of excluded pairs)."""
    require_cuda(rot, pos, dts, dvel, dpos, jac, cov, weight)
    rows = int(dts.shape[0])
    dtype = dts.dtype
    (x, H, vel), bad = _imu_solve(symbol, rows, dtype, dts.device, (
        (rot, dtype, (rows + 1, 4), names[0]), (pos, dtype, (rows + 1, 3), names[1]), (dts, dtype, (rows,), 'dts'),
        (dvel, dtype, (rows, 3), 'dvel'), (dpos, dtype, (rows, 3), 'dpos'), (jac, torch.float64, (rows, 9, 6), 'jac'),
        (cov, torch.float64, (rows, 9, 9), 'cov'), (weight, torch.float64, (max(rows - 1, 0),), 'weight')),
        (*flags, c_double(0.0 if gravity_norm is None else float(gravity_norm))), (nx, nx * nx, 3 * (rows + 1)))
    return x, H.view(nx, nx), vel.view(rows + 1, 3), bad


def imu_gravity_bias_solve(rot_ref, pos_ref, dts, dvel, dpos, jac=None, cov=None, weight=None, gravity_norm=None):
    """Gravity, accelerometer bias and velocities from pre-integrated increments and trusted body poses, in closed form
    (islam_imu_gravity_bias_solve; definition in include/islam_hip.h).  rot_ref (rows + 1, 4) xyzw, pos_ref (rows + 1, 3): world
    poses of the IMU body; dts (rows), dvel, dpos (rows, 3): duration and gravity-free increments of every interval in its
    start-body frame, float32 or float64 (dts' dtype); jac (rows, 9, 6) float64 or None (no bias is estimated), cov (rows, 9, 9)
    float64 motion-mode covariances or None (unit weights), weight (rows - 1) per pair or None, gravity_norm: the known magnitude
    or None.  Returns (g (3), b (3), H (6, 6), vel (rows + 1, 3), number of excluded pairs), float64 on the device.  Raises
    IslamHipError (code ISLAM_ENOTPD) when the normal matrix is singular.  Synchronises the stream."""
    x, H, vel, bad = _imu_alignment_solve('islam_imu_gravity_bias_solve', 6, ('rot_ref', 'pos_ref'), rot_ref, pos_ref, dts, dvel, dpos, jac,
                                          cov, weight, (), gravity_norm)
    return x[0:3], x[3:6], H, vel, bad


def imu_lever_scale_solve(rot_body, pos_cam, dts, dvel, dpos, jac=None, cov=None, weight=None, solve_lever=True, solve_scale=False,
                          gravity_norm=None):
    """imu_gravity_bias_solve with the lever arm t of the camera-IMU mount and / or the scale s of the camera positions as further
    unknowns, in closed form (islam_imu_lever_scale_solve; definition in include/islam_hip.h).  rot_body (rows + 1, 4) xyzw: world
    rotations of the IMU BODY (the camera's conjugated by the mount's rotation), pos_cam (rows + 1, 3): world positions of the
    CAMERA, body position = s pos_cam - R_body t; dts, dvel, dpos, jac, cov, weight, gravity_norm as for imu_gravity_bias_solve.
    solve_lever / solve_scale: which of t and s are unknowns (not both False: that is imu_gravity_bias_solve).  Returns (g (3),
    b (3), t (3), s (), H (10, 10), vel (rows + 1, 3) of the body, number of excluded pairs), float64 on the device; unknowns that are
    not solved come back as exactly 0 (b, t) and 1 (s), with zero rows and columns in H.  Raises IslamHipError (code ISLAM_ENOTPD)
    when the normal matrix is singular (no rotation between the poses leaves t undetermined).  Synchronises the stream."""
    x, H, vel, bad = _imu_alignment_solve('islam_imu_lever_scale_solve', 10, ('rot_body', 'pos_cam'), rot_body, pos_cam, dts, dvel, dpos, jac,
                                          cov, weight, (int(solve_lever), int(solve_scale)), gravity_norm)
    return x[0:3], x[3:6], x[6:9], x[9], H, vel, bad


def imu_extrinsic_rot_solve(rot_imu, rot_cam, weight=None, delta=None, rounds=4):
    """Camera-IMU extrinsic rotation from pairs of relative rotations, in closed form (islam_imu_extrinsic_rot_solve; definition in
    include/islam_hip.h).  rot_imu (rows, 4) xyzw: the IMU's relative rotation over every frame (the motion rows' rotations), rot_cam
    (rows, 4): the camera's over the same frame, float32 or float64 (rot_imu's dtype); weight (rows) or None; delta: the Huber
    threshold on the angular residual in rad, None = no reweighting; rounds: the reweighted solves after the first one.  Returns
    (q (4) with rot_imu_i (x) q = q (x) rot_cam_i, eig (4) the eigenvalues ascending, res (rows) the angular residuals under q, number
    of excluded pairs), float64 on the device.  Rotations about one axis only leave q undetermined: eig[1] ~ eig[0], no error.
    Raises IslamHipError (code ISLAM_ENOTPD) when no pair takes part.  Synchronises the stream."""
    require_cuda(rot_imu, rot_cam, weight)
    rows = int(rot_imu.shape[0])
    dtype = rot_imu.dtype
    (q, eig, res), bad = _imu_solve('islam_imu_extrinsic_rot_solve', rows, dtype, rot_imu.device, (
        (rot_imu, dtype, (rows, 4), 'rot_imu'), (rot_cam, dtype, (rows, 4), 'rot_cam'), (weight, torch.float64, (rows,), 'weight')),
        (c_double(0.0 if delta is None else float(delta)), int(rounds)), (4, 4, rows))
    return q, eig, res, bad


def imu_time_offset_solve(jac, rot_imu, rot_ref, rate_start, rate_end, weight=None, solve_bias=True, delta=None, rounds=4):
    """Camera-IMU time offset td and a further gyro bias dbg from relative rotations, in closed form (islam_imu_time_offset_solve;
    definition in include/islam_hip.h): x = [dbg; td] minimises sum_i w_i rho_i |Log(rot_imu_i^T rot_ref_i) - J_phig,i dbg - u_i td|^2
    with u_i = rate_end_i - rot_imu_i^T rate_start_i.  jac (rows, 9, 6) float64 (None is allowed with solve_bias=False, which solves td
    alone); rot_imu, rot_ref (rows, 4) xyzw, rate_start, rate_end (rows, 3): the gyro samples that start at the two boundaries of every
    row, float32 or float64 (rot_imu's dtype); weight (rows) or None; delta: the Huber threshold on the residual in rad, None = no
    reweighting; rounds: the reweighted solves after the first one.  Returns (dbg (3), td (), H (4, 4), res (rows), number of excluded
    rows), float64 on the device; an image stamped t was taken at t + td on the IMU's clock.  Raises IslamHipError (code ISLAM_ENOTPD)
    when H is singular (a constant angular rate leaves td undetermined).  Synchronises the stream."""
    require_cuda(jac, rot_imu, rot_ref, rate_start, rate_end, weight)
    rows = int(rot_imu.shape[0])
    dtype = rot_imu.dtype
    if solve_bias and jac is None:
        raise ValueError('jac: the (rows, 9, 6) bias Jacobians are required with solve_bias=True')
    (x, H, res), bad = _imu_solve('islam_imu_time_offset_solve', rows, dtype, rot_imu.device, (
        (jac, torch.float64, (rows, 9, 6), 'jac'), (rot_imu, dtype, (rows, 4), 'rot_imu'), (rot_ref, dtype, (rows, 4), 'rot_ref'),
        (rate_start, dtype, (rows, 3), 'rate_start'), (rate_end, dtype, (rows, 3), 'rate_end'), (weight, torch.float64, (rows,), 'weight')),
        (int(bool(solve_bias)), c_double(0.0 if delta is None else float(delta)), int(rounds)), (4, 16, rows))
    return x[0:3], x[3], H.view(4, 4), res, bad


def imu_time_shift(rot, rate_start, rate_end, tau):
    """Pre-integrated rotations of a window moved by ``tau`` seconds without re-integrating (islam_imu_time_shift):
    Exp(-rate_start_i tau) (x) rot_i (x) Exp(rate_end_i tau), renormalised.  rot (rows, 4) xyzw, rate_start, rate_end (rows, 3) in float32
    or float64 (rot's dtype).  Returns the new rot.  Forward values only."""
    require_cuda(rot, rate_start, rate_end)
    rows = int(rot.shape[0])
    dtype = rot.dtype
    code = _dtype_code(dtype)
    with torch.no_grad():
        rot = _imu_arg(rot, dtype, (rows, 4), 'rot')
        rate_start, rate_end = _imu_arg(rate_start, dtype, (rows, 3), 'rate_start'), _imu_arg(rate_end, dtype, (rows, 3), 'rate_end')
        out = torch.empty_like(rot)
        check(lib().islam_imu_time_shift(ptr(rot), ptr(rate_start), ptr(rate_end), rows, c_double(float(tau)), ptr(out), code,
                                         stream_ptr(rot.device)))
    return out


# --------------------------------------------------------------------------- PVGO
def pvgo_default_params(loss_weight=(1, 1, 1, 1), radius=1e4, seg_len=(0, 0)):
    p = _lib.PvgoParams()
    lib().islam_pvgo_default_params(ctypes.byref(p))
    for i in range(4):
        p.w[i] = float(loss_weight[i]) ** 2            # pvgo.py:125-129
    p.radius = float(radius)
    p.seg_len[0], p.seg_len[1] = int(seg_len[0]), int(seg_len[1])
    return p


def pvgo_workspace(N, device):
    nbytes = lib().islam_pvgo_workspace_bytes(N)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def pvgo_reproj_struct(points, targets, K4, rgb2imu, weight, compat_first_motion=True):
    """islam_pvgo_reproj over float64 device tensors points (M,K,3), targets (M,K,2); keeps them alive on the struct."""
    require_cuda(points, targets)
    assert points.dtype == torch.float64 and targets.dtype == torch.float64 and points.is_contiguous() and targets.is_contiguous()
    assert points.shape[:2] == targets.shape[:2] and points.shape[2] == 3 and targets.shape[2] == 2
    r = _lib.PvgoReproj()
    r.points, r.targets, r.K = points.data_ptr(), targets.data_ptr(), int(points.shape[1])
    r.fx, r.fy, r.cx, r.cy = [float(v) for v in K4]
    for i, v in enumerate(rgb2imu):
        r.rgb2imu[i] = float(v)
    r.weight = float(weight)
    r.compat_first_motion = int(bool(compat_first_motion))
    r._keep = (points, targets)
    return r


def pvgo_reproj_reduce(nodes, reproj, dx=None):
    """Per-link keypoint reduction (M, 32): [J^T J upper (21) | J^T r (6) | r^T r | pad] at nodes or Exp(dx)*nodes."""
    require_cuda(nodes, dx)
    N = nodes.shape[0]
    red = torch.empty((N - 1, _lib.REPROJ_REC), dtype=torch.float64, device=nodes.device)
    check(lib().islam_pvgo_reproj_reduce(ptr(nodes), ptr(dx), N, ctypes.byref(reproj), ptr(red), stream_ptr(nodes.device)))
    return red


def _info_pair(info, E, M):
    """(info_vo (21,E) or None, info_imu (18,M) / info_imu9 (45,M) or None) of a packed pair, checked.  The row count of the second
    array says which layout it is: 18, three 3x3 per link, or 45, one correlated 9x9 per link (``_info_imu9``)."""
    info_vo, info_imu = info
    require_cuda(info_vo, info_imu)
    rows = 45 if info_imu is not None and info_imu.dim() == 2 and info_imu.shape[0] == 45 else 18
    for t, shape, name in ((info_vo, (21, E), 'info_vo'), (info_imu, (rows, M), 'info_imu')):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous()):
            raise ValueError('%s: a contiguous float64 %s tensor expected%s, got %s %s'
                             % (name, shape, ' (or (45, %d), one 9x9 per link)' % M if name == 'info_imu' else '', t.dtype, tuple(t.shape)))
    return info_vo, info_imu


def _info_imu9(info_imu):
    """True when a checked info_imu array is the correlated layout (45,M)."""
    return info_imu is not None and info_imu.shape[0] == 45


def pvgo_run_chain(nodes, vels, poses, drots, dtrans, dvels, dts, params, workspace=None, trace_cap=0, reproj=None, robust=None, info=None):
    """In-place LM on float64 device tensors.  Returns (PvgoResult, trace ndarray (trials,3) or None).
    robust: islam_amd.robust.RobustSpec (or None) -- islam_pvgo_run_chain_robust; not combinable with ``reproj``.
    info: (info_vo (21,N-1), info_imu (18,N-1)), the packed per-factor information (PvgoInfo.packed) -- islam_pvgo_run_chain_info;
    or (info_vo, info_imu9 (45,N-1)), one correlated 9x9 per link -- islam_pvgo_run_chain_info9.  Not combinable with ``reproj`` or
    ``robust``."""
    require_cuda(nodes, vels, poses, drots, dtrans, dvels, dts)
    if robust is not None and reproj is not None:
        raise NotImplementedError('robust kernels on the reprojection factor are not implemented')
    if info is not None and (robust is not None or reproj is not None):
        raise NotImplementedError('per-factor information with robust kernels or the reprojection factor is not implemented')
    for t in (nodes, vels, poses, drots, dtrans, dvels, dts):
        assert t.dtype == torch.float64 and t.is_contiguous()
    N = nodes.shape[0]
    if reproj is not None:
        assert reproj._keep[0].shape[0] == N - 1, 'reprojection factor needs one keypoint set per link'
    if workspace is None:
        workspace = pvgo_workspace(N, nodes.device)
    ws, nbytes = workspace
    res = _lib.PvgoResult()
    trace = np.zeros((trace_cap, 3), dtype=np.float64) if trace_cap > 0 else None
    tp = trace.ctypes.data_as(c_void_p) if trace is not None else c_void_p(0)
    if info is not None:
        info_vo, info_imu = _info_pair(info, N - 1, N - 1)
        run = lib().islam_pvgo_run_chain_info9 if _info_imu9(info_imu) else lib().islam_pvgo_run_chain_info
        check(run(ptr(nodes), ptr(vels), ptr(poses), ptr(drots), ptr(dtrans), ptr(dvels), ptr(dts), N, ctypes.byref(params), ptr(info_vo),
                  ptr(info_imu), ptr(ws), c_size_t(nbytes), ctypes.byref(res), tp, trace_cap, stream_ptr(nodes.device)))
    elif robust is not None:
        check(lib().islam_pvgo_run_chain_robust(ptr(nodes), ptr(vels), ptr(poses), ptr(drots), ptr(dtrans), ptr(dvels), ptr(dts), N,
                                                ctypes.byref(params), ctypes.byref(robust.struct()), ptr(ws), c_size_t(nbytes),
                                                ctypes.byref(res), tp, trace_cap, stream_ptr(nodes.device)))
    else:
        check(lib().islam_pvgo_run_chain_reproj(ptr(nodes), ptr(vels), ptr(poses), ptr(drots), ptr(dtrans), ptr(dvels), ptr(dts), N,
                                                ctypes.byref(params), ctypes.byref(reproj) if reproj is not None else None,
                                                ptr(ws), c_size_t(nbytes), ctypes.byref(res), tp, trace_cap,
                                                stream_ptr(nodes.device)))
    if trace is not None:
        trace = trace[:min(res.trials, trace_cap)]
    return res, trace


def pvgo_linearize(nodes, vels, poses, drots, dtrans, dvels, dts):
    N = nodes.shape[0]
    M = N - 1
    lin = torch.empty((42, M), dtype=torch.float64, device=nodes.device)
    part = torch.empty(((M + 63) // 64,), dtype=torch.float64, device=nodes.device)
    check(lib().islam_pvgo_linearize(ptr(nodes), ptr(vels), ptr(poses), ptr(drots), ptr(dtrans), ptr(dvels), ptr(dts), N,
                                     ptr(lin), ptr(part), stream_ptr(nodes.device)))
    return lin, part


def pvgo_build_normal(lin, dts, N, w4, vmin=1e-4, vmax=1e32, c_imu=None):
    """c_imu (3, N-1): robust multipliers of the velocity, rotation and translation-velocity factors (islam_pvgo_build_normal_scaled)."""
    dev = lin.device
    Hd = torch.zeros((N, 9, 9), dtype=torch.float64, device=dev)
    Ho = torch.zeros((N, 9, 9), dtype=torch.float64, device=dev)
    rhs = torch.zeros((N, 9), dtype=torch.float64, device=dev)
    w = (c_double * 4)(*[float(x) for x in w4])
    if c_imu is not None:
        assert c_imu.shape == (3, N - 1) and c_imu.dtype == torch.float64 and c_imu.is_contiguous()
        check(lib().islam_pvgo_build_normal_scaled(ptr(lin), ptr(dts), N, w, ptr(c_imu), c_double(vmin), c_double(vmax), ptr(Hd),
                                                   ptr(Ho), ptr(rhs), stream_ptr(dev)))
        return Hd, Ho, rhs
    check(lib().islam_pvgo_build_normal(ptr(lin), ptr(dts), N, w, c_double(vmin), c_double(vmax), ptr(Hd), ptr(Ho),
                                        ptr(rhs), stream_ptr(dev)))
    return Hd, Ho, rhs


def pvgo_build_normal_info(lin, dts, N, info_vo, info_imu, vmin=1e-4, vmax=1e32):
    """islam_pvgo_build_normal_info: the chain normal equations under per-factor information, packed as PvgoInfo.packed gives it --
    info_vo (21,N-1) or None (no VO group), info_imu (18,N-1); or info_imu (45,N-1), one correlated 9x9 per link
    (islam_pvgo_build_normal_info9).  Returns (Hd (N,9,9), Ho (N,9,9), rhs (N,9))."""
    require_cuda(lin, dts)
    dev = lin.device
    if info_imu is None:
        raise ValueError('pvgo_build_normal_info: info_imu is required')
    info_vo, info_imu = _info_pair((info_vo, info_imu), N - 1, N - 1)
    Hd = torch.zeros((N, 9, 9), dtype=torch.float64, device=dev)
    Ho = torch.zeros((N, 9, 9), dtype=torch.float64, device=dev)
    rhs = torch.zeros((N, 9), dtype=torch.float64, device=dev)
    build = lib().islam_pvgo_build_normal_info9 if _info_imu9(info_imu) else lib().islam_pvgo_build_normal_info
    check(build(ptr(lin), ptr(dts), N, ptr(info_vo), ptr(info_imu), c_double(vmin), c_double(vmax), ptr(Hd), ptr(Ho), ptr(rhs), stream_ptr(dev)))
    return Hd, Ho, rhs


def pvgo_robust_weights(vo, lin, robust, with_weights=True):
    """Robust multipliers and loss of a general-topology linearisation (islam_pvgo_robust_weights): vo (24,E) of
    islam_pvgo_linearize_edges, lin (42,M) of islam_pvgo_linearize, robust a RobustSpec.  Returns (c_vo (E,), c_imu (3,M), rho)
    with rho the device scalar sum of rho over every factor (c_vo, c_imu None when with_weights=False)."""
    require_cuda(vo, lin)
    E, M, dev = vo.shape[1], lin.shape[1], vo.device
    c_vo = torch.empty((E,), dtype=torch.float64, device=dev) if with_weights else None
    c_imu = torch.empty((3, M), dtype=torch.float64, device=dev) if with_weights else None
    part = torch.empty(((max(E, M) + 63) // 64,), dtype=torch.float64, device=dev)
    check(lib().islam_pvgo_robust_weights(ptr(vo), E, ptr(lin), M, ctypes.byref(robust.struct()), ptr(c_vo), ptr(c_imu), ptr(part),
                                          stream_ptr(dev)))
    return c_vo, c_imu, part.sum()


def pvgo_linearize_edges(nodes, edges, poses):
    """islam_pvgo_linearize_edges: residual and Jacobian blocks of the VO factor on every edge of ``edges`` (E,2) -> vo (24,E)."""
    require_cuda(nodes, edges, poses)
    E = edges.shape[0]
    vo = torch.empty((24, E), dtype=torch.float64, device=nodes.device)
    check(lib().islam_pvgo_linearize_edges(ptr(nodes), ptr(edges), ptr(poses), E, ptr(vo), stream_ptr(nodes.device)))
    return vo


def _check_vo_assembly(who, Hd, Ho, rhs, vo, edges, node_ptr, node_adj, c_vo, info_vo, more_index=()):
    """The argument checks pvgo_assemble_dense and pvgo_band_assemble share.  Returns (N, E)."""
    N, E = Hd.shape[0], vo.shape[1]
    if tuple(Hd.shape) != (N, 9, 9) or tuple(Ho.shape) != (N, 9, 9) or tuple(rhs.shape) != (N, 9) or tuple(vo.shape) != (24, E) or \
            tuple(edges.shape) != (E, 2) or node_ptr.numel() != N + 1 or node_adj.numel() != 2 * E:
        raise ValueError('%s: Hd, Ho (N,9,9), rhs (N,9), vo (24,E), edges (E,2), node_ptr (N+1,), node_adj (2E,) expected' % who)
    if (c_vo is not None and tuple(c_vo.shape) != (E,)) or (info_vo is not None and tuple(info_vo.shape) != (21, E)):
        raise ValueError('%s: c_vo (E,) / info_vo (21,E) expected' % who)
    for x in (Hd, Ho, rhs, vo, c_vo, info_vo):
        if x is not None and (x.dtype != torch.float64 or not x.is_contiguous()):
            raise ValueError('%s: contiguous float64 arrays expected' % who)
    for x in (edges, node_ptr, node_adj) + tuple(more_index):
        if x.dtype != torch.int64 or not x.is_contiguous():
            raise ValueError('%s: contiguous int64 index arrays expected' % who)
    return N, E


def pvgo_assemble_dense(Hd, Ho, rhs, vo, edges, node_ptr, node_adj, w0, c_vo=None, info_vo=None, out=None):
    """islam_pvgo_assemble_dense / _scaled / _info: the dense A (9N,9N), both triangles, and b (9N,) from the IMU-only chain arrays
    Hd, Ho (N,9,9), rhs (N,9) plus the VO factors of ``vo`` (24,E) on ``edges`` (E,2); node_ptr / node_adj the CSR of the edge ends per
    node.  The edges enter with weight w0, w0 * c_vo[e] (c_vo (E,): robust multipliers) or their own information info_vo (21,E), which
    replaces w0; not both.  out: (A, b) to write into.  Returns (A, b)."""
    require_cuda(Hd, Ho, rhs, vo, edges, node_ptr, node_adj, c_vo, info_vo)
    if c_vo is not None and info_vo is not None:
        raise ValueError('pvgo_assemble_dense: c_vo and info_vo cannot both be given')
    N, E = _check_vo_assembly('pvgo_assemble_dense', Hd, Ho, rhs, vo, edges, node_ptr, node_adj, c_vo, info_vo)
    if out is None:
        out = (torch.empty((9 * N, 9 * N), dtype=torch.float64, device=Hd.device), torch.empty((9 * N,), dtype=torch.float64, device=Hd.device))
    A, b = out
    if tuple(A.shape) != (9 * N, 9 * N) or tuple(b.shape) != (9 * N,) or any(x.dtype != torch.float64 or not x.is_contiguous() for x in out):
        raise ValueError('pvgo_assemble_dense: out = (A (9N,9N), b (9N,)), contiguous float64, expected')
    head = (ptr(Hd), ptr(Ho), ptr(rhs), ptr(vo))
    graph = (ptr(edges), ptr(node_ptr), ptr(node_adj))
    tail = (N, E, ptr(A), ptr(b), stream_ptr(Hd.device))
    if info_vo is not None:
        check(lib().islam_pvgo_assemble_dense_info(*head, ptr(info_vo), *graph, *tail))
    elif c_vo is not None:
        check(lib().islam_pvgo_assemble_dense_scaled(*head, ptr(c_vo), *graph, c_double(w0), *tail))
    else:
        check(lib().islam_pvgo_assemble_dense(*head, *graph, c_double(w0), *tail))
    return A, b


def pvgo_band_assemble(Hd, Ho, rhs, vo, edges, node_ptr, node_adj, w0, off_idx, c_vo=None, info_vo=None):
    """islam_pvgo_band_assemble: the VO factors of ``vo`` (24,E) on the validated ``edges`` (E,2) added IN PLACE to the IMU-only chain
    arrays Hd, Ho (N,9,9), rhs (N,9); node_ptr / node_adj the CSR of the edge ends per node, off_idx (K,) the off-band edges.
    c_vo (E,): robust multipliers; info_vo (21,E): per-edge information (not both).  Returns the off-band list (io (K,), jo (K,),
    So (K,6,6))."""
    require_cuda(Hd, Ho, rhs, vo, edges, node_ptr, node_adj, off_idx, c_vo, info_vo)
    N, E = _check_vo_assembly('pvgo_band_assemble', Hd, Ho, rhs, vo, edges, node_ptr, node_adj, c_vo, info_vo, (off_idx,))
    K, dev = int(off_idx.numel()), Hd.device
    io = torch.empty((K,), dtype=torch.int64, device=dev)
    jo = torch.empty((K,), dtype=torch.int64, device=dev)
    So = torch.empty((K, 6, 6), dtype=torch.float64, device=dev)
    none_if_empty = lambda x: x if K else None
    check(lib().islam_pvgo_band_assemble(ptr(Hd), ptr(Ho), ptr(rhs), ptr(vo), ptr(c_vo), ptr(info_vo), ptr(edges), ptr(node_ptr),
                                         ptr(node_adj), c_double(w0), N, E, ptr(none_if_empty(off_idx)), K, ptr(none_if_empty(io)),
                                         ptr(none_if_empty(jo)), ptr(none_if_empty(So)), stream_ptr(dev)))
    return io, jo, So


def pvgo_band_matvec(Hd, Ho, p, off_ptr, off_adj, io, jo, So):
    """islam_pvgo_band_matvec: y (N,9) = (B + R) p with B = (Hd, Ho) and R the off-band list (io, jo, So) of pvgo_band_assemble;
    off_ptr (N+1,), off_adj (2K,): the CSR of the off-band edge ends per node (entry = 2 * position in the list + end)."""
    require_cuda(Hd, Ho, p, off_ptr, off_adj, io, jo, So)
    N, K = Hd.shape[0], int(io.numel())
    if tuple(Ho.shape) != (N, 9, 9) or tuple(p.shape) != (N, 9) or not p.is_contiguous() or p.dtype != torch.float64 or \
            off_ptr.numel() != N + 1 or off_adj.numel() != 2 * K or jo.numel() != K or tuple(So.shape) != (K, 6, 6):
        raise ValueError('pvgo_band_matvec: Hd, Ho (N,9,9), p (N,9) contiguous float64, off_ptr (N+1,), off_adj (2K,), io, jo (K,), So (K,6,6) expected')
    y = torch.empty_like(p)
    if K:
        check(lib().islam_pvgo_band_matvec(ptr(Hd), ptr(Ho), ptr(p), ptr(off_ptr), ptr(off_adj), ptr(io), ptr(jo), ptr(So), N, K, ptr(y),
                                           stream_ptr(Hd.device)))
    else:
        check(lib().islam_pvgo_band_matvec(ptr(Hd), ptr(Ho), ptr(p), None, None, None, None, None, N, 0, ptr(y), stream_ptr(Hd.device)))
    return y


def pvgo_solve_chain(Hd, Ho, rhs, damping, seg_len=(0, 0), workspace=None):
    N = Hd.shape[0]
    if workspace is None:
        workspace = pvgo_workspace(N, Hd.device)
    ws, nbytes = workspace
    dx = torch.empty((N, 9), dtype=torch.float64, device=Hd.device)
    sl = (c_int * 2)(int(seg_len[0]), int(seg_len[1]))
    check(lib().islam_pvgo_solve_chain(ptr(Hd), ptr(Ho), ptr(rhs), c_double(damping), N, sl, ptr(ws), c_size_t(nbytes),
                                       ptr(dx), stream_ptr(Hd.device)))
    return dx


def pvgo_solve_chain_enqueue(Hd, Ho, rhs, workspace, seg_len=(0, 0), damping=0.0):
    """Stream-ordered islam_pvgo_solve_chain (the diagonal of Hd is damped in place, cumulatively): no read-back, no synchronisation; pvgo_solve_status() tells later
    whether any of the enqueued solves met a non-positive pivot."""
    N = Hd.shape[0]
    ws, nbytes = workspace
    dx = torch.empty((N, 9), dtype=torch.float64, device=Hd.device)
    sl = (c_int * 2)(int(seg_len[0]), int(seg_len[1]))
    check(lib().islam_pvgo_solve_chain_enqueue(ptr(Hd), ptr(Ho), ptr(rhs), c_double(damping), N, sl, ptr(ws), c_size_t(nbytes),
                                               ptr(dx), stream_ptr(Hd.device)))
    return dx


def pvgo_solve_status(N, workspace, device):
    """Synchronises; raises IslamHipError (ISLAM_ENOTPD) if a solve enqueued since the last call was not positive definite."""
    ws, nbytes = workspace
    check(lib().islam_pvgo_solve_status(N, ptr(ws), c_size_t(nbytes), stream_ptr(device)))


def pvgo_solve_chain_timed(Hd, Ho, rhs, damping, seg_len=(0, 0), workspace=None):
    """One solve with HIP events around each launch.  Returns (dx, {launch name: ms}, [(n, m, P) per level])."""
    N = Hd.shape[0]
    if workspace is None:
        workspace = pvgo_workspace(N, Hd.device)
    ws, nbytes = workspace
    dx = torch.empty((N, 9), dtype=torch.float64, device=Hd.device)
    sl = (c_int * 2)(int(seg_len[0]), int(seg_len[1]))
    ms = (c_float * 16)()
    plan = (c_int * (3 * _lib.MAX_LEVELS + 1))()
    nl = c_int(0)
    check(lib().islam_pvgo_solve_chain_timed(ptr(Hd), ptr(Ho), ptr(rhs), c_double(damping), N, sl, ptr(ws), c_size_t(nbytes),
                                             ptr(dx), ms, plan, ctypes.byref(nl), stream_ptr(Hd.device)))
    levels = [(plan[3 * l], plan[3 * l + 1], plan[3 * l + 2]) for l in range(_lib.MAX_LEVELS) if plan[3 * l] > 0]
    top = plan[3 * _lib.MAX_LEVELS]
    if nl.value == top + 1:         # root solve + whole down-sweep in one launch (bt_downsweep_kernel)
        names = ['eliminate_L%d' % l for l in range(top)] + ['root_L%d+downsweep' % top]
    else:
        names = ['eliminate_L%d' % l for l in range(top)] + ['top_L%d-%d' % (top, len(levels) - 1)] + \
            ['backsub_L%d' % l for l in range(top - 1, -1, -1)]
    return dx, dict(zip(names, [ms[i] for i in range(nl.value)])), levels


def pvgo_marginals_workspace(N, device):
    nbytes = lib().islam_pvgo_marginals_workspace_bytes(N)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def pvgo_marginals(Hd, Ho, anchor=0, seg_len=(0, 0), workspace=None, status=None):
    """Diagonal blocks Sd (N,9,9) and neighbour blocks So (N-1,9,9) of the inverse of the block-tridiagonal (Hd, Ho) with the pose
    DoF of node ``anchor`` held fixed (None: no gauge fix).  Hd, Ho are float64 device tensors and are not modified.
    status=None: synchronous, raises IslamHipError (ISLAM_ENOTPD) on a matrix that is not positive definite; status = a device int32
    tensor of one element: stream-ordered, no synchronisation, the status lands there."""
    require_cuda(Hd, Ho)
    assert Hd.dtype == torch.float64 and Ho.dtype == torch.float64 and Hd.is_contiguous() and Ho.is_contiguous()
    N = Hd.shape[0]
    assert Hd.shape == (N, 9, 9) and Ho.shape[1:] == (9, 9) and Ho.shape[0] >= N - 1
    if workspace is None:
        workspace = pvgo_marginals_workspace(N, Hd.device)
    ws, nbytes = workspace
    a = -1 if anchor is None else int(anchor)
    Sd = torch.empty((N, 9, 9), dtype=torch.float64, device=Hd.device)
    So = torch.empty((max(N - 1, 0), 9, 9), dtype=torch.float64, device=Hd.device)
    sl = (c_int * 2)(int(seg_len[0]), int(seg_len[1]))
    if status is None:
        check(lib().islam_pvgo_marginals(ptr(Hd), ptr(Ho), N, a, sl, ptr(ws), c_size_t(nbytes), ptr(Sd), ptr(So),
                                         stream_ptr(Hd.device)))
    else:
        check(lib().islam_pvgo_marginals_enqueue(ptr(Hd), ptr(Ho), N, a, sl, ptr(ws), c_size_t(nbytes), ptr(Sd), ptr(So),
                                                 ptr(status), stream_ptr(Hd.device)))
    return Sd, So


def pvgo_marginals_plan(N, seg_len=(0, 0)):
    """[(nodes, segment length, segments) per level] of pvgo_marginals; launches per call = 2 * len(levels) (1 for one level)."""
    sl = (c_int * 2)(int(seg_len[0]), int(seg_len[1]))
    plan = (c_int * (3 * _lib.MAX_LEVELS + 1))()
    nl = lib().islam_pvgo_marginals_plan(N, sl, plan)
    if nl < 1:
        check(nl)
    return [(plan[3 * l], plan[3 * l + 1], plan[3 * l + 2]) for l in range(nl)]


def pvgo_retract(nodes, vels, dx, sign=1.0):
    N = nodes.shape[0]
    no, vo = torch.empty_like(nodes), torch.empty_like(vels)
    check(lib().islam_pvgo_retract(ptr(nodes), ptr(vels), ptr(dx), c_double(sign), N, ptr(no), ptr(vo),
                                   stream_ptr(nodes.device)))
    return no, vo


def dense_chol_workspace(n, device):
    nbytes = lib().islam_dense_chol_workspace_bytes(n)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _dense_chol_args(A, vec, what):
    require_cuda(A, vec)
    n = A.shape[0]
    if not (A.dim() == 2 and A.shape[1] == n and A.dtype == torch.float64 and A.is_contiguous()):
        raise ValueError('dense_chol: A must be a contiguous square float64 matrix')
    if vec is not None and not (vec.shape == (n,) and vec.dtype == torch.float64 and vec.is_contiguous()):
        raise ValueError('dense_chol: %s must be a contiguous float64 vector of A.shape[0] entries' % what)
    return n


def dense_chol_factor(A, diag, ws=None):
    """islam_dense_chol_factor: A = L L^T in place.  Reads the strict upper triangle of A and ``diag``; writes L into the lower triangle and
    the diagonal of A; the strict upper triangle and ``diag`` stay as they are.  Enqueue only.  Returns info, a device int32 tensor
    (1): 0, or the 1-based index of the first pivot that was <= 0 or not finite."""
    n = _dense_chol_args(A, diag, 'diag')
    if ws is None:
        ws = dense_chol_workspace(n, A.device)
    info = torch.empty((1,), dtype=torch.int32, device=A.device)
    check(lib().islam_dense_chol_factor(ptr(A), ptr(diag), n, ptr(ws[0]), c_size_t(ws[1]), ptr(info), stream_ptr(A.device)))
    return info


def dense_chol_solve(A, b, ws=None):
    """islam_dense_chol_solve: x with L L^T x = b, L = the lower triangle and diagonal of A as dense_chol_factor left them.  Enqueue only."""
    n = _dense_chol_args(A, b, 'b')
    if ws is None:
        ws = dense_chol_workspace(n, A.device)
    x = torch.empty_like(b)
    check(lib().islam_dense_chol_solve(ptr(A), n, ptr(b), ptr(x), ptr(ws[0]), c_size_t(ws[1]), stream_ptr(A.device)))
    return x


def dense_chol_inverse_workspace(n, device):
    nbytes = lib().islam_dense_chol_inverse_workspace_bytes(n)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def dense_chol_invert_factor(A, ws=None):
    """islam_dense_chol_invert_factor: W = L^-1 in place, in the lower triangle and diagonal of A as dense_chol_factor left them; the strict
    upper triangle is neither written nor read as data.  ws: dense_chol_inverse_workspace(n, device).  Enqueue only.  Returns A."""
    n = _dense_chol_args(A, None, None)
    if ws is None:
        ws = dense_chol_inverse_workspace(n, A.device)
    check(lib().islam_dense_chol_invert_factor(ptr(A), n, ptr(ws[0]), c_size_t(ws[1]), stream_ptr(A.device)))
    return A


def pvgo_dense_cov_blocks(A, anchor=None, pairs=None):
    """islam_pvgo_dense_cov_blocks: blocks of Sigma = W^T W from W = the lower triangle and diagonal of A as dense_chol_invert_factor left
    them (9N x 9N).  pairs: (P,2) integers (sequence, array or tensor; read on the host) or None.  Returns (node_cov (N,9,9), pair_cov
    (P,9,9)) on A's device; the pose rows / columns of node ``anchor`` (None: no such node) are zero.  Enqueue only."""
    n = _dense_chol_args(A, None, None)
    if n % 9 != 0:
        raise ValueError('pvgo_dense_cov_blocks: A must be 9N x 9N (got n=%d)' % n)
    N = n // 9
    if pairs is None:
        ph = np.zeros((0, 2), dtype=np.int64)
    else:
        ph = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
        ph = np.ascontiguousarray(ph.reshape(-1, 2), dtype=np.int64)
    P = ph.shape[0]
    node_cov = torch.empty((N, 9, 9), dtype=torch.float64, device=A.device)
    pair_cov = torch.empty((P, 9, 9), dtype=torch.float64, device=A.device)
    check(lib().islam_pvgo_dense_cov_blocks(ptr(A), n, -1 if anchor is None else int(anchor), c_void_p(ph.ctypes.data if P else 0), P,
                                            ptr(node_cov), ptr(pair_cov) if P else c_void_p(0), stream_ptr(A.device)))
    return node_cov, pair_cov


def pvgo_band_inverse_workspace(N, R, device):
    nbytes = lib().islam_pvgo_band_inverse_workspace_bytes(N, R)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _host_int64(x, shape):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x.reshape(shape), dtype=np.int64)


def pvgo_band_inverse_columns(Hd, Ho, cols, anchor=0, seg_len=(0, 0), workspace=None, status=None):
    """islam_pvgo_band_inverse_columns: Y (9N, R) with Y[:, r] = B_a^-1 e_cols[r], B_a the block-tridiagonal (Hd, Ho) (N,9,9) with the pose
    DoF of node ``anchor`` held fixed (None: no gauge fix); cols: R DoF indices 9 * node + c (sequence, array or tensor; read on the host).
    Hd, Ho are not modified.  workspace: pvgo_band_inverse_workspace(N, R, device); status: a device int32 tensor of one element that
    receives ISLAM_OK / ISLAM_ENOTPD.  Enqueue only.  Returns Y."""
    require_cuda(Hd, Ho, status)
    N = Hd.shape[0]
    if tuple(Hd.shape) != (N, 9, 9) or tuple(Ho.shape[1:]) != (9, 9) or Ho.shape[0] < N - 1 or Ho.shape[0] > N:
        raise ValueError('pvgo_band_inverse_columns: Hd (N,9,9), Ho (N-1,9,9) or (N,9,9) expected')
    for x in (Hd, Ho):
        if x.dtype != torch.float64 or not x.is_contiguous():
            raise ValueError('pvgo_band_inverse_columns: contiguous float64 arrays expected')
    ch = _host_int64(cols, (-1,))
    R = ch.shape[0]
    if workspace is None:
        workspace = pvgo_band_inverse_workspace(N, R, Hd.device)
    ws, nbytes = workspace
    Y = torch.empty((9 * N, R), dtype=torch.float64, device=Hd.device)
    sl = (c_int * 2)(int(seg_len[0]), int(seg_len[1]))
    check(lib().islam_pvgo_band_inverse_columns(ptr(Hd), ptr(Ho), N, -1 if anchor is None else int(anchor), c_void_p(ch.ctypes.data if R else 0),
                                                R, sl, ptr(ws), c_size_t(nbytes), ptr(Y) if R else c_void_p(0), R, ptr(status),
                                                stream_ptr(Hd.device)))
    return Y


def pvgo_band_cov_blocks(Sd, So, Y, cols, Rc, G, anchor=0, pairs=None, workspace=None, status=None):
    """islam_pvgo_band_cov_blocks: node_cov (N,9,9) = Sd[k] - V_k Y_k^T and pair_cov (P,9,9) = base(a, b) - V_a Y_b^T with V = Y[:, :Rc] G
    on the fp64 matrix cores.  Sd (N,9,9), So (N-1,9,9): pvgo_marginals of the band; Y (9N, R): pvgo_band_inverse_columns for ``cols``
    (read on the host), whose first Rc entries are the closure ends' pose DoF; G (Rc, Rc) symmetric, or None when Rc = 0 (it is padded
    with zeros to a multiple of 16 here); pairs: (P,2) integers read on the host, or None.  workspace: pvgo_band_inverse_workspace(N, R,
    device); status: a device int32 tensor of one element that receives ISLAM_OK / ISLAM_ENOTPD.  Enqueue only."""
    require_cuda(Sd, So, Y, G, status)
    N, dev = Sd.shape[0], Sd.device
    ch = _host_int64(cols, (-1,))
    R, Rc = ch.shape[0], int(Rc)
    if tuple(Sd.shape) != (N, 9, 9) or tuple(So.shape) != (max(N - 1, 0), 9, 9) or Y.dim() != 2 or Y.shape[0] != 9 * N or Y.shape[1] < R:
        raise ValueError('pvgo_band_cov_blocks: Sd (N,9,9), So (N-1,9,9), Y (9N, >= R) expected')
    if not 0 <= Rc <= R or (Rc > 0 and (G is None or tuple(G.shape) != (Rc, Rc))):
        raise ValueError('pvgo_band_cov_blocks: 0 <= Rc <= R and G (Rc, Rc) expected')
    for x in (Sd, So, Y, G):
        if x is not None and (x.dtype != torch.float64 or not x.is_contiguous()):
            raise ValueError('pvgo_band_cov_blocks: contiguous float64 arrays expected')
    ph = _host_int64(pairs, (-1, 2)) if pairs is not None else np.zeros((0, 2), dtype=np.int64)
    P = ph.shape[0]
    Gp, ldg = None, 0
    if Rc > 0:
        ldg = (Rc + 15) // 16 * 16
        Gp = torch.zeros((ldg, ldg), dtype=torch.float64, device=dev)
        Gp[:Rc, :Rc] = G
    if workspace is None:
        workspace = pvgo_band_inverse_workspace(N, R, dev)
    ws, nbytes = workspace
    node_cov = torch.empty((N, 9, 9), dtype=torch.float64, device=dev)
    pair_cov = torch.empty((P, 9, 9), dtype=torch.float64, device=dev)
    check(lib().islam_pvgo_band_cov_blocks(ptr(Sd), ptr(So), ptr(Y) if R else c_void_p(0), int(Y.shape[1]), N, -1 if anchor is None else int(anchor),
                                           c_void_p(ch.ctypes.data if R else 0), R, Rc, ptr(Gp), ldg, c_void_p(ph.ctypes.data if P else 0), P,
                                           ptr(ws), c_size_t(nbytes), ptr(node_cov), ptr(pair_cov) if P else c_void_p(0), ptr(status),
                                           stream_ptr(dev)))
    return node_cov, pair_cov


def pvgo_align(nodes, vels, target7):
    N = nodes.shape[0]
    no, vo = torch.empty_like(nodes), torch.empty_like(vels)
    check(lib().islam_pvgo_align(ptr(nodes), ptr(vels), ptr(target7), N, ptr(no), ptr(vo), stream_ptr(nodes.device)))
    return no, vo


class _VoLoss(torch.autograd.Function):
    """graph.vo_loss(edges, poses) (pvgo.py:67-78): nodes detached, gradient to ``poses`` only, in PyPose's
    convention (left-tangent 6-vector stored in a 7-vector with a trailing 0)."""

    @staticmethod
    def forward(ctx, nodes, edges, poses):
        E = edges.shape[0]
        p64 = poses.detach().to(torch.float64).contiguous()
        err = torch.empty((E, 6), dtype=torch.float64, device=nodes.device)
        tl = torch.empty(E, dtype=torch.float64, device=nodes.device)
        rl = torch.empty(E, dtype=torch.float64, device=nodes.device)
        check(lib().islam_pvgo_vo_loss_fwd(ptr(nodes), ptr(edges), ptr(p64), E, ptr(err), ptr(tl), ptr(rl),
                                           stream_ptr(nodes.device)))
        ctx.save_for_backward(p64, err)
        ctx.out_dtype = poses.dtype
        return tl.to(poses.dtype), rl.to(poses.dtype)

    @staticmethod
    def backward(ctx, g_tl, g_rl):
        p64, err = ctx.saved_tensors
        E = p64.shape[0]
        grad = torch.empty((E, 7), dtype=torch.float64, device=p64.device)
        gt = g_tl.to(torch.float64).contiguous()
        gr = g_rl.to(torch.float64).contiguous()
        check(lib().islam_pvgo_vo_loss_bwd(ptr(p64), ptr(err), ptr(gt), ptr(gr), E, ptr(grad), stream_ptr(p64.device)))
        return None, None, grad.to(ctx.out_dtype)


def pvgo_vo_loss(nodes64, edges, poses):
    return _VoLoss.apply(nodes64, edges, poses)


class ClockProbe:
    """Shader clock the chip sustains while it is busy (islam_clock_probe): ``sample()`` queues a one-wavefront dependent-FMA kernel of
    ~40 us on a stream of this object's own -- it runs beside whatever the other streams are doing -- and ``mhz()`` reads the samples
    back (synchronises that stream only).  bench.py samples it before, during and after the stereo_vio measurement, so that a slow
    run names its cause (a box that clocks lower under load vs. anything else)."""

    def __init__(self, device, capacity=64, iters=20000):
        from ._lib import lib
        self.device, self.iters, self.n = torch.device(device), iters, 0
        self.buf = torch.zeros(capacity, 3, dtype=torch.int64, device=self.device)
        self.stream = torch.cuda.Stream(self.device)
        self.khz = lib().islam_wall_clock_khz(self.device.index or 0)

    def sample(self):
        from ._lib import check, lib, ptr, stream_ptr
        if self.n >= self.buf.shape[0]:
            return
        with torch.cuda.stream(self.stream):
            check(lib().islam_clock_probe(ptr(self.buf[self.n]), self.iters, stream_ptr(self.device)))
        self.n += 1

    def mhz(self):
        self.stream.synchronize()
        h = self.buf[:self.n].cpu().numpy().astype(float)
        return [float(c / w * self.khz * 1e-3) for w, c, _ in h if w > 0]
