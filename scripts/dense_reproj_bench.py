"""Cost of the dense reprojection normal equations and of a 10-evaluation refinement at B = 8 links on
112 x 160 and 448 x 640 images: us per call beside the eager-torch DenseReprojectionLoss.__call__ on the same tensors (float32 and
float64; the only way to evaluate this residual without the kernel, value only, no derivative), and the fraction of the HBM roof
the reduction reaches at the 13 bytes per pixel it has to read (depth, two flow floats, one mask byte; 8 TB/s).  The time of
ops.dense_reproj_normal holds both of its launches and its allocations; a refinement evaluation is two launches as well.  HIP
events around every call, 5 warm-up calls, the median of 30.  There is no earlier version to compare against and no target.

    python scripts/dense_reproj_bench.py [--out profiles/dense_reproj_bench.json]

--grad times the gradient of the refined pose in depth and flow instead: ops.dense_reproj_vjp alone, the
backward (ops.dense_reproj_ift_weights and ops.dense_reproj_vjp), a 10-evaluation refinement with its backward through autograd, and
what the gradient costs without the kernel: eager float64 torch autograd of w^T g on the same tensors.

    python scripts/dense_reproj_bench.py --grad [--case 448x640] [--out profiles/dense_reproj_grad_bench.json]

--joint times the joint (pose, inverse depth) problem instead: ops.dense_ba_normal, a 20- and a 10-evaluation
ops.dense_ba_refine, beside the pose-only ops.dense_reproj_normal / ops.dense_reproj_refine on the same tensors.

    python scripts/dense_reproj_bench.py --joint [--case 448x640] [--out profiles/dense_ba_bench.json]

--joint-grad times the gradient of the joint refinement in depth and flow instead, by the method of --grad:
ops.dense_ba_vjp alone (beside ops.dense_reproj_vjp on the same tensors), the whole backward (ops.dense_ba_ift_weights and
ops.dense_ba_vjp) with and without a gradient on inv_depth, a 20-evaluation refine_joint(differentiable=True) with its backward through
autograd, and what the gradient costs without the kernels: eager float64 torch autograd of the same Phi.

    python scripts/dense_reproj_bench.py --joint-grad [--case 448x640] [--out profiles/dense_ba_grad_bench.json]

--joint-grad-exact times the same backward with the exact (Newton) Hessian instead: ops.dense_ba_newton_weights and
ops.dense_ba_newton_vjp alone, the exact backward (both) with and without a gradient on inv_depth and with a weight map, and a
20-evaluation refine_joint(differentiable=True, hessian='exact') with its backward through autograd.  The yardstick is the Gauss-Newton
backward of --joint-grad and its refine_joint(differentiable=True), timed in the same process on the same tensors.

    python scripts/dense_reproj_bench.py --joint-grad-exact [--case 448x640] [--out profiles/dense_ba_newton_bench.json]

--uncertainty times the per-pixel prior weights and the posterior depth variance instead: a 20-evaluation
ops.dense_ba_refine without and with a weight map (the yardstick is the run without the map, in the same process), and
ops.dense_ba_depth_variance at the refined state with the sums given, marginal over the pose and conditional on it, beside
ops.dense_ba_vjp on the same tensors, which moves about as many bytes.

    python scripts/dense_reproj_bench.py --uncertainty [--case 448x640] [--out profiles/dense_ba_uncertainty_bench.json]

--propagate times the depth propagation instead: ops.dense_ba_depth_propagate of a refined state and its
variance into the next frame, alone and fused with a measurement at gate 3.  The yardstick is ops.dense_ba_depth_variance on the same
tensors in the same process, a pixel pass that moves about half as many bytes.

    python scripts/dense_reproj_bench.py --propagate [--case 448x640] [--out profiles/depth_propagate_bench.json]

--regularize times the regularisation of the propagated map instead: ops.dense_ba_depth_regularize with a
measurement at gate 3 on the pure propagation of the same state, all radii 0, 1 and 2, and the pure propagation followed by it.  The
yardstick is ops.dense_ba_depth_propagate with the same measurement in the same process, the one call it replaces.

    python scripts/dense_reproj_bench.py --regularize [--case 448x640] [--out profiles/depth_regularize_bench.json]

--propagate-grad times the gradient of the depth propagation instead: ops.dense_ba_depth_propagate_vjp on the
source and flags of the propagation fused with a measurement at gate 3, with both cotangents and with the one on the inverse depth
alone, and the propagation followed by it.  The yardstick is the forward ops.dense_ba_depth_propagate on the same tensors in the same
process.

    python scripts/dense_reproj_bench.py --propagate-grad [--case 448x640] [--out profiles/depth_propagate_grad_bench.json]

--uncertainty-grad times the gradient of the posterior variance instead: ops.dense_ba_depth_variance_vjp at
the refined state of --uncertainty's scene (weight map included) with the sums given, marginal over the pose and conditional on it.
The yardstick is the forward ops.dense_ba_depth_variance on the same tensors in the same process.

    python scripts/dense_reproj_bench.py --uncertainty-grad [--case 448x640] [--out profiles/dense_ba_uncertainty_grad_bench.json]

--regularize-grad times the gradient of the depth regularisation instead: ops.dense_ba_depth_regularize_vjp on
the flags of --regularize's regularisation fused with a measurement at gate 3, at radii 1, 2 and 0, with both cotangents and with the
one on the inverse depth alone.  The yardstick is the forward ops.dense_ba_depth_regularize at the same radii in the same process.

    python scripts/dense_reproj_bench.py --regularize-grad [--case 448x640] [--out profiles/depth_regularize_grad_bench.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'112x160': (112, 160), '448x640': (448, 640)}
B = 8
HBM_GBS = 8000.0
PIXEL_BYTES = 13


def run_case(H, W):
    import numpy as np
    import torch
    from islam_amd import lietensor as pp
    from islam_amd import ops, robust
    from islam_amd.dense_ba import DenseReprojectionLoss
    from tests.dense_reproj_f64 import MOUNT, make_scene, right_perturb
    dev = torch.device('cuda:0')
    # the scene of the tests at this size (a quarter-resolution pinhole camera: fx = W / 2)
    sc = make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    fx, fy, cx, cy = sc['intr'][0]
    loss32 = DenseReprojectionLoss(depth, flow, fx, fy, cx, cy, mask, pp.SE3(mount.float()), device=dev)
    loss64 = DenseReprojectionLoss(depth.double(), flow.double(), fx, fy, cx, cy, mask, pp.SE3(mount), device=dev)
    m32, m64 = pp.SE3(motion.float()), pp.SE3(motion)
    fns = {'normal': lambda: ops.dense_reproj_normal(depth, flow, mask, motion, intr, rgb2imu=mount),
           'normal_huber': lambda: ops.dense_reproj_normal(depth, flow, mask, motion, intr, rgb2imu=mount, kernel=robust.Huber(1.0)),
           'refine10': lambda: ops.dense_reproj_refine(depth, flow, mask, motion, intr, rgb2imu=mount, iters=10),
           'torch_call_f32': lambda: loss32(m32), 'torch_call_f64': lambda: loss64(m64)}

    def median(fn, n=30):
        us = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        return 0.5 * (us[n // 2 - 1] + us[n // 2])

    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[name] = median(fn)
    ne = fns['normal']()
    out['l1_mean_vs_torch_f64'] = float(((ne.l1 / ne.count) - loss64(m64)).abs().max())
    out['valid_fraction'] = float(ne.count.sum()) / (B * H * W)
    out['MB_read'] = PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_normal'] = PIXEL_BYTES * B * H * W / (out['normal'] * 1e-6) / 1e9 / HBM_GBS
    out['hbm_frac_refine_eval'] = PIXEL_BYTES * B * H * W / (out['refine10'] / 10 * 1e-6) / 1e9 / HBM_GBS
    return out


GRAD_PIXEL_BYTES = 25          # the 13 of the forward pass and three float32 stores


def torch_wtg(depth, flow, mask, R, t, A, intr, w):
    """w^T g of every link in eager torch (float64, differentiable in depth and flow; the valid set is held fixed): what the gradient
    costs without the kernel.  R (B,3,3), t (B,3): T^-1 per link; A (6,6) = Ad(C^-1)."""
    import torch
    B, H, W = depth.shape
    fx, fy, cx, cy = (intr[:, k].view(B, 1, 1) for k in range(4))
    u = torch.arange(W, dtype=torch.float64, device=depth.device).view(1, 1, W)
    v = torch.arange(H, dtype=torch.float64, device=depth.device).view(1, H, 1)
    P = torch.stack([depth * ((u - cx) / fx), depth * ((v - cy) / fy), depth], -1)
    Q = (P.view(B, H * W, 3) @ R.mT + t.view(B, 1, 3)).view(B, H, W, 3)
    Qx, Qy, Qz = Q.unbind(-1)
    with torch.no_grad():
        valid = mask & (Qz > 0.1)
        valid = valid & ((Qx / Qz).abs() <= 1.0) & ((Qy / Qz).abs() <= 1.0)
    Qz = torch.where(valid, Qz, torch.ones_like(Qz))
    ru = fx * Qx / Qz + cx - (flow[:, 0] + u)
    rv = fy * Qy / Qz + cy - (flow[:, 1] + v)
    wc = w @ A.T
    wr, wf = wc[:, :3].view(B, 1, 1, 3), wc[:, 3:].view(B, 1, 1, 3).expand(B, H, W, 3)
    m = torch.cross(Q, wf, dim=-1) - wr
    qu = fx / Qz * m[..., 0] - fx * Qx / Qz ** 2 * m[..., 2]
    qv = fy / Qz * m[..., 1] - fy * Qy / Qz ** 2 * m[..., 2]
    return torch.where(valid, qu * ru + qv * rv, torch.zeros_like(ru)).sum()


def run_grad_case(H, W):
    """--grad: the backward of the refined pose alone and behind a 10-evaluation refinement, beside the
    forward pass it is expected to cost about as much as, and beside eager float64 torch autograd of w^T g on the same tensors."""
    import numpy as np
    import torch
    from islam_amd import lietensor as pp
    from islam_amd import ops, robust
    from islam_amd.dense_ba import DenseReprojectionLoss
    from oracle import lie
    from tests.dense_reproj_f64 import MOUNT, make_scene, right_perturb
    dev = torch.device('cuda:0')
    sc = make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    coeff = d(np.random.default_rng(0).standard_normal((B, 7)))
    fx, fy, cx, cy = sc['intr'][0]
    ref = ops.dense_reproj_refine(depth, flow, mask, motion, intr, rgb2imu=mount, iters=10)
    w, status = ops.dense_reproj_ift_weights(ref.H, ref.motion, coeff, ref.status)
    zl, fl = depth.clone().requires_grad_(), flow.clone().requires_grad_()
    loss = DenseReprojectionLoss(zl, fl, fx, fy, cx, cy, mask, pp.SE3(mount), device=dev)

    def refine_backward():
        zl.grad = fl.grad = None
        (loss.refine(pp.SE3(motion), iters=10, differentiable=True).motion * coeff).sum().backward()

    def backward():
        wk, st = ops.dense_reproj_ift_weights(ref.H, ref.motion, coeff, ref.status)
        return ops.dense_reproj_vjp(depth, flow, mask, ref.motion, intr, wk, rgb2imu=mount, status=st)

    # eager torch on the same tensors, float64, at the refined pose
    pose = ref.motion.cpu().numpy()
    Ti = np.stack([lie.se3_inv(lie.se3_mul(lie.se3_mul(lie.se3_inv(MOUNT), p), MOUNT)) for p in pose])
    R, t = d(np.stack([lie.quat_matrix(x[3:]) for x in Ti])), d(Ti[:, :3])
    A = d(lie.se3_adj(lie.se3_inv(MOUNT)))
    z64, f64 = depth.double().requires_grad_(), flow.double().requires_grad_()

    def torch_autograd():
        return torch.autograd.grad(torch_wtg(z64, f64, mask, R, t, A, intr, w), (z64, f64))

    fns = {'normal': lambda: ops.dense_reproj_normal(depth, flow, mask, motion, intr, rgb2imu=mount),
           'vjp': lambda: ops.dense_reproj_vjp(depth, flow, mask, ref.motion, intr, w, rgb2imu=mount, status=status),
           'vjp_huber': lambda: ops.dense_reproj_vjp(depth, flow, mask, ref.motion, intr, w, rgb2imu=mount, kernel=robust.Huber(1.0), status=status),
           'backward': backward, 'refine10': lambda: ops.dense_reproj_refine(depth, flow, mask, motion, intr, rgb2imu=mount, iters=10),
           'refine10_backward': refine_backward, 'torch_autograd_f64': torch_autograd}

    def median(fn, n=30):
        us = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        return 0.5 * (us[n // 2 - 1] + us[n // 2])

    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[name] = median(fn)
    gd, gf = backward()
    td, tf = torch_autograd()
    out['grad_depth_vs_torch_f64'] = float((gd.double() - td).abs().max() / td.abs().max())
    out['grad_flow_vs_torch_f64'] = float((gf.double() - tf).abs().max() / tf.abs().max())
    out['MB_moved'] = GRAD_PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_vjp'] = GRAD_PIXEL_BYTES * B * H * W / (out['vjp'] * 1e-6) / 1e9 / HBM_GBS
    out['hbm_frac_normal'] = PIXEL_BYTES * B * H * W / (out['normal'] * 1e-6) / 1e9 / HBM_GBS
    out['vjp_over_normal'] = out['vjp'] / out['normal']
    out['torch_over_backward'] = out['torch_autograd_f64'] / out['backward']
    return out


def main_grad(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_grad_case(*hw) for case, hw in cases.items()}
    cols = ('normal', 'vjp', 'vjp_huber', 'backward', 'refine10', 'refine10_backward', 'torch_autograd_f64', 'MB_moved', 'hbm_frac_vjp',
            'hbm_frac_normal', 'vjp_over_normal', 'torch_over_backward', 'grad_depth_vs_torch_f64', 'grad_flow_vs_torch_f64')
    print('us per call at B = %d: the median of 30; hbm_frac_vjp: %d bytes per pixel over the time, of %.0f GB/s' % (B, GRAD_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'dense_reproj_grad_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


JOINT_PIXEL_BYTES = 29          # an evaluation of the joint refinement: the 13 of the pose-only pass, 8 of rho read, 8 of trial rho written


def run_joint_case(H, W):
    """--joint: the depth-marginalised normal equations and the joint refinement beside the pose-only calls on
    the same tensors (the depth map carries sigma_rho = 0.02 /m of inverse-depth noise)."""
    import numpy as np
    import torch
    from islam_amd import ops
    from tests.dense_reproj_f64 import MOUNT, PRIOR_W, make_scene, noisy_prior, right_perturb
    dev = torch.device('cuda:0')
    sc = noisy_prior(make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False), seed=2)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    w = torch.full((B,), PRIOR_W, dtype=torch.float64, device=dev)
    fns = {'normal': lambda: ops.dense_reproj_normal(depth, flow, mask, motion, intr, rgb2imu=mount),
           'ba_normal': lambda: ops.dense_ba_normal(depth, flow, mask, motion, intr, w, rgb2imu=mount),
           'refine10': lambda: ops.dense_reproj_refine(depth, flow, mask, motion, intr, rgb2imu=mount, iters=10),
           'refine20': lambda: ops.dense_reproj_refine(depth, flow, mask, motion, intr, rgb2imu=mount, iters=20),
           'ba_refine10': lambda: ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=10),
           'ba_refine20': lambda: ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20)}

    def median(fn, n=30):
        us = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        return 0.5 * (us[n // 2 - 1] + us[n // 2])

    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[name] = median(fn)
    out['ba_eval'] = (out['ba_refine20'] - out['ba_refine10']) / 10          # the slope: one evaluation without the call's fixed cost
    out['eval'] = (out['refine20'] - out['refine10']) / 10
    out['ba_eval_over_eval'] = out['ba_eval'] / out['eval']
    out['MB_moved_per_eval'] = JOINT_PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_ba_eval'] = JOINT_PIXEL_BYTES * B * H * W / (out['ba_eval'] * 1e-6) / 1e9 / HBM_GBS
    r = fns['ba_refine20']()
    out['status_ok'] = int((r.status == 0).sum())
    out['accepted_mean'] = float(r.accepted.double().mean())
    return out


def main_joint(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_joint_case(*hw) for case, hw in cases.items()}
    cols = ('normal', 'ba_normal', 'refine10', 'refine20', 'ba_refine10', 'ba_refine20', 'eval', 'ba_eval', 'ba_eval_over_eval', 'MB_moved_per_eval',
            'hbm_frac_ba_eval', 'status_ok', 'accepted_mean')
    print('us per call at B = %d: the median of 30; hbm_frac_ba_eval: %d bytes per pixel over the time, of %.0f GB/s' % (B, JOINT_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'dense_ba_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


JOINT_GRAD_PIXEL_BYTES = 41          # the joint VJP: the 13 of the pose-only pass, rho and the gradient on it (8 each), three float32 stores


def torch_phi(depth, flow, mask, rho, R, t, A, intr, lam, v_d, w):
    """Phi = lambda_p^T g_p + sum lambda_d g_d of every link in eager torch (float64, no robust kernel, differentiable in depth and flow;
    the state, lambda and the valid set are held fixed; lambda_d is formed here from lam and v_d as the kernel forms it): what the
    gradient of the joint refinement costs without the kernels.  R (B,3,3), t (B,3): T^-1 per link; A (6,6) = Ad(C^-1); w (B)."""
    import torch
    B, H, W = depth.shape
    fx, fy, cx, cy = (intr[:, k].view(B, 1, 1) for k in range(4))
    u = torch.arange(W, dtype=torch.float64, device=depth.device).view(1, 1, W)
    v = torch.arange(H, dtype=torch.float64, device=depth.device).view(1, H, 1)
    wb = w.view(B, 1, 1)
    with torch.no_grad():
        prior = torch.isfinite(depth) & (depth > 0)
        usable = prior & (rho > 0)
    zi = 1.0 / torch.where(usable, rho, torch.ones_like(rho))
    ray = torch.stack([((u - cx) / fx).expand(B, H, W), ((v - cy) / fy).expand(B, H, W), torch.ones_like(rho)], -1)
    Q = ((zi.unsqueeze(-1) * ray).view(B, H * W, 3) @ R.mT + t.view(B, 1, 3)).view(B, H, W, 3)
    dR = (ray.view(B, H * W, 3) @ R.mT).view(B, H, W, 3)
    Qx, Qy, Qz = Q.unbind(-1)
    with torch.no_grad():
        valid = mask & usable & (Qz > 0.1)
        valid = valid & ((Qx / Qz).abs() <= 1.0) & ((Qy / Qz).abs() <= 1.0)
    Qz = torch.where(valid, Qz, torch.ones_like(Qz))
    ru = fx * Qx / Qz + cx - (flow[:, 0] + u)
    rv = fy * Qy / Qz + cy - (flow[:, 1] + v)
    lc = lam @ A.T
    lr, lf = lc[:, :3].view(B, 1, 1, 3), lc[:, 3:].view(B, 1, 1, 3).expand(B, H, W, 3)
    m = torch.cross(Q, lf, dim=-1) - lr
    a, bq, cq, dq = fx / Qz, -fx * Qx / Qz ** 2, fy / Qz, -fy * Qy / Qz ** 2
    du, dv = a * m[..., 0] + bq * m[..., 2], cq * m[..., 1] + dq * m[..., 2]
    k = -(zi * zi)
    jdu, jdv = (a * dR[..., 0] + bq * dR[..., 2]) * k, (cq * dR[..., 1] + dq * dR[..., 2]) * k
    zero = torch.zeros_like(ru)
    ld = -(v_d + torch.where(valid, jdu * du + jdv * dv, zero)) / (torch.where(valid, jdu * jdu + jdv * jdv, zero) + wb)
    ld = torch.where(prior, ld, zero)
    rho0 = 1.0 / torch.where(prior, depth, torch.ones_like(depth))
    return torch.where(valid, (du + jdu * ld) * ru + (dv + jdv * ld) * rv, zero).sum() + torch.where(prior, wb * ld * (rho - rho0), zero).sum()


def run_joint_grad_case(H, W):
    """--joint-grad: the backward of the joint refinement -- the VJP alone, the whole backward with and without a
    gradient on inv_depth, and a 20-evaluation refine_joint(differentiable=True) with its backward through autograd -- beside the
    pose-only VJP of section 3.24 on the same tensors and beside eager float64 torch autograd of the same Phi."""
    import numpy as np
    import torch
    from islam_amd import lietensor as pp
    from islam_amd import ops
    from islam_amd.dense_ba import DenseReprojectionLoss
    from oracle import lie
    from tests.dense_reproj_f64 import MOUNT, PRIOR_W, SIGMA_RHO, make_scene, noisy_prior, right_perturb
    dev = torch.device('cuda:0')
    sc = noisy_prior(make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False), seed=2)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    w = torch.full((B,), PRIOR_W, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    coeff, coeff_depth = d(rng.standard_normal((B, 7))), d(rng.standard_normal((B, H, W)).astype(np.float32))
    v_d = d(rng.standard_normal((B, H, W)))
    fx, fy, cx, cy = sc['intr'][0]
    ref = ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20)
    state = (depth, flow, mask, ref.motion, intr, w, ref.inv_depth)
    lam, status = ops.dense_ba_ift_weights(*state, ref.S, coeff, grad_inv_depth=v_d, rgb2imu=mount, status=ref.status)
    zl, fl = depth.clone().requires_grad_(), flow.clone().requires_grad_()
    loss = DenseReprojectionLoss(zl, fl, fx, fy, cx, cy, mask, pp.SE3(mount), device=dev)

    def refine_backward():
        zl.grad = fl.grad = None
        out = loss.refine_joint(pp.SE3(motion), SIGMA_RHO, sigma_px=0.3, iters=20, differentiable=True)
        ((out.motion * coeff).sum() + (out.depth * coeff_depth).sum()).backward()

    def backward(g=v_d):
        lk, st = ops.dense_ba_ift_weights(*state, ref.S, coeff, grad_inv_depth=g, rgb2imu=mount, status=ref.status)
        return ops.dense_ba_vjp(*state, lk, grad_inv_depth=g, rgb2imu=mount, status=st)

    pose = ref.motion.cpu().numpy()
    Ti = np.stack([lie.se3_inv(lie.se3_mul(lie.se3_mul(lie.se3_inv(MOUNT), p), MOUNT)) for p in pose])
    R, t = d(np.stack([lie.quat_matrix(x[3:]) for x in Ti])), d(Ti[:, :3])
    A = d(lie.se3_adj(lie.se3_inv(MOUNT)))
    z64, f64 = depth.double().requires_grad_(), flow.double().requires_grad_()

    def torch_autograd():
        return torch.autograd.grad(torch_phi(z64, f64, mask, ref.inv_depth, R, t, A, intr, lam, v_d, w), (z64, f64))

    pw, _ = ops.dense_reproj_ift_weights(ref.S, ref.motion, coeff, ref.status)
    fns = {'reproj_vjp': lambda: ops.dense_reproj_vjp(depth, flow, mask, ref.motion, intr, pw, rgb2imu=mount, status=ref.status),
           'ba_vjp': lambda: ops.dense_ba_vjp(*state, lam, grad_inv_depth=v_d, rgb2imu=mount, status=status),
           'ba_vjp_pose_loss': lambda: ops.dense_ba_vjp(*state, lam, rgb2imu=mount, status=status),
           'backward': backward, 'backward_pose_loss': lambda: backward(None),
           'ba_refine20': lambda: ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20),
           'refine_joint20_backward': refine_backward, 'torch_autograd_f64': torch_autograd}

    def median(fn, n=30):
        us = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        return 0.5 * (us[n // 2 - 1] + us[n // 2])

    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[name] = median(fn)
    gd, gf = fns['ba_vjp']()
    td, tf = torch_autograd()
    out['grad_depth_vs_torch_f64'] = float((gd.double() - td).abs().max() / td.abs().max())
    out['grad_flow_vs_torch_f64'] = float((gf.double() - tf).abs().max() / tf.abs().max())
    out['status_ok'] = int((status == 0).sum())
    out['MB_moved'] = JOINT_GRAD_PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_ba_vjp'] = JOINT_GRAD_PIXEL_BYTES * B * H * W / (out['ba_vjp'] * 1e-6) / 1e9 / HBM_GBS
    out['ba_vjp_over_reproj_vjp'] = out['ba_vjp'] / out['reproj_vjp']
    out['torch_over_backward'] = out['torch_autograd_f64'] / out['backward']
    return out


def main_joint_grad(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_joint_grad_case(*hw) for case, hw in cases.items()}
    cols = ('reproj_vjp', 'ba_vjp', 'ba_vjp_pose_loss', 'backward', 'backward_pose_loss', 'ba_refine20', 'refine_joint20_backward', 'torch_autograd_f64',
            'MB_moved', 'hbm_frac_ba_vjp', 'ba_vjp_over_reproj_vjp', 'torch_over_backward', 'grad_depth_vs_torch_f64', 'grad_flow_vs_torch_f64', 'status_ok')
    print('us per call at B = %d: the median of 30; hbm_frac_ba_vjp: %d bytes per pixel over the time, of %.0f GB/s' % (B, JOINT_GRAD_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'dense_ba_grad_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


def run_joint_grad_exact_case(H, W):
    """--joint-grad-exact: the backward of the joint refinement with the exact Hessian beside the Gauss-Newton
    backward of section 3.26 on the same tensors in the same process."""
    import numpy as np
    import torch
    from islam_amd import lietensor as pp
    from islam_amd import ops
    from islam_amd.dense_ba import DenseReprojectionLoss
    from tests.dense_reproj_f64 import MOUNT, PRIOR_W, SIGMA_RHO, make_scene, noisy_prior, right_perturb
    dev = torch.device('cuda:0')
    sc = noisy_prior(make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False), seed=2)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    w = torch.full((B,), PRIOR_W, dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)
    coeff, coeff_depth = d(rng.standard_normal((B, 7))), d(rng.standard_normal((B, H, W)).astype(np.float32))
    v_d = d(rng.standard_normal((B, H, W)))
    ones = torch.ones((B, H, W), dtype=torch.float32, device=dev)
    fx, fy, cx, cy = sc['intr'][0]
    ref = ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20)
    state = (depth, flow, mask, ref.motion, intr, w, ref.inv_depth)
    nw = ops.dense_ba_newton_weights(*state, coeff, grad_inv_depth=v_d, rgb2imu=mount, status=ref.status)
    zl, fl = depth.clone().requires_grad_(), flow.clone().requires_grad_()
    loss = DenseReprojectionLoss(zl, fl, fx, fy, cx, cy, mask, pp.SE3(mount), device=dev)

    def refine_backward(**kw):
        zl.grad = fl.grad = None
        out = loss.refine_joint(pp.SE3(motion), SIGMA_RHO, sigma_px=0.3, iters=20, differentiable=True, **kw)
        ((out.motion * coeff).sum() + (out.depth * coeff_depth).sum()).backward()

    def gn_backward(g=v_d):
        lk, st = ops.dense_ba_ift_weights(*state, ref.S, coeff, grad_inv_depth=g, rgb2imu=mount, status=ref.status)
        return ops.dense_ba_vjp(*state, lk, grad_inv_depth=g, rgb2imu=mount, status=st)

    def exact_backward(g=v_d, m=None):
        k = ops.dense_ba_newton_weights(*state, coeff, grad_inv_depth=g, rgb2imu=mount, status=ref.status, prior_scale=m)
        return ops.dense_ba_newton_vjp(*state, k.lambda_p, grad_inv_depth=g, rgb2imu=mount, status=k.status, prior_scale=m)

    fns = {'gn_backward': gn_backward, 'gn_backward_pose_loss': lambda: gn_backward(None),
           'newton_weights': lambda: ops.dense_ba_newton_weights(*state, coeff, grad_inv_depth=v_d, rgb2imu=mount, status=ref.status),
           'newton_vjp': lambda: ops.dense_ba_newton_vjp(*state, nw.lambda_p, grad_inv_depth=v_d, rgb2imu=mount, status=nw.status),
           'exact_backward': exact_backward, 'exact_backward_pose_loss': lambda: exact_backward(None), 'exact_backward_map': lambda: exact_backward(v_d, ones),
           'gn_refine_joint20_backward': refine_backward, 'exact_refine_joint20_backward': lambda: refine_backward(hessian='exact')}
    out = timed(fns)
    gd, gf = gn_backward()
    ed, ef = exact_backward()
    out['exact_over_gn_backward'] = out['exact_backward'] / out['gn_backward']
    out['exact_over_gn_refine_joint20_backward'] = out['exact_refine_joint20_backward'] / out['gn_refine_joint20_backward']
    out['grad_depth_exact_vs_gn'] = float((ed - gd).abs().max() / gd.abs().max())
    out['grad_flow_exact_vs_gn'] = float((ef - gf).abs().max() / gf.abs().max())
    out['fallback_pixels'] = int(nw.fallback.sum())
    out['status_ok'] = int((nw.status == 0).sum())
    return out


def main_joint_grad_exact(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_joint_grad_exact_case(*hw) for case, hw in cases.items()}
    cols = ('gn_backward', 'gn_backward_pose_loss', 'newton_weights', 'newton_vjp', 'exact_backward', 'exact_backward_pose_loss', 'exact_backward_map',
            'gn_refine_joint20_backward', 'exact_refine_joint20_backward', 'exact_over_gn_backward', 'exact_over_gn_refine_joint20_backward',
            'grad_depth_exact_vs_gn', 'grad_flow_exact_vs_gn', 'fallback_pixels', 'status_ok')
    print('us per call at B = %d: the median of 30; the Gauss-Newton backward (gn_*) is the yardstick of the same run' % B)
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'dense_ba_newton_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


VAR_PIXEL_BYTES = 33          # the variance pass: the 13 of the pose-only pass, the map (4), rho (8) and one float64 store (8)


def run_uncertainty_case(H, W):
    """--uncertainty: the weight map's cost per refinement evaluation and the cost of the variance pass."""
    import numpy as np
    import torch
    from islam_amd import ops
    from tests.dense_reproj_f64 import MOUNT, PRIOR_W, make_scene, noisy_prior, right_perturb
    dev = torch.device('cuda:0')
    sc = noisy_prior(make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False), seed=2)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    w = torch.full((B,), PRIOR_W, dtype=torch.float64, device=dev)
    m = d(np.exp2(np.random.default_rng(3).uniform(-1.0, 1.0, (B, H, W))).astype(np.float32))
    ref = ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20, prior_scale=m)
    state = (depth, flow, mask, ref.motion, intr, w)
    lam = torch.zeros((B, 6), dtype=torch.float64, device=dev)
    var = lambda marginal: ops.dense_ba_depth_variance(*state, inv_depth=ref.inv_depth, sums=ref.sums, status=ref.status, prior_scale=m, rgb2imu=mount,
                                                       marginal=marginal)
    fns = {'ba_refine20': lambda: ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20),
           'ba_refine20_map': lambda: ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20, prior_scale=m),
           'depth_var_marginal': lambda: var(True), 'depth_var_conditional': lambda: var(False),
           'ba_vjp': lambda: ops.dense_ba_vjp(*state, ref.inv_depth, lam, grad_inv_depth=ref.inv_depth, rgb2imu=mount, status=ref.status)}

    def median(fn, n=30):
        us = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        return 0.5 * (us[n // 2 - 1] + us[n // 2])

    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[name] = median(fn)
    v = var(True)
    out['status_ok'] = int((v.status == 0).sum())
    out['finite_fraction'] = float(torch.isfinite(v.var).double().mean())
    out['map_over_no_map'] = out['ba_refine20_map'] / out['ba_refine20']
    out['map_us_per_eval'] = (out['ba_refine20_map'] - out['ba_refine20']) / 20
    out['var_over_ba_vjp'] = out['depth_var_marginal'] / out['ba_vjp']
    out['var_over_refine_eval'] = out['depth_var_marginal'] / (out['ba_refine20'] / 20)
    out['MB_moved_var'] = VAR_PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_var_marginal'] = VAR_PIXEL_BYTES * B * H * W / (out['depth_var_marginal'] * 1e-6) / 1e9 / HBM_GBS
    out['hbm_frac_var_conditional'] = VAR_PIXEL_BYTES * B * H * W / (out['depth_var_conditional'] * 1e-6) / 1e9 / HBM_GBS
    return out


def main_uncertainty(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_uncertainty_case(*hw) for case, hw in cases.items()}
    cols = ('ba_refine20', 'ba_refine20_map', 'map_over_no_map', 'map_us_per_eval', 'depth_var_marginal', 'depth_var_conditional', 'ba_vjp',
            'var_over_ba_vjp', 'var_over_refine_eval', 'MB_moved_var', 'hbm_frac_var_marginal', 'hbm_frac_var_conditional', 'status_ok',
            'finite_fraction')
    print('us per call at B = %d: the median of 30; hbm_frac_var: %d bytes per pixel over the time, of %.0f GB/s' % (B, VAR_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'dense_ba_uncertainty_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


# the nominal bytes of one pixel in ops.dense_ba_depth_propagate with a measurement: the key cleared (8), the splat's rho, variance and
# mask (17) and its atomic (8), the fuse pass's key (8), the winner's rho, variance and mask again (17), depth_next and var_next (8), and
# its five stores (8 + 8 + 4 + 4 + 1); without a measurement 8 fewer
PROP_PIXEL_BYTES = 91


def propagate_scene(H, W):
    """What --propagate and --regularize time: a refined state of the scene and its variance, the next frame's measurement, and the
    calls on them.  Returns (var_fn: ops.dense_ba_depth_variance at the state, prop(**kw): ops.dense_ba_depth_propagate of it,
    depth_next, var_next)."""
    import numpy as np
    import torch
    from islam_amd import ops
    from tests.dense_reproj_f64 import MOUNT, PRIOR_W, make_scene, noisy_prior, right_perturb
    dev = torch.device('cuda:0')
    sc = noisy_prior(make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False), seed=2)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    w = torch.full((B,), PRIOR_W, dtype=torch.float64, device=dev)
    ref = ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20)
    state = (depth, flow, mask, ref.motion, intr, w)
    var_fn = lambda: ops.dense_ba_depth_variance(*state, inv_depth=ref.inv_depth, sums=ref.sums, status=ref.status, rgb2imu=mount)
    var = 0.09 * var_fn().var
    depth_next = d(sc['depth'] * (1.0 + 0.02 * np.random.default_rng(4).standard_normal(sc['depth'].shape)).astype(np.float32))
    var_next = torch.full((B, H, W), 4e-4, dtype=torch.float32, device=dev)
    pv = torch.full((B,), 1e-6, dtype=torch.float64, device=dev)          # on the device, like w: no host-to-device copy inside the timed call
    prop = lambda **kw: ops.dense_ba_depth_propagate(ref.inv_depth, var, ref.motion, intr, mask=mask, status=ref.status, rgb2imu=mount, process_var=pv, **kw)
    prop.state = dict(inv_depth=ref.inv_depth, var_inv_depth=var, motion=ref.motion, intr=intr, rgb2imu=mount, process_var=pv)      # for --propagate-grad
    return var_fn, prop, depth_next, var_next


def timed(fns, n=30):
    """us per call of every entry of fns: 5 warm-up calls, HIP events around each of n calls, the median."""
    import torch
    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        out[name] = 0.5 * (us[n // 2 - 1] + us[n // 2])
    return out


def run_propagate_case(H, W):
    """--propagate: the cost of carrying a refined state into the next frame."""
    var_fn, prop, depth_next, var_next = propagate_scene(H, W)
    fns = {'depth_var_marginal': var_fn, 'propagate': prop, 'propagate_fuse': lambda: prop(depth_next=depth_next, var_next=var_next, gate=3.0)}
    out = timed(fns)
    p = fns['propagate_fuse']()
    out['status_ok'] = int((p.status == 0).sum())
    out['hit_fraction'] = float(((p.flags & 1) != 0).double().mean())
    out['gated_fraction'] = float(((p.flags & 4) != 0).double().mean())
    out['propagate_over_var'] = out['propagate'] / out['depth_var_marginal']
    out['fuse_over_var'] = out['propagate_fuse'] / out['depth_var_marginal']
    out['MB_moved_fuse'] = PROP_PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_fuse'] = PROP_PIXEL_BYTES * B * H * W / (out['propagate_fuse'] * 1e-6) / 1e9 / HBM_GBS
    return out


def main_propagate(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_propagate_case(*hw) for case, hw in cases.items()}
    cols = ('depth_var_marginal', 'propagate', 'propagate_fuse', 'propagate_over_var', 'fuse_over_var', 'MB_moved_fuse', 'hbm_frac_fuse', 'status_ok',
            'hit_fraction', 'gated_fraction')
    print('us per call at B = %d: the median of 30; hbm_frac_fuse: %d bytes per pixel over the time, of %.0f GB/s' % (B, PROP_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'depth_propagate_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


# the nominal bytes of one pixel in ops.dense_ba_depth_regularize with a measurement: rho and its variance (16), the source index (4),
# depth_next and var_next (8), and the five stores (25); the halo is read again by the neighbouring tiles (a factor of up to
# 44 x 20 / (32 x 8) = 3.4 on the first 16 bytes at radii 2, 2, 2, mostly from the L2) and is not counted
REG_PIXEL_BYTES = 53


def run_regularize_case(H, W):
    """--regularize: the cost of regularising a propagated map beside the propagation that feeds it."""
    import torch
    from islam_amd import ops
    var_fn, prop, depth_next, var_next = propagate_scene(H, W)
    meas = dict(depth_next=depth_next, var_next=var_next, gate=3.0)
    pure = prop()
    dv = torch.full((B,), 1e-8, dtype=torch.float64, device=pure.inv_depth.device)          # on the device: no copy inside the timed call
    reg = lambda r, **kw: ops.dense_ba_depth_regularize(pure.inv_depth, pure.var_inv_depth, source=pure.source, status=pure.status, dist_var=dv,
                                                        occl_radius=r, fill_radius=r, smooth_radius=r, **kw)
    out = timed({'propagate_fuse': lambda: prop(**meas), 'propagate': prop, 'regularize_r1': lambda: reg(1, **meas),
                 'regularize_r2': lambda: reg(2, **meas), 'regularize_r0': lambda: reg(0, **meas),
                 'propagate_then_regularize_r1': lambda: (prop(), reg(1, **meas))})
    p, q = prop(**meas), reg(1, **meas)
    out['status_ok'] = int((q.status == 0).sum())
    out['hit_fraction'] = float(((p.flags & 1) != 0).double().mean())
    out['present_fraction_r1'] = float(((q.flags & 1) != 0).double().mean())
    out['filled_fraction_r1'] = float(((q.flags & 8) != 0).double().mean())
    out['removed_fraction_r1'] = float(((q.flags & 16) != 0).double().mean())
    out['r1_over_fuse'] = out['regularize_r1'] / out['propagate_fuse']
    out['r2_over_fuse'] = out['regularize_r2'] / out['propagate_fuse']
    out['chain_over_fuse'] = out['propagate_then_regularize_r1'] / out['propagate_fuse']
    out['hbm_frac_r1'] = REG_PIXEL_BYTES * B * H * W / (out['regularize_r1'] * 1e-6) / 1e9 / HBM_GBS
    return out


def main_regularize(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_regularize_case(*hw) for case, hw in cases.items()}
    cols = ('propagate_fuse', 'propagate', 'regularize_r0', 'regularize_r1', 'regularize_r2', 'propagate_then_regularize_r1', 'r1_over_fuse', 'r2_over_fuse',
            'chain_over_fuse', 'hbm_frac_r1', 'status_ok', 'hit_fraction', 'present_fraction_r1', 'filled_fraction_r1', 'removed_fraction_r1')
    print('us per call at B = %d: the median of 30; hbm_frac_r1: %d bytes per pixel over the time, of %.0f GB/s' % (B, REG_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'depth_regularize_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


# the nominal bytes of one pixel in ops.dense_ba_depth_propagate_vjp with a measurement and both cotangents.  As a target: flags (1),
# source (4), depth_next and var_next (8), the two cotangents (16), the winner's rho and variance gathered (16), two float32 stores (8).
# As a source: rho and variance (16), the source index, the flags, the cotangents and the measurement of its target gathered (4 + 1 +
# 16 + 8), two float64 stores (16)
PROP_GRAD_PIXEL_BYTES = 114


def run_propagate_grad_case(H, W):
    """--propagate-grad: the cost of the gradient of the propagation beside the propagation itself."""
    import torch
    from islam_amd import ops
    _, prop, depth_next, var_next = propagate_scene(H, W)
    meas = dict(depth_next=depth_next, var_next=var_next)
    fwd = prop(gate=3.0, **meas)
    g = torch.Generator(device='cuda').manual_seed(5)
    gr = torch.randn((B, H, W), dtype=torch.float64, device='cuda', generator=g)
    gs = 1e3 * torch.randn((B, H, W), dtype=torch.float64, device='cuda', generator=g)
    st = prop.state
    vjp = lambda **kw: ops.dense_ba_depth_propagate_vjp(st['inv_depth'], st['var_inv_depth'], st['motion'], st['intr'], fwd.source, fwd.flags, fwd.status,
                                                        rgb2imu=st['rgb2imu'], process_var=st['process_var'], **meas, **kw)
    out = timed({'propagate_fuse': lambda: prop(gate=3.0, **meas), 'vjp': lambda: vjp(grad_inv_depth=gr, grad_var_inv_depth=gs),
                 'vjp_inv_depth_only': lambda: vjp(grad_inv_depth=gr),
                 'propagate_then_vjp': lambda: (prop(gate=3.0, **meas), vjp(grad_inv_depth=gr, grad_var_inv_depth=gs))})
    r = vjp(grad_inv_depth=gr, grad_var_inv_depth=gs)
    out['status_ok'] = int((fwd.status == 0).sum())
    out['hit_fraction'] = float(((fwd.flags & 1) != 0).double().mean())
    out['nonzero_grad_fraction'] = float((r.grad_inv_depth != 0).double().mean())
    out['finite'] = int(all(bool(torch.isfinite(t).all()) for t in r))
    out['vjp_over_fuse'] = out['vjp'] / out['propagate_fuse']
    out['chain_over_fuse'] = out['propagate_then_vjp'] / out['propagate_fuse']
    out['MB_moved_vjp'] = PROP_GRAD_PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_vjp'] = PROP_GRAD_PIXEL_BYTES * B * H * W / (out['vjp'] * 1e-6) / 1e9 / HBM_GBS
    return out


def main_propagate_grad(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_propagate_grad_case(*hw) for case, hw in cases.items()}
    cols = ('propagate_fuse', 'vjp', 'vjp_inv_depth_only', 'propagate_then_vjp', 'vjp_over_fuse', 'chain_over_fuse', 'MB_moved_vjp', 'hbm_frac_vjp',
            'status_ok', 'hit_fraction', 'nonzero_grad_fraction', 'finite')
    print('us per call at B = %d: the median of 30; hbm_frac_vjp: %d bytes per pixel over the time, of %.0f GB/s' % (B, PROP_GRAD_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'depth_propagate_grad_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


# the nominal bytes of one pixel in ops.dense_ba_depth_regularize_vjp with a measurement, both cotangents and every stage on, at a pixel
# that is present: the front reads rho and its variance (16), flags (1), the measurement (8) and the cotangents (16) and stores two
# float32 (8), six float64 maps (48) and the state byte (1); the smoothing adjoint reads five maps, g3s and the state (49) and stores
# two (16); the filling adjoint reads four maps and the state (33) and stores two (16).  The halos and the three maps of the filled
# pixels are not counted
REG_GRAD_PIXEL_BYTES = 212


def run_regularize_grad_case(H, W):
    """--regularize-grad: the cost of the gradient of the regularisation beside the regularisation itself."""
    import torch
    from islam_amd import ops
    _, prop, depth_next, var_next = propagate_scene(H, W)
    meas = dict(depth_next=depth_next, var_next=var_next, gate=3.0)
    pure = prop()
    dv = torch.full((B,), 1e-8, dtype=torch.float64, device=pure.inv_depth.device)          # on the device: no copy inside the timed call
    radii = lambda r: dict(occl_radius=r, fill_radius=r, smooth_radius=r)
    reg = lambda r: ops.dense_ba_depth_regularize(pure.inv_depth, pure.var_inv_depth, source=pure.source, status=pure.status, dist_var=dv, **radii(r), **meas)
    fwd = {r: reg(r) for r in (0, 1, 2)}
    g = torch.Generator(device='cuda').manual_seed(5)
    gr = torch.randn((B, H, W), dtype=torch.float64, device='cuda', generator=g)
    gs = 1e3 * torch.randn((B, H, W), dtype=torch.float64, device='cuda', generator=g)
    vjp = lambda r, **kw: ops.dense_ba_depth_regularize_vjp(pure.inv_depth, pure.var_inv_depth, fwd[r].flags, status=fwd[r].status, dist_var=dv, **radii(r),
                                                            **meas, **kw)
    both = dict(grad_inv_depth=gr, grad_var_inv_depth=gs)
    out = timed({'regularize_r1': lambda: reg(1), 'regularize_r2': lambda: reg(2), 'regularize_r0': lambda: reg(0), 'vjp_r1': lambda: vjp(1, **both),
                 'vjp_r2': lambda: vjp(2, **both), 'vjp_r0': lambda: vjp(0, **both), 'vjp_r1_inv_depth_only': lambda: vjp(1, grad_inv_depth=gr),
                 'regularize_then_vjp_r1': lambda: (reg(1), vjp(1, **both))})
    r = vjp(1, **both)
    out['status_ok'] = int((fwd[1].status == 0).sum())
    out['present_fraction_r1'] = float(((fwd[1].flags & 1) != 0).double().mean())
    out['filled_fraction_r1'] = float(((fwd[1].flags & 8) != 0).double().mean())
    out['nonzero_grad_fraction'] = float((r.grad_inv_depth != 0).double().mean())
    out['finite'] = int(all(bool(torch.isfinite(t).all()) for t in r))
    for k in (0, 1, 2):
        out['vjp_over_forward_r%d' % k] = out['vjp_r%d' % k] / out['regularize_r%d' % k]
    out['MB_moved_vjp_r1'] = REG_GRAD_PIXEL_BYTES * B * H * W / 1e6
    out['hbm_frac_vjp_r1'] = REG_GRAD_PIXEL_BYTES * B * H * W / (out['vjp_r1'] * 1e-6) / 1e9 / HBM_GBS
    return out


def main_regularize_grad(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_regularize_grad_case(*hw) for case, hw in cases.items()}
    cols = ('regularize_r0', 'regularize_r1', 'regularize_r2', 'vjp_r0', 'vjp_r1', 'vjp_r2', 'vjp_r1_inv_depth_only', 'regularize_then_vjp_r1',
            'vjp_over_forward_r0', 'vjp_over_forward_r1', 'vjp_over_forward_r2', 'MB_moved_vjp_r1', 'hbm_frac_vjp_r1', 'status_ok',
            'present_fraction_r1', 'filled_fraction_r1', 'nonzero_grad_fraction', 'finite')
    print('us per call at B = %d: the median of 30; hbm_frac_vjp_r1: %d bytes per pixel over the time, of %.0f GB/s' % (B, REG_GRAD_PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'depth_regularize_grad_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


# the nominal bytes of one pixel in ops.dense_ba_depth_variance_vjp: per pixel pass the 25 that the variance pass reads (depth, flow, mask,
# map, rho) and the cotangent (8); the marginal mode makes two such passes (the sums of G, then the gradients), and the second stores
# grad_inv_depth (8) and grad_flow (8)
VAR_GRAD_PIXEL_BYTES = {True: 2 * 33 + 16, False: 33 + 16}


def run_uncertainty_grad_case(H, W):
    """--uncertainty-grad: the cost of the gradient of the variance beside the variance pass itself."""
    import numpy as np
    import torch
    from islam_amd import ops
    from tests.dense_reproj_f64 import MOUNT, PRIOR_W, make_scene, noisy_prior, right_perturb
    dev = torch.device('cuda:0')
    sc = noisy_prior(make_scene(B, H, W, seed=1, noise=0.3, intr0=(0.5 * W, 0.5 * W, 0.5 * W - 0.5, 0.5 * H - 0.5), vary=False), seed=2)
    start = right_perturb(sc['motion'], [0.01, -0.008, 0.012, 0.006, -0.005, 0.007])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    depth, flow, mask, motion, intr, mount = d(sc['depth']), d(sc['flow']), d(sc['mask']), d(start), d(sc['intr']), d(MOUNT)
    w = torch.full((B,), PRIOR_W, dtype=torch.float64, device=dev)
    m = d(np.exp2(np.random.default_rng(3).uniform(-1.0, 1.0, (B, H, W))).astype(np.float32))
    ref = ops.dense_ba_refine(depth, flow, mask, motion, intr, w, rgb2imu=mount, iters=20, prior_scale=m)
    state = (depth, flow, mask, ref.motion, intr, w)
    g = torch.randn((B, H, W), dtype=torch.float64, device=dev, generator=torch.Generator(device='cuda').manual_seed(5))
    var = lambda marginal: ops.dense_ba_depth_variance(*state, inv_depth=ref.inv_depth, sums=ref.sums, status=ref.status, prior_scale=m, rgb2imu=mount,
                                                       marginal=marginal)
    vjp = lambda marginal: ops.dense_ba_depth_variance_vjp(*state, ref.inv_depth, ref.sums, g, status=ref.status, prior_scale=m, rgb2imu=mount,
                                                           marginal=marginal)
    out = timed({'depth_var_marginal': lambda: var(True), 'depth_var_conditional': lambda: var(False), 'vjp_marginal': lambda: vjp(True),
                 'vjp_conditional': lambda: vjp(False), 'var_then_vjp_marginal': lambda: (var(True), vjp(True))})
    r = vjp(True)
    out['status_ok'] = int((r.status == 0).sum())
    out['nonzero_grad_fraction'] = float((r.grad_inv_depth != 0).double().mean())
    out['finite'] = int(all(bool(torch.isfinite(t.double()).all()) for t in r[:3]))
    out['vjp_over_var_marginal'] = out['vjp_marginal'] / out['depth_var_marginal']
    out['vjp_over_var_conditional'] = out['vjp_conditional'] / out['depth_var_conditional']
    for marginal, name in ((True, 'marginal'), (False, 'conditional')):
        out['MB_moved_vjp_' + name] = VAR_GRAD_PIXEL_BYTES[marginal] * B * H * W / 1e6
        out['hbm_frac_vjp_' + name] = VAR_GRAD_PIXEL_BYTES[marginal] * B * H * W / (out['vjp_' + name] * 1e-6) / 1e9 / HBM_GBS
    return out


def main_uncertainty_grad(argv):
    import torch
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    cases = {argv[argv.index('--case') + 1]: CASES[argv[argv.index('--case') + 1]]} if '--case' in argv else CASES
    rows = {case: run_uncertainty_grad_case(*hw) for case, hw in cases.items()}
    cols = ('depth_var_marginal', 'depth_var_conditional', 'vjp_marginal', 'vjp_conditional', 'var_then_vjp_marginal', 'vjp_over_var_marginal',
            'vjp_over_var_conditional', 'MB_moved_vjp_marginal', 'hbm_frac_vjp_marginal', 'MB_moved_vjp_conditional', 'hbm_frac_vjp_conditional',
            'status_ok', 'nonzero_grad_fraction', 'finite')
    print('us per call at B = %d: the median of 30; hbm_frac_vjp: %d (marginal) / %d (conditional) bytes per pixel over the time, of %.0f GB/s' % (
        B, VAR_GRAD_PIXEL_BYTES[True], VAR_GRAD_PIXEL_BYTES[False], HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in cases:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    path = argv[argv.index('--out') + 1] if '--out' in argv else os.path.join(ROOT, 'profiles', 'dense_ba_uncertainty_grad_bench.json')
    with open(path, 'w') as f:
        f.write(line + '\n')


def main():
    import torch
    if '--regularize-grad' in sys.argv[1:]:
        return main_regularize_grad(sys.argv[1:])
    if '--uncertainty-grad' in sys.argv[1:]:
        return main_uncertainty_grad(sys.argv[1:])
    if '--propagate-grad' in sys.argv[1:]:
        return main_propagate_grad(sys.argv[1:])
    if '--regularize' in sys.argv[1:]:
        return main_regularize(sys.argv[1:])
    if '--propagate' in sys.argv[1:]:
        return main_propagate(sys.argv[1:])
    if '--uncertainty' in sys.argv[1:]:
        return main_uncertainty(sys.argv[1:])
    if '--joint-grad-exact' in sys.argv[1:]:
        return main_joint_grad_exact(sys.argv[1:])
    if '--joint-grad' in sys.argv[1:]:
        return main_joint_grad(sys.argv[1:])
    if '--grad' in sys.argv[1:]:
        return main_grad(sys.argv[1:])
    if '--joint' in sys.argv[1:]:
        return main_joint(sys.argv[1:])
    assert torch.cuda.is_available(), 'dense_reproj_bench.py needs the GPU'
    rows = {case: run_case(*hw) for case, hw in CASES.items()}
    cols = ('normal', 'normal_huber', 'refine10', 'torch_call_f32', 'torch_call_f64', 'MB_read', 'hbm_frac_normal', 'hbm_frac_refine_eval',
            'valid_fraction', 'l1_mean_vs_torch_f64')
    print('us per call at B = %d: the median of 30; hbm_frac: %d bytes per pixel over the time, of %.0f GB/s' % (B, PIXEL_BYTES, HBM_GBS))
    print('| image | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in CASES:
        print('| %s | ' % case + ' | '.join('%.3g' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    if len(sys.argv) == 3 and sys.argv[1] == '--out':
        with open(sys.argv[2], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
