"""Cost of the dense reprojection normal equations and of a 10-evaluation refinement at B = 8 links on
112 x 160 and 448 x 640 images: us per call beside the eager-torch DenseReprojectionLoss.__call__ on the same tensors (float32 and
float64; the only way to evaluate this residual without the kernel, value only, no derivative), and the fraction of the HBM roof
the reduction reaches at the 13 bytes per pixel it has to read (depth, two flow floats, one mask byte; 8 TB/s).  The time of
ops.dense_reproj_normal holds both of its launches and its allocations; a refinement evaluation is two launches as well.  HIP
events around every call, 5 warm-up calls, the median of 30.  There is no earlier version to compare against and no target.

    python scripts/dense_reproj_bench.py [--out profiles/dense_reproj_bench.json]
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
    from tests.test_dense_reproj_cpu import MOUNT, make_scene, right_perturb
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


def main():
    import torch
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
