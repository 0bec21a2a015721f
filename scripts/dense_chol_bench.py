"""Cost of the dense fp64 Cholesky (islam_dense_chol_factor + islam_dense_chol_solve) at n = 9 * 257, 9 * 1025 and
9 * 2049, beside torch.linalg.cholesky_ex + torch.cholesky_solve on the same matrices in the same process.  Recorded, not gated: there is
no target ratio.

The matrix is A = G G^T / n + I (G seeded normal), well conditioned: the time of a Cholesky does not depend on the values.  Per size:
two warm-up calls of each solver, then `reps` rounds that ALTERNATE the two solvers, each call between a pair of HIP events on the
current stream (the calls only enqueue; the second event's synchronise ends the window); the median and the spread are reported.  The
window of one solver at one size is reps x its time: reps is chosen so that it is at least about half a second.  The factor's flop count
is n^3 / 3 (the matrix-core share of the work; the O(n^2) solves are not counted), and the fraction of peak is that over the factor's own
time over the FP64 matrix peak of AMD's public MI355X data sheet, 78.6 TFLOP/s (at the 2.4 GHz peak engine clock).  The shader clock
levels the driver reports before and after the timed windows are noted as read from sysfs (pp_dpm_sclk, read only) where visible.

    python scripts/dense_chol_bench.py [--out profiles/dense_chol_bench.json] [--sizes 257,1025,2049]
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MATRIX_PEAK_TFLOPS = 78.6
PEAK_SOURCE = 'AMD Instinct MI355X data sheet (public): peak FP64 matrix 78.6 TFLOP/s at 2.4 GHz'


def clock_state():
    """The current shader clock level per card as the driver lists it (the starred line of pp_dpm_sclk), or why it is not known."""
    out = {}
    for p in sorted(glob.glob('/sys/class/drm/card*/device/pp_dpm_sclk')):
        try:
            cur = [l.strip() for l in open(p) if '*' in l]
            out[p.split('/')[4]] = cur[0] if cur else 'no current level listed'
        except OSError as e:
            out[p.split('/')[4]] = 'unreadable: %s' % e
    return out or 'pp_dpm_sclk not visible to this process'


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def bench_size(N, dev):
    import numpy as np
    import torch
    from islam_amd import ops
    n = 9 * N
    g = torch.Generator(device=dev).manual_seed(N)
    G = torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)
    A = G @ G.t() / n
    del G
    A.diagonal().add_(1.0)
    A = 0.5 * (A + A.t())
    b = torch.randn((n,), dtype=torch.float64, device=dev, generator=g)
    d = A.diagonal().clone()
    Ah = A.clone()                     # the array the project's solver factors in place; its upper triangle stays A's
    ws = ops.dense_chol_workspace(n, dev)

    def hip_factor():
        return ops.dense_chol_factor(Ah, d, ws)

    def hip_both():
        info = ops.dense_chol_factor(Ah, d, ws)
        return info, ops.dense_chol_solve(Ah, b, ws)

    def torch_factor():
        return torch.linalg.cholesky_ex(A)

    def torch_both():
        L, info = torch.linalg.cholesky_ex(A)
        return info, torch.cholesky_solve(b[:, None], L)[:, 0]

    for _ in range(2):
        for fn in (hip_both, torch_both, hip_factor, torch_factor):
            fn()
    torch.cuda.synchronize()
    t_hip, _ = timed(hip_both)
    reps = int(min(200, max(5, round(500.0 / max(t_hip, 1e-3)))))
    ms = {k: [] for k in ('hip_factor_solve', 'torch_factor_solve', 'hip_factor', 'torch_factor')}
    for _ in range(reps):
        t, (ih, xh) = timed(hip_both)
        ms['hip_factor_solve'].append(t)
        t, (it, xt) = timed(torch_both)
        ms['torch_factor_solve'].append(t)
        ms['hip_factor'].append(timed(hip_factor)[0])
        ms['torch_factor'].append(timed(torch_factor)[0])
    assert int(ih.item()) == 0 and int(it.item()) == 0
    res = float((A @ xh - b).norm() / b.norm())
    res_t = float((A @ xt - b).norm() / b.norm())
    flop = n ** 3 / 3.0
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v))}
    out = {'N': N, 'n': n, 'reps': reps, 'factor_flop': flop, 'launches': {'factor': 3 * -(-n // 64) - 1, 'solve': 2 * -(-n // 64)}}
    for k, v in ms.items():
        out[k] = stat(v)
    for k in ('hip', 'torch'):
        tf = flop / (out[k + '_factor']['median_ms'] * 1e-3) / 1e12
        out[k + '_factor']['tflops'] = tf
        out[k + '_factor']['frac_of_fp64_matrix_peak'] = tf / FP64_MATRIX_PEAK_TFLOPS
    out['torch_over_hip_factor_solve'] = out['torch_factor_solve']['median_ms'] / out['hip_factor_solve']['median_ms']
    out['relative_residual'] = {'hip': res, 'torch': res_t, 'x_max_abs_diff': float((xh - xt).abs().max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', default='257,1025,2049')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'dense_chol_bench.py needs the GPU'
    dev = torch.device('cuda:0')
    out = {'what': 'islam_dense_chol_factor + _solve vs torch.linalg.cholesky_ex + cholesky_solve, fp64, HIP events, alternating',
           'device': torch.cuda.get_device_name(0), 'peak_tflops': FP64_MATRIX_PEAK_TFLOPS, 'peak_source': PEAK_SOURCE,
           'clock_before': clock_state(), 'sizes': []}
    for N in [int(s) for s in args.sizes.split(',')]:
        out['sizes'].append(bench_size(N, dev))
        print(json.dumps(out['sizes'][-1]), flush=True)
    out['clock_after'] = clock_state()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
