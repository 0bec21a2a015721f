"""Cost of the covariance step of the dense path (islam_dense_chol_invert_factor + islam_pvgo_dense_cov_blocks) at
n = 9 * 257 and 9 * 1025 (and 9 * 2049 on request), beside torch.cholesky_inverse of the same factor in the same process.  Recorded, not
gated: there is no target ratio.

The matrix is A = G G^T / n + I (G seeded normal), well conditioned; it is factored once by islam_dense_chol_factor.  The inverse works in
place, so every timed call of it starts from a fresh copy of the factor made OUTSIDE the timed window; torch.cholesky_inverse reads the
same factor (its lower triangle) and returns a second n x n array with all of Sigma.  Requested from the project's path: all N diagonal
blocks and the N - 1 neighbour pairs plus the two end-to-end pairs -- what run_pvgo(marginals=True) asks for on a chain with one closure.
Per size: two warm-up calls of each, then `reps` rounds that ALTERNATE the two, each call between a pair of HIP events on the current stream
(the calls only enqueue; the second event's synchronise ends the window); the median and the spread are reported.  Flop counts: the
triangular inverse n^3 / 3 (matrix cores), the blocks 2 * 81 * n / 2 per block on average (vector units); torch's POTRI n^3 * 2 / 3.

    python scripts/dense_marginals_bench.py [--out profiles/dense_marginals_bench.json] [--sizes 257,1025]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.dense_chol_bench import FP64_MATRIX_PEAK_TFLOPS, PEAK_SOURCE, clock_state, timed      # noqa: E402


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
    d = A.diagonal().clone()
    assert int(ops.dense_chol_factor(A, d).item()) == 0               # L in the lower triangle, A's entries above it
    L = A
    W = torch.empty_like(L)
    ws = ops.dense_chol_inverse_workspace(n, dev)
    pairs = np.concatenate([np.stack([np.arange(N - 1), np.arange(1, N)], 1), [[0, N - 1], [N - 1, 0]]]).astype(np.int64)

    def hip_invert():
        return ops.dense_chol_invert_factor(W, ws)

    def hip_both():
        ops.dense_chol_invert_factor(W, ws)
        return ops.pvgo_dense_cov_blocks(W, None, pairs)

    def torch_inverse():
        return torch.cholesky_inverse(L)

    torch_error = None
    for _ in range(2):
        for fn in (hip_both, hip_invert):
            W.copy_(L)
            fn()
        try:
            torch_inverse()
        except RuntimeError as e:                  # (the solver library behind torch refuses some sizes: recorded, the project's side is still timed)
            torch_error = str(e).split('\n')[0][:300]
            break
    torch.cuda.synchronize()
    W.copy_(L)
    t_hip, _ = timed(hip_both)
    reps = int(min(100, max(5, round(500.0 / max(t_hip, 1e-3)))))
    ms = {k: [] for k in ('hip_invert_blocks', 'hip_invert', 'torch_cholesky_inverse')}
    for _ in range(reps):
        W.copy_(L)
        t, (node, pair) = timed(hip_both)
        ms['hip_invert_blocks'].append(t)
        W.copy_(L)
        ms['hip_invert'].append(timed(hip_invert)[0])
        if torch_error is None:
            t, S = timed(torch_inverse)
            ms['torch_cholesky_inverse'].append(t)
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v))}
    nb = -(-n // 64)
    out = {'N': N, 'n': n, 'reps': reps, 'blocks': {'node': N, 'pair': len(pairs)},
           'launches': {'invert': 2 * nb - 1, 'blocks': 1 + -(-len(pairs) // 384)},
           'flop': {'triangular_inverse': n ** 3 / 3.0, 'blocks': 81.0 * n * (N + len(pairs)), 'torch_potri': 2.0 * n ** 3 / 3.0}}
    for k, v in ms.items():
        out[k] = stat(v) if v else {'error': torch_error}
    tf = out['flop']['triangular_inverse'] / (out['hip_invert']['median_ms'] * 1e-3) / 1e12
    out['hip_invert']['tflops'] = tf
    out['hip_invert']['frac_of_fp64_matrix_peak'] = tf / FP64_MATRIX_PEAK_TFLOPS
    if torch_error is None:
        idx = torch.arange(N, device=dev)
        Sn = S.view(N, 9, N, 9)[idx, :, idx, :]
        Sp = S.view(N, 9, N, 9)[idx[:-1], :, idx[1:], :]
        scale = float(S.abs().max())
        out['torch_over_hip'] = out['torch_cholesky_inverse']['median_ms'] / out['hip_invert_blocks']['median_ms']
        out['max_abs_diff_over_max_abs'] = {'node': float((node - Sn).abs().max()) / scale,
                                            'neighbour': float((pair[:N - 1] - Sp).abs().max()) / scale}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--sizes', default='257,1025')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'dense_marginals_bench.py needs the GPU'
    dev = torch.device('cuda:0')
    out = {'what': 'islam_dense_chol_invert_factor + islam_pvgo_dense_cov_blocks vs torch.cholesky_inverse of the same factor, fp64, HIP '
                   'events, alternating',
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
