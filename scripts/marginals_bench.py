"""Device time of islam_pvgo_marginals against one islam_pvgo_solve_chain on the same matrix (the undamped Gauss-Newton matrix of
bench.py's graph at its dead-reckoning start, anchored at node 0).  HIP events around every call, warmed up, median of the passes;
one JSON line per size.    python scripts/marginals_bench.py [--passes 20] [N ...]   (default N = 9 5001 300007)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from islam_amd import ops
from islam_amd._lib import IslamHipError


def timed(fn, passes, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(passes)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--passes', type=int, default=20)
    ap.add_argument('sizes', type=int, nargs='*', default=[9, 5001, 300007])
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for N in a.sizes:
        prob, _ = bench.build_problem(dev, N)
        n = prob['init_nodes'].shape[0]
        lin, _ = ops.pvgo_linearize(prob['init_nodes'], prob['init_vels'], prob['vo'], prob['drots'], prob['dtrans'],
                                    prob['dvels'], prob['dts'])
        w4 = [float(w) ** 2 for w in bench.LOSS_WEIGHT]
        Hd, Ho, rhs = ops.pvgo_build_normal(lin, prob['dts'], n, w4, vmin=0.0, vmax=float('inf'))
        mws = ops.pvgo_marginals_workspace(n, dev)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        matrix = 'undamped'
        try:
            ops.pvgo_marginals(Hd, Ho, anchor=0, workspace=mws)                # synchronous once: raises if not PD
        except IslamHipError:
            # the undamped matrix of a very long chain anchored at one end is not positive definite in fp64 (its drift grows
            # ~N^3): time the same structure on the matrix of the LM's first damped step, A + 1e-4 diag(A) (the cost does not
            # depend on the values)
            matrix = 'A + 1e-4 diag(A) (undamped: ISLAM_ENOTPD)'
            Hd = Hd + torch.diag_embed(torch.diagonal(Hd, dim1=1, dim2=2) * 1e-4)
            ops.pvgo_marginals(Hd, Ho, anchor=0, workspace=mws)
        t_marg = timed(lambda: ops.pvgo_marginals(Hd, Ho, anchor=0, workspace=mws, status=status), a.passes)
        assert int(status.item()) == 0
        # the solve on the same matrix, the pose DoF of node 0 pinned like the anchor (solve_chain needs a PD matrix)
        Ha = Hd.clone()
        Ha[0, :6, :] = 0.0
        Ha[0, :, :6] = 0.0
        Ha[0, :6, :6] = torch.eye(6, dtype=torch.float64, device=dev)
        Hoa = Ho.clone()
        Hoa[0, :6, :] = 0.0
        sws = ops.pvgo_workspace(n, dev)
        ops.pvgo_solve_status(n, sws, dev)
        t_solve = timed(lambda: ops.pvgo_solve_chain_enqueue(Ha, Hoa, rhs, sws, damping=0.0), a.passes)
        try:
            ops.pvgo_solve_status(n, sws, dev)
        except IslamHipError:
            matrix += '; solve: ISLAM_ENOTPD'
        levels = ops.pvgo_marginals_plan(n)
        print(json.dumps({'N': n, 'marginals_us': round(t_marg, 1), 'solve_chain_us': round(t_solve, 1),
                          'ratio': round(t_marg / t_solve, 2), 'launches': 2 * len(levels) if len(levels) > 1 else 1,
                          'levels': [list(l) for l in levels], 'matrix': matrix, 'passes': a.passes}), flush=True)


if __name__ == '__main__':
    main()
