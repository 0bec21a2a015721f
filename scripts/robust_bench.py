"""Cost of the robust kernels on the chain LM: microseconds per LM iteration (wall time of whole
islam_pvgo_run_chain calls / their trials) on bench.py's graph from its dead-reckoning start, in the modes
  default        the loop run_pvgo takes without a kernel (fused trial + elimination above N = 96, one-launch loop up to N = 16),
  no_fuse        ISLAM_PVGO_NO_FUSE=1: the launch-per-stage loop (still the one-launch loop up to N = 16),
  no_fuse_small  ISLAM_PVGO_NO_FUSE=1 ISLAM_PVGO_NO_SMALL=1: the launch-per-stage loop at every size,
  huber          Huber(0.1) on all four factor groups: the launch-per-stage loop with the robust kernel variants,
  huber_inactive Huber(1e6): the same kernels with c = 1 everywhere, so the LM takes no_fuse_small's trajectory (same trials,
                 same rejects): the difference is the kernels' own cost.
One JSON line per size.    python scripts/robust_bench.py [--runs 12] [N ...]   (default N = 9 5001 300007)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from islam_amd import ops
from islam_amd.robust import Huber, parse_kernel

MODES = {'default': ({}, None), 'no_fuse': ({'ISLAM_PVGO_NO_FUSE': '1'}, None),
         'no_fuse_small': ({'ISLAM_PVGO_NO_FUSE': '1', 'ISLAM_PVGO_NO_SMALL': '1'}, None), 'huber': ({}, Huber(0.1)),
         'huber_inactive': ({}, Huber(1e6))}


def us_per_iter(prob, prm, robust, runs, device):
    """Wall time of `runs` whole LM runs (after two warm-up runs) divided by their trials; every run starts from the same state."""
    N = prob['init_nodes'].shape[0]
    ws = ops.pvgo_workspace(N, device)
    states = [(prob['init_nodes'].clone(), prob['init_vels'].clone()) for _ in range(runs + 2)]
    trials = 0
    for i, (nodes, vels) in enumerate(states):
        if i == 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        res, _ = ops.pvgo_run_chain(nodes, vels, prob['vo'], prob['drots'], prob['dtrans'], prob['dvels'], prob['dts'], prm, workspace=ws,
                                    robust=robust)
        if i >= 2:
            trials += res.trials
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return el / trials * 1e6, trials / runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=12)
    ap.add_argument('sizes', type=int, nargs='*', default=[9, 5001, 300007])
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for N in a.sizes:
        prob, _ = bench.build_problem(dev, N)
        prm = ops.pvgo_default_params(bench.LOSS_WEIGHT)
        out = {'N': int(prob['init_nodes'].shape[0])}
        for name, (env, kernel) in MODES.items():
            saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                us, it = us_per_iter(prob, prm, parse_kernel(kernel), a.runs, dev)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            out[name] = {'us_per_lm_iter': round(us, 2), 'lm_iters_per_run': it}
        out['huber_over_no_fuse'] = round(out['huber']['us_per_lm_iter'] / out['no_fuse']['us_per_lm_iter'], 3)
        out['huber_over_no_fuse_small'] = round(out['huber']['us_per_lm_iter'] / out['no_fuse_small']['us_per_lm_iter'], 3)
        out['huber_inactive_over_no_fuse_small'] = round(out['huber_inactive']['us_per_lm_iter'] / out['no_fuse_small']['us_per_lm_iter'], 3)
        out['runs'] = a.runs
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
