"""Cost of per-factor information on the chain LM: microseconds per LM trial (wall time of whole
islam_pvgo_run_chain[_info] calls / their trials) on bench.py's graph from its dead-reckoning start, in the modes
  default        the loop run_pvgo takes without information (fused trial + elimination above N = 96, one-launch loop up to N = 16),
  staged         ISLAM_PVGO_NO_FUSE=1 ISLAM_PVGO_NO_SMALL=1: the launch-per-stage loop at every size, scalar weights,
  info           information = loss_weight^2 I on every factor: the launch-per-stage loop with info_build_kernel behind every
                 linearisation.  The LM takes staged's trajectory (same trials, same rejects): the difference is the extra launch,
  info9          the same information as ONE 9x9 per link, blockdiag(lw1^2 I, lw2^2 I, lw3^2 I): the same loop
                 with info9_build_kernel, which reads 45 doubles per link where info_build_kernel reads 18, and the same trajectory,
and the assembly kernels alone, islam_pvgo_build_normal against islam_pvgo_build_normal_info and islam_pvgo_build_normal_info9 on the
same `lin` record: HIP events, warm-up, median of 20 launches.  One JSON line per size.
    python scripts/pvgo_info_bench.py [--runs 12] [N ...]   (default N = 9 5001 300007)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from islam_amd import ops
from islam_amd.information import PvgoInfo

STAGED = {'ISLAM_PVGO_NO_FUSE': '1', 'ISLAM_PVGO_NO_SMALL': '1'}
MODES = {'default': ({}, None), 'staged': (STAGED, None), 'info': ({}, 'info'), 'info9': ({}, 'info9')}


def us_per_trial(prob, prm, info, runs, device):
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
                                    info=info)
        if i >= 2:
            trials += res.trials
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return el / trials * 1e6, trials / runs


def kernel_us(fn, reps=20, warmup=5):
    """Median over `reps` launches of the time between two HIP events around fn()."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def assembly_us(prob, packed, packed9):
    """The three assembly launches alone, on preallocated outputs (the ops wrappers allocate theirs: not part of the kernel)."""
    from islam_amd._lib import c_double, check, lib, ptr, stream_ptr
    dev = prob['init_nodes'].device
    N = prob['init_nodes'].shape[0]
    lin, _ = ops.pvgo_linearize(prob['init_nodes'], prob['init_vels'], prob['vo'], prob['drots'], prob['dtrans'], prob['dvels'], prob['dts'])
    Hd, Ho = (torch.zeros((N, 9, 9), dtype=torch.float64, device=dev) for _ in range(2))
    rhs = torch.zeros((N, 9), dtype=torch.float64, device=dev)
    w = (c_double * 4)(*[float(x) ** 2 for x in bench.LOSS_WEIGHT[:4]])
    tail = (c_double(1e-4), c_double(1e32), ptr(Hd), ptr(Ho), ptr(rhs), stream_ptr(dev))
    scalar = lambda: check(lib().islam_pvgo_build_normal(ptr(lin), ptr(prob['dts']), N, w, *tail))
    info = lambda: check(lib().islam_pvgo_build_normal_info(ptr(lin), ptr(prob['dts']), N, ptr(packed[0]), ptr(packed[1]), *tail))
    info9 = lambda: check(lib().islam_pvgo_build_normal_info9(ptr(lin), ptr(prob['dts']), N, ptr(packed9[0]), ptr(packed9[1]), *tail))
    return kernel_us(scalar), kernel_us(info), kernel_us(info9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=12)
    ap.add_argument('sizes', type=int, nargs='*', default=[9, 5001, 300007])
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for N in a.sizes:
        prob, _ = bench.build_problem(dev, N)
        N = int(prob['init_nodes'].shape[0])
        prm = ops.pvgo_default_params(bench.LOSS_WEIGHT)
        packed = PvgoInfo().packed(N - 1, N - 1, bench.LOSS_WEIGHT, dev)
        w9 = np.diag(np.repeat(np.asarray(bench.LOSS_WEIGHT[1:4], dtype=np.float64) ** 2, 3))
        packed9 = PvgoInfo(imu=np.broadcast_to(w9, (N - 1, 9, 9)), validate=False).packed(N - 1, N - 1, bench.LOSS_WEIGHT, dev)
        assert tuple(packed9[1].shape) == (45, N - 1)
        given = {None: None, 'info': packed, 'info9': packed9}
        out = {'N': N}
        for name, (env, which) in MODES.items():
            saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                us, it = us_per_trial(prob, prm, given[which], a.runs, dev)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            out[name] = {'us_per_trial': round(us, 2), 'trials_per_run': it}
        out['info_minus_staged_us'] = round(out['info']['us_per_trial'] - out['staged']['us_per_trial'], 2)
        out['info_over_staged'] = round(out['info']['us_per_trial'] / out['staged']['us_per_trial'], 3)
        out['info_over_default'] = round(out['info']['us_per_trial'] / out['default']['us_per_trial'], 3)
        out['info9_minus_info_us'] = round(out['info9']['us_per_trial'] - out['info']['us_per_trial'], 2)
        out['info9_over_info'] = round(out['info9']['us_per_trial'] / out['info']['us_per_trial'], 3)
        s_us, i_us, i9_us = assembly_us(prob, packed, packed9)
        out['build_normal_us'], out['build_normal_info_us'], out['build_normal_info9_us'] = round(s_us, 2), round(i_us, 2), round(i9_us, 2)
        out['runs'] = a.runs
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
