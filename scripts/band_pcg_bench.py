"""Wall time of run_pvgo(general_solver='band_pcg') on a long trajectory with six loop closures.

The graph is that of tests/test_surface_gpu.py::test_general_topology_long_chain_with_loop_closures (3000 frames): with
--closures replaced the six long edges take the place of six chain edges (E = N - 1), with --closures added they are appended
(E = N + 5).  Per process: two warm-up runs, then --reps runs, each ended by a device synchronise; the median, minimum and maximum
of the wall times, the same divided by the LM trials and by the PCG iterations of a run, and, apart from the LM, the time of one
assembly of the band system and of one matrix-vector product (the two pieces the PCG loop calls), each over a window of many
calls between two synchronises.  One JSON line.  --package-root DIR imports islam_amd from DIR (a built tree of another commit), so
that two commits can be timed alternately from one shell loop:
    for i in 1 2 3; do python scripts/band_pcg_bench.py --package-root ../parent; python scripts/band_pcg_bench.py; done"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOSURES = {100: (0, 2900), 700: (350, 2100), 1300: (1299, 40), 1900: (2500, 600), 2400: (10, 1500), 2800: (2999, 1)}
LW = (1, 0.1, 10, 0.1)


def problem(F, how, seed=9):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle import lie
    from tests.helpers import chain_problem
    prob, tr = chain_problem(F)
    links, vo = prob['links'].copy(), prob['vo_motions'].copy()
    gt = np.concatenate([tr['gt_pos'], tr['gt_quat']], 1)
    rng = np.random.default_rng(seed)
    for e, (i, j) in CLOSURES.items():
        rel = lie.se3_mul(lie.se3_mul(lie.se3_inv(gt[i]), gt[j]), lie.se3_exp(rng.normal(0, 0.01, 6)))
        if how == 'replaced':
            links[e], vo[e] = (i, j), rel
        else:
            links, vo = np.concatenate([links, [[i, j]]]), np.concatenate([vo, rel[None]])
    return dict(prob, links=links, vo_motions=vo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--closures', choices=('replaced', 'added'), default='replaced')
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--package-root', default=ROOT)
    ap.add_argument('--label', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('band_pcg_bench needs the GPU: a CPU run gives no time')
    import islam_amd
    from islam_amd import lietensor as pp, pvgo_dense
    from islam_amd.pvgo import run_pvgo
    p = problem(a.frames, a.closures)
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    args = (pp.SE3(t(p['init_nodes'])), t(p['init_vels']), pp.SE3(t(p['vo_motions']).to('cuda')), torch.tensor(p['links']), t(p['dts']),
            pp.SO3(t(p['imu_drots'])), t(p['imu_dtrans']), t(p['imu_dvels']))
    run = lambda: run_pvgo(*args, device='cuda', loss_weight=LW, general_solver='band_pcg', return_info=True)
    for _ in range(2):
        out = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = run()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    info = out[5]
    # the two pieces on their own, at the initial state
    d = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device='cuda')
    nodes, vels = d(p['init_nodes']), d(p['init_vels'])
    g = pvgo_dense._lm_graph(nodes, torch.tensor(p['links'], device='cuda'), d(p['vo_motions']), d(p['imu_drots']), d(p['imu_dtrans']),
                             d(p['imu_dvels']), d(p['dts']), LW, None, None)
    sysm = pvgo_dense._BandPcgSystem(g, 1e-4, 1e32)
    vo, lin = g.linearize(nodes, vels)

    def window(fn, n):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / n

    asm = [window(lambda: sysm.assemble(vo, lin, None, None, None), 200) for _ in range(3)]
    x = torch.randn((a.frames, 9), dtype=torch.float64, device='cuda')
    mv = [window(lambda: sysm.band.matvec(x), 1000) for _ in range(3)]
    med = statistics.median(ms)
    print(json.dumps(dict(label=a.label or os.path.abspath(a.package_root), package=os.path.dirname(islam_amd.__file__), closures=a.closures,
                          N=a.frames, E=int(p['links'].shape[0]), reps=a.reps, run_ms=dict(median=med, min=min(ms), max=max(ms)),
                          steps=info['steps'], trials=info['trials'], pcg_iterations=info['pcg_iterations'],
                          ms_per_trial=med / info['trials'], us_per_pcg_iteration=1e3 * med / max(info['pcg_iterations'], 1),
                          assemble_us=dict(median=statistics.median(asm), min=min(asm), max=max(asm)),
                          matvec_us=dict(median=statistics.median(mv), min=min(mv), max=max(mv)), loss=info['loss'])), flush=True)


if __name__ == '__main__':
    main()
