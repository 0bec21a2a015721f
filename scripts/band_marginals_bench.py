"""Cost and agreement of the band covariances of loop-closure graphs (pvgo_marginals_general(method='band')) on
the graphs of scripts/loop_closure_bench.py: N = 3000 with 6 closures, 5001 with 24, 50 001 with 12.  Recorded, not gated.

Timed, per graph, after two warm-up calls of everything: the whole call (host clock around a call that ends in its one read-back, plus a
device synchronise inside the window), and apart from it, between HIP events with the synchronise inside the window, the column solves
(islam_pvgo_band_inverse_columns, R columns), the projection + blocks (islam_pvgo_band_cov_blocks) and one chain solve
(islam_pvgo_solve_chain_enqueue) of the same band -- the unit of the prediction "R x one chain solve".  Medians of `--reps` rounds.  Where
N <= 12 000, method='dense' is timed in the same process, the two ALTERNATING; there is no earlier version of the band call to compare with.
Agreement: worst |band - dense| / (largest entry of the dense block's column) over the node and pair blocks at N = 65, 200, 513, 1025,
3000 (nothing is asserted here; at N = 200 and 513 tests/test_real_matrix_accuracy_gpu.py measures both sides against a double-double
reference: the error is the band formula's, the dense path is at LAPACK's floor).

    python scripts/band_marginals_bench.py [--out profiles/band_marginals_bench.json] [--graphs 3000:6,5001:24,50001:12] [--agree 65:3,...]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.dense_chol_bench import clock_state, timed      # noqa: E402

LW = (1, 0.1, 10, 0.1)
DENSE_MAX_NODES = 12000


def closure_problem(F, nclose):
    """The generator of scripts/loop_closure_bench.py: nclose chain edges replaced by random long-range ones (seed 1)."""
    import numpy as np
    import torch
    from oracle import lie
    from tests.helpers import chain_problem
    prob, tr = chain_problem(F)
    links, vo = prob['links'].copy(), prob['vo_motions'].copy()
    gt = np.concatenate([tr['gt_pos'], tr['gt_quat']], 1)
    rng = np.random.default_rng(1)
    for e in rng.choice(F - 1, nclose, replace=False):
        i, j = rng.choice(F, 2, replace=False)
        if abs(int(i) - int(j)) < 2:
            j = (i + F // 2) % F
        links[e] = (i, j)
        vo[e] = lie.se3_mul(lie.se3_mul(lie.se3_inv(gt[i]), gt[j]), lie.se3_exp(rng.normal(0, 0.01, 6)))
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device='cuda')
    return dict(nodes=t(prob['init_nodes']), vels=t(prob['init_vels']), vo_motions=t(vo),
                links=torch.tensor(links, dtype=torch.int64, device='cuda'), dts=t(prob['dts']), imu_drots=t(prob['imu_drots']),
                imu_dtrans=t(prob['imu_dtrans']), imu_dvels=t(prob['imu_dvels']))


def whole_call(d, method):
    import torch
    from islam_amd import pvgo
    from islam_amd._lib import IslamHipError
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        mg = pvgo.pvgo_marginals_general(**d, loss_weight=LW, method=method)
    except IslamHipError as e:                             # (ISLAM_ENOTPD: recorded; the call has done all its device work by then)
        mg = str(e)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, mg


def disagreement(band, dense):
    """worst |band - dense| / largest entry of the dense path's block column, over node and pair blocks"""
    import torch
    if isinstance(band, str) or isinstance(dense, str):
        return None
    col = dense.node_cov.abs().amax(dim=1).clamp_min(1e-300)               # (N, 9): the diagonal block stands for the column
    e = ((band.node_cov - dense.node_cov).abs() / col[:, None, :]).max()
    colp = torch.maximum(dense.pair_cov.abs().amax(dim=1), col[dense.pairs[:, 1]])
    return float(torch.maximum(e, ((band.pair_cov - dense.pair_cov).abs() / colp[:, None, :]).max()))


def band_parts(d):
    """The pieces marginals_band strings together, kept for timing them one by one."""
    import torch
    from islam_amd import ops
    from islam_amd import pvgo_dense as pd
    N, dev = d['nodes'].shape[0], d['nodes'].device
    eh = d['links'].cpu().numpy()
    g = pd._Graph(d['nodes'], d['links'], d['vo_motions'], d['imu_drots'], d['imu_dtrans'], d['imu_dvels'], d['dts'], LW)
    vo, lin = g.linearize(d['nodes'], d['vels'])
    band = pd._BandSystem(g, vo, lin, -pd._NOCLAMP, pd._NOCLAMP, pd._BandTopology(eh, N, dev))
    cols, Rc = pd.band_columns(N, eh, 0, eh)
    ws = ops.pvgo_band_inverse_workspace(N, cols.size, dev)
    sws = ops.pvgo_workspace(N, dev)
    try:
        ops.pvgo_solve_status(N, sws, dev)                # initialises the fresh workspace's status / hand-off words
    except Exception:
        pass
    Sd, So = ops.pvgo_marginals(band.Hd, band.Ho, anchor=0)
    status = torch.zeros((2,), dtype=torch.int32, device=dev)
    columns = lambda: ops.pvgo_band_inverse_columns(band.Hd, band.Ho, cols, 0, workspace=ws, status=status[0:1])
    Y = columns()
    G = pd._capacitance(band, eh[pd.off_band_edges(eh)], Y, cols, Rc, 0)
    blocks = lambda: ops.pvgo_band_cov_blocks(Sd, So, Y, cols, Rc, G, 0, eh, workspace=ws, status=status[1:2])
    rhs = torch.zeros((N, 9), dtype=torch.float64, device=dev)
    rhs[N // 2, 0] = 1.0
    Hd = band.Hd.clone()
    Hd[0, :6, :] = 0.0
    Hd[0, :, :6] = 0.0
    Hd[0, :6, :6] = torch.eye(6, dtype=torch.float64, device=dev)
    one_solve = lambda: ops.pvgo_solve_chain_enqueue(Hd, band.Ho, rhs, sws)
    selected = lambda: ops.pvgo_marginals(band.Hd, band.Ho, anchor=0, status=status[0:1])
    diag = torch.diagonal(blocks()[0], dim1=1, dim2=2).reshape(-1)[6:]     # every variance outside the anchor's pose
    return dict(R=int(cols.size), Rc=Rc, nonpositive=int((~(diag > 0)).sum()), variances=int(diag.numel()), columns=columns, blocks=blocks, one_solve=one_solve, selected_inverse=selected, status=status)


def bench_graph(N, nclose, reps, with_dense):
    import numpy as np
    import torch
    d = closure_problem(N, nclose)
    parts = band_parts(d)
    fns = {k: parts[k] for k in ('columns', 'blocks', 'one_solve', 'selected_inverse')}
    dense_on = with_dense and N <= DENSE_MAX_NODES
    for _ in range(2):                                     # warm-up: every shape the timed windows use
        whole_call(d, 'band')
        for fn in fns.values():
            fn()
    if dense_on:
        whole_call(d, 'dense')
    torch.cuda.synchronize()
    ms = {k: [] for k in ('band_whole_call', 'dense_whole_call', *fns)}
    torch.cuda.reset_peak_memory_stats()
    agree = None
    dense_reps = min(reps, 3)
    for r in range(reps):
        t, band = whole_call(d, 'band')
        ms['band_whole_call'].append(t)
        if r == 0:
            peak_band = torch.cuda.max_memory_allocated()
        if dense_on and r < dense_reps:
            t, dense = whole_call(d, 'dense')
            ms['dense_whole_call'].append(t)
            agree = disagreement(band, dense)
            del dense
        for k, fn in fns.items():
            ms[k].append(timed(fn)[0])
    stat = lambda v: {'median_ms': float(np.median(v)), 'min_ms': float(min(v)), 'max_ms': float(max(v)), 'reps': len(v)} if v else None
    out = {'N': N, 'closures': nclose, 'R': parts['R'], 'Rc': parts['Rc'], 'pairs': int(d['links'].shape[0]),
           'band_call': band if isinstance(band, str) else 'ok', 'status_columns_blocks': parts['status'].tolist(),
           'nonpositive_variances': [parts['nonpositive'], parts['variances']], 'peak_bytes_band_call': int(peak_band), 'dense_matrix_bytes': (9 * N) ** 2 * 8, 'band_vs_dense_worst_relative': agree}
    out.update({k: stat(v) for k, v in ms.items()})
    out['predicted_columns_ms'] = parts['R'] * out['one_solve']['median_ms']
    out['columns_over_prediction'] = out['columns']['median_ms'] / out['predicted_columns_ms']
    if out['dense_whole_call']:
        out['dense_over_band'] = out['dense_whole_call']['median_ms'] / out['band_whole_call']['median_ms']
    return out


def agreement(N, nclose):
    d = closure_problem(N, nclose)
    band, dense = whole_call(d, 'band')[1], whole_call(d, 'dense')[1]
    return {'N': N, 'closures': nclose, 'band_call': band if isinstance(band, str) else 'ok',
            'band_vs_dense_worst_relative': disagreement(band, dense)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--graphs', default='3000:6,5001:24,50001:12')
    ap.add_argument('--agree', default='65:3,200:4,513:6,1025:6,3000:6')
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--no-dense', action='store_true')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'band_marginals_bench.py needs the GPU'
    pairs = lambda s: [tuple(int(x) for x in g.split(':')) for g in s.split(',') if g]
    out = {'what': "pvgo_marginals_general(method='band') and its stages, fp64; method='dense' alternating where N <= 12000",
           'device': torch.cuda.get_device_name(0), 'clock_before': clock_state(), 'agreement': [], 'graphs': []}
    for N, k in pairs(args.agree):
        out['agreement'].append(agreement(N, k))
        print(json.dumps(out['agreement'][-1]), flush=True)
    for N, k in pairs(args.graphs):
        out['graphs'].append(bench_graph(N, k, args.reps, not args.no_dense))
        print(json.dumps(out['graphs'][-1]), flush=True)
    out['clock_after'] = clock_state()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
