"""Cost of islam_imu_extrinsic_rot_solve: us per call (float64, the residuals asked for, its 8-byte read-back
and synchronise included) at 5000 and at 300 007 pairs, with no reweighting (K = 0) and with four Huber rounds (K = 4), beside the bytes
the pair kernel must move per round (two quaternions in, twelve terms out per pair) and beside the numpy restatement of
tests/test_imu_extrinsic_gpu.py on one core (one run, K = 0; at 300 007 pairs on the first 20 000, scaled).  HIP events around every
call, 3 warm-up calls, the median of 20.  There is no earlier version to compare against and no target.  Every case runs in a child
process of its own under a time limit; a child that fails or runs out of time ends the script.

    python scripts/imu_extrinsic_bench.py [--out profiles/imu_extrinsic_bench.json]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'5000': 5000, 'N300007': 300007}
WHAT = ('K0', 'K4')
NUMPY_ROWS = 20000
PAIR_BYTES = 8 * (4 + 4 + 12)                               # float64: two quaternions read, twelve terms written


def child(case):
    import numpy as np
    import torch
    from islam_amd import ops
    from tests.test_imu_extrinsic_gpu import Q_TRUE, extrinsic_reference, qangle, qexp, qinv, qmul
    assert torch.cuda.is_available(), 'imu_extrinsic_bench.py needs the GPU'
    rows = CASES[case]
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(1)
    # the Huber data of the tests at this size: 2e-4 rad of noise on every body rotation, every tenth one corrupted
    qc = qexp(rng.normal(0.0, 0.05, (rows, 3)))
    qb = qmul(qmul(qmul(Q_TRUE, qc), qinv(Q_TRUE)), qexp(rng.normal(0.0, 2e-4, (rows, 3))))
    qb[::10] = qmul(qb[::10], qexp(rng.normal(0.0, 0.05, (len(qb[::10]), 3))))
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    b, c = t64(qb), t64(qc)
    fns = {'K0': lambda: ops.imu_extrinsic_rot_solve(b, c), 'K4': lambda: ops.imu_extrinsic_rot_solve(b, c, None, 1e-3, 4)}

    def median20(fn):
        us = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        us.sort()
        return 0.5 * (us[9] + us[10])

    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {w: median20(fns[w]) for w in WHAT}
    out['err_K0'], out['err_K4'] = (float(qangle(fns[w]()[0].cpu().numpy(), Q_TRUE)) for w in WHAT)
    out['pair_MB_per_round'] = PAIR_BYTES * rows / 1e6
    m = min(rows, NUMPY_ROWS)
    t0 = time.perf_counter()
    extrinsic_reference(qb[:m], qc[:m])
    out['numpy_one_core'] = (time.perf_counter() - t0) * 1e6 * rows / m
    out['numpy_rows'] = m
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        os.environ.setdefault('OMP_NUM_THREADS', '1')
        print('RESULT ' + json.dumps(child(sys.argv[2])))
        return
    rows = {}
    for case in CASES:
        env = dict(os.environ, OMP_NUM_THREADS='1', OPENBLAS_NUM_THREADS='1', MKL_NUM_THREADS='1')
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', case], capture_output=True, text=True, timeout=400, env=env)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit('%s failed with exit code %d: nothing more is started' % (case, r.returncode))
        rows[case] = json.loads([ln for ln in r.stdout.split('\n') if ln.startswith('RESULT ')][-1][7:])
    cols = WHAT + ('pair_MB_per_round', 'numpy_one_core', 'err_K0', 'err_K4')
    print('us per call: the median of 20 (numpy: one run on one core, K = 0, scaled from numpy_rows pairs); err: rad to the planted mount')
    print('| pairs | ' + ' | '.join(cols) + ' |')
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
