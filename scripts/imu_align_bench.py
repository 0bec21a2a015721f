"""Cost of islam_imu_gravity_bias_solve: us per call (float64, its 8-byte read-back and synchronise
included) with Jacobians, with Jacobians and covariances, and with the gravity norm, at 5000 frames x 10 samples and at N = 300 007
rows, beside islam_imu_gyro_bias_solve on the same rows IN THE SAME PROCESS and beside the numpy restatement of
tests/test_imu_align_gpu.py on one core (one run; at N = 300 007 on the first 20 000 rows, scaled).  HIP events around every call,
3 warm-up calls, the median of 20.  Two builds are compared by running the script once per build, alternating, with ISLAM_HIP_LIB
naming the other library (profiles/imu_align_bench.json: the solve as a file of its own against the NX = 6 instantiation of
csrc/imu_align.hip's kernel family); the expectation to check is "within a small
multiple of the gyro-bias solve at 5000 rows; the large case not serial in one workgroup".  Every case runs in a child process of its
own under a time limit; a child that fails or runs out of time ends the script.

    python scripts/imu_align_bench.py [--out profiles/imu_align_bench.json]
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'5000x10': 5000, 'N300007': 300007}
WHAT = ('align', 'align_cov', 'align_cov_norm', 'gyro_bias_solve')
NUMPY_ROWS = 20000


def child(case):
    import numpy as np
    import torch
    from islam_amd import ops
    from tests.test_imu_align_gpu import align_reference
    assert torch.cuda.is_available(), 'imu_align_bench.py needs the GPU'
    rows = CASES[case]
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(1)
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    if case == '5000x10':                                   # the rows of a real stream: increments, Jacobians and covariances of the library
        from islam_amd import synthetic
        from scripts.imu_cov_bench import ACC_COV, GYRO_COV
        tr = synthetic.car_trajectory(rows + 1, imu_per_frame=10, seed=1)
        seg_h = np.ascontiguousarray(tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0], dtype=np.int64)
        seg_d = torch.tensor(seg_h, device=dev)
        S = int(seg_h[-1])
        # the car turns about one axis only, which leaves b and g along that axis inseparable: a three-axis sway is added
        tt = np.cumsum(tr['imu_dts'][:S])
        sway = 0.5 * np.stack([np.sin(1.3 * tt + 0.2), np.sin(0.7 * tt + 1.1), np.sin(2.1 * tt + 0.5)], 1)
        dt, gyro, acc = t64(tr['imu_dts'][:S]), t64(tr['gyros'][:S] + sway), t64(tr['accels'][:S])
        z3, q0 = t64(np.zeros(3)), t64([0.0, 0.0, 0.0, 1.0])
        world, motion, _ = ops.imu_preint_both(dt, gyro, acc, seg_d, seg_h, z3, q0, z3, 0.0)
        jac = ops.imu_preint_bias_jac(dt, gyro, acc, seg_d, seg_h, True)
        cov = ops.imu_preint_cov(dt, gyro, acc, seg_d, seg_h, GYRO_COV, ACC_COV, True)
        dur = t64(np.add.reduceat(tr['imu_dts'][:S], seg_h[:-1]))
        quat, rot_m = world[1].contiguous(), motion[1].contiguous()
        from islam_amd import lietensor as pp
        R0t = pp._qmat(quat[:rows]).transpose(-1, -2)
        dvel = (R0t @ motion[2].unsqueeze(-1)).squeeze(-1).contiguous()
        dpos = (R0t @ motion[0].unsqueeze(-1)).squeeze(-1).contiguous()
        # positions that satisfy (P_i), (V_i) for a planted g: the dead-reckoned ones
        g = np.array([0.0, 0.0, -9.81])
        dn, R = dur.cpu().numpy(), pp._qmat(quat).cpu().numpy()
        p, v = np.zeros((rows + 1, 3)), np.array([1.0, 0.0, 0.0])
        dvn, dpn = dvel.cpu().numpy(), dpos.cpu().numpy()
        for i in range(rows):
            p[i + 1] = p[i] + v * dn[i] + 0.5 * g * dn[i] ** 2 + R[i] @ dpn[i]
            v = v + g * dn[i] + R[i] @ dvn[i]
        pos = t64(p)
    else:                                                   # rows of the same sizes, made up: the cost does not depend on the values
        q = rng.normal(0, 1, (rows + 1, 4))
        quat = t64(q / np.linalg.norm(q, axis=1, keepdims=True))
        rot_m = quat[:rows].contiguous()
        pos, dur = t64(np.cumsum(rng.normal(0, 0.1, (rows + 1, 3)), 0)), t64(rng.uniform(0.04, 0.06, rows))
        dvel, dpos = t64(rng.normal(0, 0.5, (rows, 3))), t64(rng.normal(0, 0.02, (rows, 3)))
        J = np.zeros((rows, 9, 6))
        J[:, 0:3, 0:3] = J[:, 3:6, 3:6] = -0.05 * np.eye(3) + rng.normal(0, 1e-3, (rows, 3, 3))
        J[:, 6:9, 3:6] = -0.00125 * np.eye(3) + rng.normal(0, 1e-5, (rows, 3, 3))
        jac = t64(J)
        A = rng.normal(0, 1e-3, (rows, 9, 9))
        cov = t64(A @ A.transpose(0, 2, 1) + 1e-8 * np.eye(9))
    ref = quat[1:].contiguous()
    a = (quat, pos, dur, dvel, dpos)
    fns = {'align': lambda: ops.imu_gravity_bias_solve(*a, jac),
           'align_cov': lambda: ops.imu_gravity_bias_solve(*a, jac, cov),
           'align_cov_norm': lambda: ops.imu_gravity_bias_solve(*a, jac, cov, None, 9.81),
           'gyro_bias_solve': lambda: ops.imu_gyro_bias_solve(jac, rot_m, ref)}

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
    m = min(rows, NUMPY_ROWS)
    h = [t[:m + 1].cpu().numpy() for t in a[:2]] + [t[:m].cpu().numpy() for t in a[2:]]
    t0 = time.perf_counter()
    align_reference(*h, jac[:m].cpu().numpy())
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
    cols = WHAT + ('numpy_one_core',)
    print('us per call: the median of 20 (numpy: one run on one core, scaled from numpy_rows rows)')
    print('| rows | ' + ' | '.join(cols) + ' |')
    print('|---|' + '---|' * len(cols))
    for case in CASES:
        print('| %s | ' % case + ' | '.join('%.1f' % rows[case][w] for w in cols) + ' |')
    line = json.dumps(rows)
    print(line)
    if len(sys.argv) == 3 and sys.argv[1] == '--out':
        with open(sys.argv[2], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
