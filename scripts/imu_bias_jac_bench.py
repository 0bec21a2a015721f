"""Cost of islam_imu_preint_bias_jac: us per call in world and motion mode at 5000 frames x 10 samples and
at 4 frames x 200 samples (float64), beside islam_imu_preint_cov and islam_imu_preint_both on the same stream IN THE SAME PROCESS,
and beside islam_imu_bias_correct / islam_imu_gyro_bias_solve on the motion rows.  HIP events around every call, 3 warm-up calls,
the median of 20; the block of medians is taken three times, alternating the calls, and the spread of a call's three medians is
printed beside it: a difference between two calls below that spread is not a difference.  Every case runs in a child process of its
own under a time limit; a child that fails or runs out of time ends the script.

    python scripts/imu_bias_jac_bench.py       # the table, and the launches / dependent joins of each mode
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.imu_cov_bench import ACC_COV, CASES, GYRO_COV, depth        # the launch structure is imu_cov.hip's      # noqa: E402

WHAT = ('jac_world', 'jac_motion', 'cov_world', 'cov_motion', 'preint_both', 'bias_correct', 'gyro_bias_solve')
REPEATS = 3


def child(case):
    import numpy as np
    import torch
    from islam_amd import ops, synthetic
    assert torch.cuda.is_available(), 'imu_bias_jac_bench.py needs the GPU'
    frames, per = CASES[case]
    tr = synthetic.car_trajectory(frames, imu_per_frame=per, seed=1)
    seg_h = np.ascontiguousarray(tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0], dtype=np.int64)
    dev = torch.device('cuda:0')
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    seg_d = torch.tensor(seg_h, device=dev)
    dt, gyro, acc = t64(tr['imu_dts']), t64(tr['gyros']), t64(tr['accels'])
    ip, ir, iv = t64(tr['init']['pos']), t64(tr['init']['rot']), t64(tr['init']['vel'])
    jac = ops.imu_preint_bias_jac(dt, gyro, acc, seg_d, seg_h, True)
    pos, rot, vel = ops.imu_preint(dt, gyro, acc, seg_d, seg_h, ip, ir, iv, 0.0, True)
    ref = ops.imu_preint(dt, gyro + 0.01, acc, seg_d, seg_h, ip, ir, iv, 0.0, True)[1]
    dbg, dba = np.array([1e-3, -2e-3, 5e-4]), np.array([1e-2, 2e-2, -1e-2])
    fns = {'jac_world': lambda: ops.imu_preint_bias_jac(dt, gyro, acc, seg_d, seg_h, False),
           'jac_motion': lambda: ops.imu_preint_bias_jac(dt, gyro, acc, seg_d, seg_h, True),
           'cov_world': lambda: ops.imu_preint_cov(dt, gyro, acc, seg_d, seg_h, GYRO_COV, ACC_COV, False),
           'cov_motion': lambda: ops.imu_preint_cov(dt, gyro, acc, seg_d, seg_h, GYRO_COV, ACC_COV, True),
           'preint_both': lambda: ops.imu_preint_both(dt, gyro, acc, seg_d, seg_h, ip, ir, iv, tr['gravity']),
           'bias_correct': lambda: ops.imu_bias_correct(jac, rot, vel, pos, dbg, dba),
           'gyro_bias_solve': lambda: ops.imu_gyro_bias_solve(jac, rot, ref)}       # (includes its 8-byte read-back and synchronise)

    def median20(fn):
        us = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1e3)
        us.sort()
        return 0.5 * (us[9] + us[10])

    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    med = {w: [] for w in WHAT}
    for _ in range(REPEATS):
        for w in WHAT:
            med[w].append(median20(fns[w]))
    return {w: {'us': sorted(v)[REPEATS // 2], 'lo': min(v), 'hi': max(v)} for w, v in med.items()}


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        print('RESULT ' + json.dumps(child(sys.argv[2])))
        return
    rows = {}
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', case], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit('%s failed with exit code %d: nothing more is started' % (case, r.returncode))
        rows[case] = json.loads([ln for ln in r.stdout.split('\n') if ln.startswith('RESULT ')][-1][7:])
    print('us per call: the median of %d medians of 20 (lowest .. highest median)' % REPEATS)
    print('| frames x samples | ' + ' | '.join(WHAT) + ' |')
    print('|---|' + '---|' * len(WHAT))
    for case in CASES:
        print('| %s | ' % case + ' | '.join('%.1f (%.1f .. %.1f)' % (rows[case][w]['us'], rows[case][w]['lo'], rows[case][w]['hi']) for w in WHAT) + ' |')
    for case, (frames, per) in CASES.items():
        d = depth(frames - 1, per)
        print('%s: world %d launches, %d dependent joins; motion %d launch, %d dependent joins' % ((case,) + d['world'] + d['motion']))
    print(json.dumps(rows))


if __name__ == '__main__':
    main()
