"""Cost of islam_imu_preint_cov: us per call in world and motion mode at 5000 frames x 10 samples and at
4 frames x 200 samples (float64), beside islam_imu_preint_both on the same stream and the float64 numpy restatement of the
recurrence on one core.  HIP events around every call, 3 warm-up calls, the median of 20.  Every measurement runs in a child
process of its own under a time limit; a child that fails or runs out of time ends the script.

    python scripts/imu_cov_bench.py            # the table, and the launches / dependent joins of each mode
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'5000x10': (5001, 10), '4x200': (5, 200)}
WHAT = ('cov_world', 'cov_motion', 'preint_both', 'numpy_world', 'numpy_motion')
GYRO_COV, ACC_COV = (1.6968e-4) ** 2, (2.0e-3) ** 2


def depth(nframes, per):
    """(launches, dependent joins on the longest path) per mode, from the kernel's structure (csrc/imu_cov.hip)."""
    chunk = -(-per // 64)
    lanes = -(-per // chunk)
    frame = (chunk - 1) + (lanes - 1).bit_length()           # a lane's fold, then the tree over the lanes
    levels, n = [], nframes
    while True:
        levels.append(n)
        if n <= 64:
            break
        n = -(-n // 64)
    scan = sum((min(64, m) - 1).bit_length() for m in levels)
    carry = len(levels) - 1                                   # one join per level below the top
    launches = 1 + len(levels) + max(0, len(levels) - 2) + 1
    return {'motion': (1, frame), 'world': (launches, frame + scan + carry)}


def child(case, what):
    import numpy as np
    frames, per = CASES[case]
    from islam_amd import synthetic
    tr = synthetic.car_trajectory(frames, imu_per_frame=per, seed=1)
    seg_h = np.ascontiguousarray(tr['rgb2imu_sync'] - tr['rgb2imu_sync'][0], dtype=np.int64)
    if what.startswith('numpy'):
        os.environ.setdefault('OMP_NUM_THREADS', '1')
        from tests.test_imu_cov_gpu import cov_reference
        t0 = time.perf_counter()
        cov_reference(tr['imu_dts'], tr['gyros'], tr['accels'], seg_h, GYRO_COV, ACC_COV, what == 'numpy_motion')
        return {'us': (time.perf_counter() - t0) * 1e6, 'calls': 1}
    import torch
    from islam_amd import ops
    assert torch.cuda.is_available(), 'imu_cov_bench.py needs the GPU'
    dev = torch.device('cuda:0')
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    seg_d = torch.tensor(seg_h, device=dev)
    dt, gyro, acc = t64(tr['imu_dts']), t64(tr['gyros']), t64(tr['accels'])
    ip, ir, iv = t64(tr['init']['pos']), t64(tr['init']['rot']), t64(tr['init']['vel'])
    if what == 'preint_both':
        fn = lambda: ops.imu_preint_both(dt, gyro, acc, seg_d, seg_h, ip, ir, iv, tr['gravity'])
    else:
        fn = lambda: ops.imu_preint_cov(dt, gyro, acc, seg_d, seg_h, GYRO_COV, ACC_COV, what == 'cov_motion')
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    us.sort()
    return {'us': 0.5 * (us[9] + us[10]), 'min': us[0], 'max': us[-1], 'calls': 20}


def main():
    if len(sys.argv) == 4 and sys.argv[1] == '--child':
        print('RESULT ' + json.dumps(child(sys.argv[2], sys.argv[3])))
        return
    rows = {}
    for case in CASES:
        for what in WHAT:
            limit = 300 if what.startswith('numpy') else 180
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', case, what], capture_output=True, text=True, timeout=limit)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit('%s %s failed with exit code %d: nothing more is started' % (case, what, r.returncode))
            rows[case, what] = json.loads([ln for ln in r.stdout.split('\n') if ln.startswith('RESULT ')][-1][7:])
    print('| frames x samples | cov world (us) | cov motion (us) | imu_preint_both (us) | numpy world, 1 core (us) | numpy motion, 1 core (us) |')
    print('|---|---|---|---|---|---|')
    for case in CASES:
        print('| %s | ' % case + ' | '.join('%.1f' % rows[case, w]['us'] for w in WHAT) + ' |')
    for case, (frames, per) in CASES.items():
        d = depth(frames - 1, per)
        print('%s: world %d launches, %d dependent joins; motion %d launch, %d dependent joins' % ((case,) + d['world'] + d['motion']))
    print(json.dumps({'%s %s' % k: v for k, v in rows.items()}))


if __name__ == '__main__':
    main()
