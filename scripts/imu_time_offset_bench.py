"""Cost of islam_imu_time_offset_solve: us per call (float64, the residuals asked for, its 8-byte read-back and
synchronise included) at 5000 rows of 10 samples and at 300 007 rows, for td alone, for bias + td, and for bias + td with four Huber
rounds, beside islam_imu_gyro_bias_solve (section 3.12, one workgroup) on the same rows in the same process as the yardstick.  The rows
come from the shipped integrator and its bias Jacobians on a stream of uniform dt whose three gyro axes are sines of different
frequency; the references are planted linear-exact, every tenth one turned by 0.05 rad.  HIP events around every call, 3 warm-up calls,
the median of 20, three runs.  There is no earlier version to compare against and no target.  Every case runs in a child process of its
own under a time limit; a child that fails or runs out of time ends the script.

    python scripts/imu_time_offset_bench.py [--out profiles/imu_time_offset_bench.json]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'5000x10': 5000, 'N300007': 300007}
WHAT = ('td', 'bias_td', 'bias_td_K4', 'gyro_bias_solve')
PER = 10
ROW_BYTES = 8 * (9 + 4 + 4 + 3 + 3 + 15)                    # float64: J_phig, two quaternions, two rates read, fifteen terms written


def child(case):
    import numpy as np
    import torch
    from islam_amd import ops
    from tests.test_imu_extrinsic_gpu import qexp, qmul
    from tests.test_imu_time_offset_gpu import B_PLANTED, DT, TD_PLANTED, true_rates
    assert torch.cuda.is_available(), 'imu_time_offset_bench.py needs the GPU'
    rows = CASES[case]
    dev = torch.device('cuda:0')
    S = rows * PER + 1
    seg_host = np.arange(rows + 1, dtype=np.int64) * PER
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    dts, gyros, accels = t64(np.full(S, DT)), t64(true_rates(S)), t64(np.tile(np.array([0.0, 0.0, 9.8]), (S, 1)))
    seg = torch.from_numpy(seg_host).to(dev)
    init = t64(np.array([0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0]))
    _, rot, _ = ops.imu_preint(dts, gyros, accels, seg, seg_host, init[0:3], init[3:7], init[7:10], 0.0, True)
    jac = ops.imu_preint_bias_jac(dts, gyros, accels, seg, seg_host, True)
    ws, we = gyros[seg[:-1]].contiguous(), gyros[seg[1:]].contiguous()
    # the planted references, on the host: DR Exp(J b + u td), every tenth one turned by 0.05 rad
    q, J = rot.cpu().numpy(), jac[:, 0:3, 0:3].cpu().numpy()
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(rows, 3, 3)
    u = we.cpu().numpy() - np.einsum('nkc,nk->nc', R, ws.cpu().numpy())
    ref = qmul(q, qexp(J @ B_PLANTED + u * TD_PLANTED))
    ref[::10] = qmul(ref[::10], qexp(np.tile(np.array([0.0, 0.05, 0.0]), (len(ref[::10]), 1))))
    ref = t64(ref)
    fns = {'td': lambda: ops.imu_time_offset_solve(None, rot, ref, ws, we, None, False),
           'bias_td': lambda: ops.imu_time_offset_solve(jac, rot, ref, ws, we),
           'bias_td_K4': lambda: ops.imu_time_offset_solve(jac, rot, ref, ws, we, None, True, 1e-3, 4),
           'gyro_bias_solve': lambda: ops.imu_gyro_bias_solve(jac, rot, ref)}

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
    out = {k: [median20(fns[k]) for _ in range(3)] for k in WHAT}
    got = fns['bias_td_K4']()
    out['err_b_K4'] = float(np.abs(got[0].cpu().numpy() - B_PLANTED).max())
    out['err_td_K4'] = abs(float(got[1]) - TD_PLANTED)
    out['row_MB_per_round'] = ROW_BYTES * rows / 1e6
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        print('RESULT ' + json.dumps(child(sys.argv[2])))
        return
    rows = {}
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', case], capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit('%s failed with exit code %d: nothing more is started' % (case, r.returncode))
        rows[case] = json.loads([ln for ln in r.stdout.split('\n') if ln.startswith('RESULT ')][-1][7:])
    print('us per call: the median of 20, three runs; err: against the planted (b, td) after four Huber rounds')
    print('| rows | ' + ' | '.join(WHAT) + ' | row_MB_per_round | err_b_K4 | err_td_K4 |')
    print('|---|' + '---|' * (len(WHAT) + 3))
    for case in CASES:
        c = rows[case]
        print('| %s | ' % case + ' | '.join(' / '.join('%.3g' % v for v in c[k]) for k in WHAT)
              + ' | %.3g | %.3g | %.3g |' % (c['row_MB_per_round'], c['err_b_K4'], c['err_td_K4']))
    line = json.dumps(rows)
    print(line)
    if len(sys.argv) == 3 and sys.argv[1] == '--out':
        with open(sys.argv[2], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
