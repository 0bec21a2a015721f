"""bench.py's command line without a GPU: the --full / --dump-outputs options exist, and dump_outputs writes float64 .npy files within
64 MB (a fixed, seeded sample of rows above that).  Run in a child process: importing bench sets GPU_MAX_HW_QUEUES for the process."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DUMP = '''
import sys, torch
sys.path.insert(0, %r)
import bench
g = torch.Generator().manual_seed(1)
for d, n in ((%r, 5001), (%r, 900000), (%r, 900000)):
    bench.dump_outputs(d, torch.randn(n, 7, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g, dtype=torch.float64),
                       torch.tensor(2.5, dtype=torch.float64), 10, 14)
'''


def test_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, check=True).stdout
    assert '--full' in out and '--dump-outputs' in out and '--steps' in out


def test_dump_outputs_float64_within_64mb(tmp_path):
    small, big, big2 = (str(tmp_path / d) for d in ('small', 'big', 'big2'))
    subprocess.run([sys.executable, '-c', DUMP % (ROOT, small, big, big2)], check=True)
    z = {f[:-4]: np.load(os.path.join(small, f)) for f in os.listdir(small)}
    assert set(z) == {'nodes', 'vels', 'loss', 'lm_counts'}
    assert all(a.dtype == np.float64 for a in z.values())
    assert z['nodes'].shape == (5001, 7) and z['vels'].shape == (5001, 3)
    assert z['loss'].tolist() == [2.5] and z['lm_counts'].tolist() == [10.0, 14.0]
    assert sum(os.path.getsize(os.path.join(big, f)) for f in os.listdir(big)) <= 64 << 20
    rows = np.load(os.path.join(big, 'rows.npy'))
    assert np.all(np.diff(rows) > 0) and rows[-1] < 900000 and np.load(os.path.join(big, 'nodes.npy')).shape == (len(rows), 7)
    np.testing.assert_array_equal(rows, np.load(os.path.join(big2, 'rows.npy')))       # the sample is the same every run
