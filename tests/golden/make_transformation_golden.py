"""Generates tests/golden/transformation_ref.npz by EXECUTING THE REFERENCE's own Datasets/transformation.py (:72-124) on top of
islam_amd.compat's PyPose shim -- the drop-in claim of SURVEY.md section 8b for that file -- so that
tests/test_compat_cpu.py::test_reference_transformation_module_runs_on_the_shim can hold islam_amd.transformation to the reference's
results without a checkout of the reference:

  python tests/golden/make_transformation_golden.py <checkout of the reference>   ->  tests/golden/transformation_ref.npz

Stored: the inputs (m6: 7 se(3)-style motion rows, T0: one SE3), the reference's cvtSE3_pypose / tartan2kitti_pypose of m6,
motion2pose_pypose of the latter from T0, pose2motion_pypose of that, and the gradient of sum(motion2pose(tartan2kitti(m6), T0))
with respect to m6 (the path train.py takes from the motions into the poses)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(ref_root):
    from islam_amd import compat
    compat.install(force=True)
    from islam_amd import lietensor as pp
    spec = importlib.util.spec_from_file_location('_ref_transformation', os.path.join(ref_root, 'Datasets', 'transformation.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = torch.Generator().manual_seed(0)
    m6 = torch.randn(7, 6, generator=g, dtype=torch.float64) * 0.3
    T0 = pp.se3(torch.randn(6, generator=g, dtype=torch.float64) * 0.2).Exp()
    out = {'in_m6': m6.numpy(), 'in_T0': T0.tensor().numpy()}
    for fn in ('cvtSE3_pypose', 'tartan2kitti_pypose'):
        a = getattr(ref, fn)(m6)
        assert isinstance(a, pp.LieTensor), fn
        out[fn] = a.tensor().numpy()
    P = ref.motion2pose_pypose(ref.tartan2kitti_pypose(m6), T0)
    out['motion2pose_pypose'] = P.tensor().numpy()
    out['pose2motion_pypose'] = ref.pose2motion_pypose(P).tensor().numpy()
    m = m6.clone().requires_grad_(True)
    ref.motion2pose_pypose(ref.tartan2kitti_pypose(m), T0).tensor().sum().backward()
    out['grad_m6'] = m.grad.numpy()
    np.savez(os.path.join(HERE, 'transformation_ref.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main(sys.argv[1])
