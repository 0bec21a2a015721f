"""Recipe for a PyPose pin of the pre-integration covariance -- NOT run yet: PyPose is not installed where this
repository is built, so no fixture is committed and the match of islam_imu_preint_cov to pp.module.IMUPreintegrator(prop_cov=True)
stays unpinned.  On a machine that has PyPose:

    python tests/golden/make_imu_cov_golden.py        # writes tests/golden/imu_cov_pypose.npz

The file holds seeded inputs (one frame each, identity initial rotation) and the 9x9 covariance PyPose returns for them, with the
PyPose version.  A test that reads it must say which of the two differences it allows for: PyPose's state ordering / perturbation
side (compare after the permutation and the DR^T rotation DESIGN.md gives, if they differ) and its discretisation of B."""
import os

import numpy as np


def main():
    import pypose as pp
    import torch
    torch.set_default_dtype(torch.float64)
    rng = np.random.default_rng(0)
    out = {'pypose_version': np.array(pp.__version__)}
    for name, n in (('n10', 10), ('n70', 70), ('n200', 200)):
        dt = rng.uniform(0.004, 0.012, (n, 1))
        gyro = rng.normal(0, 0.5, (n, 3))
        acc = rng.normal(0, 1.0, (n, 3)) + np.array([0, 0, 9.81])
        integ = pp.module.IMUPreintegrator(torch.zeros(3), pp.identity_SO3(), torch.zeros(3), gravity=0.0, prop_cov=True, reset=True)
        state = integ(dt=torch.tensor(dt)[None], gyro=torch.tensor(gyro)[None], acc=torch.tensor(acc)[None])
        out[name + '_dt'], out[name + '_gyro'], out[name + '_acc'] = dt[:, 0], gyro, acc
        out[name + '_cov'] = state['cov'][0, -1].numpy() if state['cov'].dim() == 4 else state['cov'][0].numpy()
        out[name + '_gyro_cov'], out[name + '_acc_cov'] = (torch.as_tensor(integ.gyro_cov).reshape(-1).numpy(),
                                                             torch.as_tensor(integ.acc_cov).reshape(-1).numpy())
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'imu_cov_pypose.npz'), **out)


if __name__ == '__main__':
    main()
