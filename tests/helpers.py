"""Shared builders of seeded test problems (tests only; may import the oracle)."""
import numpy as np

from islam_amd import synthetic
from oracle import imu as oimu


def chain_problem(n_frames, seed=11, **kw):
    """Synthetic car trajectory -> run_pvgo inputs, IMU quantities from the oracle integrator."""
    tr = synthetic.car_trajectory(n_frames, seed=seed, **kw)
    F = n_frames
    pos, rot, vel = oimu.integrate(tr['accels'], tr['gyros'], tr['imu_dts'], tr['rgb2imu_sync'], 0, F - 1, tr['init'],
                                   tr['gravity'], False)
    dpos, drot, dvel = oimu.integrate(tr['accels'], tr['gyros'], tr['imu_dts'], tr['rgb2imu_sync'], 0, F - 1, tr['init'],
                                      tr['gravity'], True)
    return synthetic.pvgo_problem_from_deltas(tr, drot, dpos, dvel, pos, rot, vel), tr


def tumbling_trajectory(n_frames, seed=5, frame_dt=0.1, imu_per_frame=10, gravity=9.81, gyro_sigma=1.7e-4, acc_sigma=2e-3,
                        vo_sigma_t=0.05, vo_sigma_r=0.002):
    """An airborne body that tumbles: body rates up to ~2 rad/s about all three axes (0.2 rad per frame about a general, moving
    axis; the attitude covers SO(3), w < 0 included) on a closed 3-D curve.  Same keys and IMU / VO construction as
    synthetic.car_trajectory, whose yaw rate stays below 0.1 rad/s with 0.01 rad of roll and pitch."""
    from scipy.spatial.transform import Rotation
    F = int(n_frames)
    S = (F - 1) * imu_per_frame + 1
    h = frame_dt / imu_per_frame
    sub = 8
    hs = h / sub
    T = np.arange((S + 1) * sub + 1) * hs
    rng = np.random.default_rng(seed)
    ph = rng.uniform(0, 2 * np.pi, 6)
    Tm = 0.5 * (T[1:] + T[:-1])
    rate = np.stack([2.0 * np.sin(0.7 * Tm + ph[0]), 1.7 * np.sin(1.1 * Tm + ph[1]), 1.9 * np.cos(0.9 * Tm + ph[2])], 1)
    q = np.zeros((len(T), 4))
    q[0] = Rotation.random(random_state=seed).as_quat()
    inc = Rotation.from_rotvec(rate * hs).as_quat()
    x, y, z, w = inc.T
    for i in range(len(T) - 1):                                         # R_{i+1} = R_i Exp(rate hs)
        ax, ay, az, aw = q[i]
        q[i + 1] = (aw * x[i] + ax * w[i] + ay * z[i] - az * y[i], aw * y[i] - ax * z[i] + ay * w[i] + az * x[i],
                    aw * z[i] + ax * y[i] - ay * x[i] + az * w[i], aw * w[i] - ax * x[i] - ay * y[i] - az * z[i])
    R = Rotation.from_quat(q)
    pos_w = np.stack([8.0 * np.sin(0.5 * T + ph[3]), 8.0 * np.cos(0.3 * T + ph[4]), 3.0 * np.sin(0.7 * T + ph[5])], 1)
    vel_w = np.stack([4.0 * np.cos(0.5 * T + ph[3]), -2.4 * np.sin(0.3 * T + ph[4]), 2.1 * np.cos(0.7 * T + ph[5])], 1)
    idx = np.arange(S) * sub
    Rc = R[idx]
    gyro = (Rc.inv() * R[idx + sub]).as_rotvec() / h + rng.normal(0.0, gyro_sigma, (S, 3))
    acc = Rc.inv().apply((vel_w[idx + sub] - vel_w[idx]) / h + np.array([0.0, 0.0, gravity])) + rng.normal(0.0, acc_sigma, (S, 3))
    fidx = np.arange(F) * imu_per_frame
    gt_R = R[fidx * sub]
    gt_quat, gt_pos, gt_vel = gt_R.as_quat(), pos_w[fidx * sub], vel_w[fidx * sub]
    rel_R = gt_R[:-1].inv() * gt_R[1:]
    rel_t = gt_R[:-1].inv().apply(gt_pos[1:] - gt_pos[:-1])
    vo_q = (rel_R * Rotation.from_rotvec(rng.normal(0.0, vo_sigma_r, rel_t.shape))).as_quat()
    vo_t = rel_t + rel_R.apply(rng.normal(0.0, vo_sigma_t, rel_t.shape))
    links = np.stack([np.arange(F - 1), np.arange(1, F)], 1).astype(np.int64)
    return dict(gt_pos=gt_pos, gt_quat=gt_quat, gt_vel=gt_vel, accels=acc, gyros=gyro, imu_dts=np.full(S, h),
                rgb2imu_sync=fidx.astype(np.int64), vo_motions=np.concatenate([vo_t, vo_q], 1), links=links,
                dts=np.full(F - 1, frame_dt), gravity=gravity,
                init=dict(pos=gt_pos[0].copy(), rot=gt_quat[0].copy(), vel=gt_vel[0].copy()))


def tumbling_problem(n_frames, seed=5):
    """chain_problem on tumbling_trajectory: run_pvgo inputs with IMU deltas from the oracle integrator."""
    tr = tumbling_trajectory(n_frames, seed=seed)
    F = n_frames
    a = (tr['accels'], tr['gyros'], tr['imu_dts'], tr['rgb2imu_sync'], 0, F - 1, tr['init'], tr['gravity'])
    pos, rot, vel = oimu.integrate(*a, False)
    dpos, drot, dvel = oimu.integrate(*a, True)
    return synthetic.pvgo_problem_from_deltas(tr, drot, dpos, dvel, pos, rot, vel), tr


def se3_log_err(X, Xref):
    from oracle import lie
    d = lie.se3_log(lie.se3_mul(lie.se3_inv(Xref), X))
    return np.linalg.norm(d, axis=-1)


def reproj_inputs(tr, K, T_IL, H=112, W=160, K4=(80.0, 80.0, 80.0, 56.0), seed=0, noise_px=0.3):
    """Keypoints, depth and flow maps for a SparseReprojectionLoss over every link of trajectory `tr`: the flow at the
    keypoints is the true reprojection under the ground-truth motion (camera frame) plus pixel noise."""
    from oracle import lie, reproj as orp
    rng = np.random.default_rng(seed)
    gt = np.concatenate([tr['gt_pos'], tr['gt_quat']], 1)
    M = len(gt) - 1
    T_IL = np.asarray(T_IL, dtype=np.float64)
    mot = lie.se3_mul(lie.se3_inv(gt[:-1]), gt[1:])
    cam = lie.se3_mul(lie.se3_mul(lie.se3_inv(T_IL)[None], mot), T_IL[None])
    pts2d = np.stack([rng.integers(0, W, (M, K)), rng.integers(0, H, (M, K))], -1).astype(np.float64)
    depth = rng.uniform(5, 40, (M, H, W))
    flow = np.zeros((M, 2, H, W))
    b = np.arange(M)[:, None]
    col, row = pts2d[..., 0].astype(int), pts2d[..., 1].astype(int)
    fx, fy, cx, cy = K4
    P = orp.pixel2point(pts2d, depth[b, row, col], K4)
    p = lie.se3_act(lie.se3_inv(cam)[:, None, :], P)
    uv = np.stack([fx * p[..., 0] / p[..., 2] + cx, fy * p[..., 1] / p[..., 2] + cy], -1)
    flow[b, :, row, col] = uv - pts2d + rng.normal(0, noise_px, uv.shape)
    return dict(points2d=pts2d, depth=depth, flow=flow, fx=fx, fy=fy, cx=cx, cy=cy, rgb2imu_pose=T_IL)


def edge_test_image(seed, B=2, H=448, W=640, amp=0.5, cells=32, boxes=6):
    """Smooth low-contrast texture + a few rectangles of random contrast (strong and weak step edges): an edge mask that is
    neither empty nor full (the synthetic stereo texture is so busy that its mask is all ones)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(B, 3, H // cells + 2, W // cells + 2, generator=g)
    x = torch.nn.functional.interpolate(lo, size=(H, W), mode='bicubic', align_corners=False)
    x = 0.5 + amp * (x - 0.5)
    for b in range(B):
        for _ in range(boxes):
            y0 = int(torch.randint(0, max(H - 80, 1), (1,), generator=g))
            x0 = int(torch.randint(0, max(W - 80, 1), (1,), generator=g))
            h = int(torch.randint(20, 80, (1,), generator=g))
            w = int(torch.randint(20, 80, (1,), generator=g))
            x[b, :, y0:y0 + h, x0:x0 + w] += (torch.rand(1, generator=g).item() - 0.5) * 0.6
    return x.clamp(0, 1).contiguous()


# ------------------------------------------------------------------ differentiable torch restatement of the IMU frame loop
def _tq_mul(a, b):
    import torch
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def _tq_act(q, p):
    import torch
    u, w = q[..., :3], q[..., 3:]
    c = 2 * torch.linalg.cross(u, p)
    return p + w * c + torch.linalg.cross(u, c)


def _tq_exp(phi):
    import torch
    th = phi.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    return torch.cat([phi * torch.sin(0.5 * th) / th, torch.cos(0.5 * th)], -1)


def tq_log(q):
    """SO3 Log on raw quaternions (plain autograd), SURVEY Appendix C item 2."""
    import torch
    v, w = q[..., :3], q[..., 3:]
    n = v.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    return v * 2 * torch.atan(n / w) / n


def imu_preint_torch(dt, gyro, acc, seg, init_pos, init_rot, init_vel, gravity, motion_mode):
    """oracle/imu_preint_body.inc in plain torch ops (float64, sequential products instead of the doubling scan), so that
    torch.autograd gives reference gradients w.r.t. gyro / acc for the HIP backward (islam_imu_preint_bwd)."""
    import torch
    g = torch.tensor([0, 0, gravity], dtype=dt.dtype)
    lp, lr, lv = (torch.zeros(3, dtype=dt.dtype), init_rot, torch.zeros(3, dtype=dt.dtype)) if motion_mode else (init_pos, init_rot, init_vel)
    sp, sr, sv = lp, lr, lv
    P, R, V = ([], [], []) if motion_mode else ([lp], [lr], [lv])
    for i in range(len(seg) - 1):
        a, F = int(seg[i]), int(seg[i + 1] - seg[i])
        if F == 0:
            if motion_mode:
                sp = torch.zeros(3, dtype=dt.dtype)
            sv = torch.zeros(3, dtype=dt.dtype)
        else:
            A = torch.tensor([0, 0, 0, 1.0], dtype=dt.dtype)
            iv, ip, it = torch.zeros(3, dtype=dt.dtype), torch.zeros(3, dtype=dt.dtype), 0.0
            for j in range(a, a + F):
                A1 = _tq_mul(A, _tq_exp(gyro[j] * dt[j]))
                q = _tq_mul(lr, A1)
                gb = _tq_act(q * torch.tensor([-1, -1, -1, 1.0], dtype=dt.dtype), g)
                ra = _tq_act(A, acc[j] - gb)
                ip = ip + iv * dt[j] + ra * 0.5 * dt[j] * dt[j]
                iv = iv + ra * dt[j]
                it = it + dt[j]
                A = A1
            sr = _tq_mul(lr, A)
            sv = lv + _tq_act(lr, iv)
            sp = lp + _tq_act(lr, ip) + lv * it
        P.append(sp)
        V.append(sv)
        R.append(_tq_mul(lr * torch.tensor([-1, -1, -1, 1.0], dtype=dt.dtype), sr) if motion_mode else sr)
        lr = sr
        if not motion_mode:
            lp, lv = sp, sv
    return torch.stack(P), torch.stack(R), torch.stack(V)


def spawn_ranks(worker, nprocs, *args, retries=1):
    """torch.multiprocessing.spawn(worker, args=(nprocs, port, *args)) on a free 127.0.0.1 port.  The workers open their gloo group with a
    3-minute timeout (GLOO_TIMEOUT_S below), so a peer that never arrives fails the attempt in minutes instead of gloo's default 30 --
    seen once in round 6: the whole `-m gpu` run sat 35 minutes in one spawn test that passes in 4 s alone and in the next full run --
    and the attempt is repeated once on a fresh port."""
    import socket
    import torch.multiprocessing as mp
    last = None
    for attempt in range(retries + 1):
        s = socket.socket()
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
        s.close()
        try:
            mp.spawn(worker, args=(nprocs, port) + tuple(args), nprocs=nprocs, join=True)
            return
        except Exception as e:          # pragma: no cover (transient)
            last = e
    raise last


GLOO_TIMEOUT_S = 180
