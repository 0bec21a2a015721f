"""IMUModule with the reference's call surface (reference imu_integrator.py:11-164) on the HIP integrator.

One ``integrate`` call = slice the stream (:94-99), static-bias / denoiser correction (:101-113, PyTorch-ROCm),
then ONE call into libislam_hip.so for the whole frame loop (:116-158): the reference runs ~60 tiny kernels
and 3 device->host copies per frame.  Outputs come back on the CPU like the reference's (poses, rots, covs, vels).
``covs`` is ``[]`` like the reference's unless the module was built with ``prop_cov=True``: then it is the (rows, 9, 9)
covariance of the pre-integration (islam_imu_preint_cov), which the reference's PyPose integrator propagates and drops.
``bias_jac=True`` keeps the (rows, 9, 6) bias Jacobians of the rows (islam_imu_preint_bias_jac) on the module as
``last_bias_jac``; ``estimate_gyro_bias`` recovers a gyro bias from trusted relative rotations in closed form.
"""
import numpy as np
import torch

from . import lietensor as pp
from . import ops
from .nets import IMUCorrector_CNN_GRU_WO_COV


def prase_init(init=None, motion_mode=False, device='cuda:0', dtype=None):
    """imu_integrator.py:11-28 (name kept, typo included)."""
    dtype = dtype or torch.get_default_dtype()
    z3 = torch.zeros(3, dtype=dtype, device=device)
    if init is not None:
        rot = torch.as_tensor(np.asarray(init['rot']), dtype=dtype).to(device)
        if motion_mode:
            return z3, pp.SO3(rot), z3.clone()
        return (torch.as_tensor(np.asarray(init['pos']), dtype=dtype).to(device), pp.SO3(rot),
                torch.as_tensor(np.asarray(init['vel']), dtype=dtype).to(device))
    return z3, pp.identity_SO3(dtype=dtype, device=device), z3.clone()


class IMUModule:
    def __init__(self, accels, gyros, dts, accel_bias=torch.zeros(3), gyro_bias=torch.zeros(3), init=None, gravity=9.81007,
                 rgb2imu_sync=None, device='cuda:0', denoise_model_name=None, denoise_accel=True, denoise_gyro=True,
                 use_est_cov=False, dtype=None, prop_cov=False, gyro_cov=(1.6968e-4) ** 2, acc_cov=(2.0e-3) ** 2,
                 bias_jac=False):
        if torch.device(device).type != 'cuda':
            raise RuntimeError('islam_amd.IMUModule runs on the MI355X only (device=%r); there is no CPU fallback' % (device,))
        self.device = device
        self.last_frame_dt = 0.1
        self.dtype = dtype or torch.get_default_dtype()       # the reference integrates in the default dtype (:44)
        self.gravity = float(gravity)
        self.rgb2imu_sync = np.arange(len(accels), dtype=np.int64) if rgb2imu_sync is None else \
            np.asarray(rgb2imu_sync, dtype=np.int64)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=self.dtype).to(device)
        self.accels, self.gyros = t(accels), t(gyros)
        self.dts = t(dts).unsqueeze(-1)
        self.denoise_accel, self.denoise_gyro = denoise_accel, denoise_gyro
        self.use_denoise_model = denoise_model_name is not None and denoise_model_name != '' and (denoise_accel or denoise_gyro)
        self.optm_bias = not self.use_denoise_model and (denoise_accel or denoise_gyro)
        self.accel_bias, self.gyro_bias = t(accel_bias), t(gyro_bias)
        if self.use_denoise_model:
            self.denoiser = IMUCorrector_CNN_GRU_WO_COV()
            self.denoiser.load_state_dict(torch.load(denoise_model_name))
            self.denoiser = self.denoiser.to(device)
            self.use_est_cov = use_est_cov
        # The reference calls the denoiser with eval=True (imu_integrator.py:109): no gradient ever reaches it, so its
        # "IMU epochs" (train.py:177-179) step the optimizer on empty gradients.  train_denoiser = True is the
        # fix SURVEY section 8f rank 4 asks for: the denoiser runs with grad enabled and the pre-integration is differentiable
        # (islam_imu_preint_bwd), so run_pvgo(target='imu') back-propagates into its parameters.  Default: reference behaviour.
        self.train_denoiser = False
        # prop_cov: integrate() also returns the 9x9 covariances of the pre-integration, error state [dphi, dv, dp], from the per-sample
        # measurement variances gyro_cov / acc_cov (a scalar or three values; believed to be PyPose's defaults -- unpinned).  The
        # denoiser predicts no covariance (IMUCorrector_CNN_GRU_WO_COV returns None for both), so use_est_cov stays inert.
        self.prop_cov = bool(prop_cov)
        self.gyro_cov, self.acc_cov = gyro_cov, acc_cov
        # bias_jac: integrate() / integrate_both() also leave the (rows, 9, 6) Jacobians of the rows w.r.t. a further gyro / accelerometer
        # bias on the module (CPU, module dtype; integrate_both: the (world, motion) pair).  The returned tuples do not change.
        self.bias_jac = bool(bias_jac)
        self.last_bias_jac = None

    def _jac(self, dts, gyros, accels, seg, seg_host, motion_mode):
        """(rows, 9, 6) bias Jacobians in the module dtype, on the device; forward values only."""
        return ops.imu_preint_bias_jac(dts.contiguous(), gyros.detach().contiguous(), accels.detach().contiguous(), seg, seg_host,
                                       motion_mode).to(self.dtype)

    def _cov(self, dts, gyros, accels, seg, seg_host, motion_mode, init_cov):
        """(rows, 9, 9) covariance rows in the module dtype, on the device; forward values only."""
        if init_cov is not None:
            init_cov = torch.as_tensor(np.asarray(init_cov, dtype=np.float64)).to(self.device)
        with torch.no_grad():
            cov = ops.imu_preint_cov(dts.contiguous(), gyros.detach().contiguous(), accels.detach().contiguous(), seg, seg_host,
                                     self.gyro_cov, self.acc_cov, motion_mode, None if motion_mode else init_cov)
        return cov.to(self.dtype)

    def _corrected(self, st, end):
        """The stream slice of frames [st, end] after the static-bias / denoiser correction (imu_integrator.py:94-113)."""
        b0 = int(self.rgb2imu_sync[st])
        b1 = int(self.rgb2imu_sync[end]) + 1
        dts = self.dts[b0:b1, 0]                    # contiguous views of the stream; only written to through new tensors
        gyros = self.gyros[b0:b1]
        accels = self.accels[b0:b1]
        if self.optm_bias:
            if self.denoise_accel:
                accels = accels - self.accel_bias.view(1, 3)
            if self.denoise_gyro:
                gyros = gyros - self.gyro_bias.view(1, 3)
        if self.use_denoise_model and b1 - b0 >= 10:
            ddt = next(self.denoiser.parameters()).dtype          # the reference's denoiser lives in the default dtype too
            d_acc, d_gyro, _, _ = self.denoiser({'acc': accels.to(ddt), 'gyro': gyros.to(ddt)}, eval=not self.train_denoiser)
            if self.denoise_accel:
                accels = d_acc.to(self.dtype)
            if self.denoise_gyro:
                gyros = d_gyro.to(self.dtype)
        return b0, dts, gyros, accels

    def _start(self, st, end, b0, init, motion_mode):
        """What integrate / integrate_both send ahead of the samples: prase_init (imu_integrator.py:11-28) packed into one transfer,
        [pos(3) | rot(4) | vel(3)] (the motion rows ignore pos / vel: the kernel starts them from zero), and the frame offsets inside the
        slice that starts at sample b0, on the host and on the device."""
        np_dt = {torch.float32: np.float32, torch.float64: np.float64}[self.dtype]
        i10 = np.zeros(10, dtype=np_dt)
        i10[6] = 1.0
        if init is not None:
            i10[3:7] = np.asarray(init['rot'], dtype=np_dt)
            if not motion_mode:
                i10[0:3] = np.asarray(init['pos'], dtype=np_dt)
                i10[7:10] = np.asarray(init['vel'], dtype=np_dt)
        i10 = torch.from_numpy(i10).to(self.device)
        seg_host = np.ascontiguousarray(self.rgb2imu_sync[st:end + 1] - b0, dtype=np.int64)
        return i10, seg_host, torch.from_numpy(seg_host).to(self.device)

    def _as_device(self, a, dtype):
        """An SO3, a tensor or an array as a detached tensor of ``dtype`` on the device."""
        a = a.tensor() if hasattr(a, 'tensor') else torch.as_tensor(np.asarray(a))
        return a.detach().to(dtype).to(self.device)

    def _weight(self, weight):
        """The optional weights of a solve as a float64 tensor on the device."""
        return None if weight is None else torch.as_tensor(np.asarray(weight), dtype=torch.float64).to(self.device)

    def _window(self, st, end, gyro_bias=None, accel_bias=None, k=None):
        """Frames [st, end] of the stored stream as the samples of a closed-form solve: (seg_host, seg, dts, gyros, accels), the frame
        offsets inside the slice on the host and on the device and the contiguous slice with the given biases (device tensors, None =
        none) subtracted, whatever ``optm_bias`` says; the denoiser is not run.  k: the frame boundaries moved by k whole samples and
        clipped to the stored stream."""
        sync = np.asarray(self.rgb2imu_sync[st:end + 1], dtype=np.int64)
        if k is not None:
            sync = np.clip(sync + k, 0, int(self.dts.shape[0]) - 1)
        b0, b1 = int(sync[0]), int(sync[-1]) + 1
        seg_host = np.ascontiguousarray(sync - b0, dtype=np.int64)
        seg = torch.from_numpy(seg_host).to(self.device)
        gyros, accels = self.gyros[b0:b1], self.accels[b0:b1]
        if gyro_bias is not None:
            gyros = gyros - gyro_bias.view(1, 3)
        if accel_bias is not None:
            accels = accels - accel_bias.view(1, 3)
        return seg_host, seg, self.dts[b0:b1, 0].contiguous(), gyros.contiguous(), accels.contiguous()

    def _motion_rows(self, dts, gyros, accels, seg, seg_host, jac):
        """The motion rows of a window from the identity at gravity 0: their rotations and, with ``jac``, their bias Jacobians (else None)."""
        init = torch.zeros(10, dtype=self.dtype, device=self.device)
        init[6] = 1.0
        _, rot, _ = ops.imu_preint(dts, gyros, accels, seg, seg_host, init[0:3], init[3:7], init[7:10], 0.0, True)
        return rot, (ops.imu_preint_bias_jac(dts, gyros, accels, seg, seg_host, True) if jac else None)

    def integrate_both(self, st, end, init=None, init_cov=None):
        """``integrate(st, end, init, motion_mode=False)`` and ``integrate(st, end, init, motion_mode=True)`` -- the pair the
        reference's loop asks for on every batch (train.py:200-215) -- from ONE pass over the samples (islam_imu_preint_both: the
        scan, the rotation chain and the frame sums are common to the two modes) and one device->host copy.  Returns the two
        result tuples, bit-identical to the two calls.  Forward values only: with ``train_denoiser`` the two differentiable calls
        are made instead.  With ``prop_cov`` both tuples carry their covariances (``init_cov``: row 0 of the world rows)."""
        if self.train_denoiser and self.use_denoise_model:
            return self.integrate(st, end, init, motion_mode=False, init_cov=init_cov), self.integrate(st, end, init, motion_mode=True)
        b0, dts, gyros, accels = self._corrected(st, end)
        i10, seg_host, seg = self._start(st, end, b0, init, False)
        with torch.no_grad():
            world, motion, packed = ops.imu_preint_both(dts.contiguous(), gyros.detach().contiguous(), accels.detach().contiguous(), seg,
                                                        seg_host, i10[0:3], i10[3:7], i10[7:10], self.gravity)
        n = len(seg_host) - 1
        if self.prop_cov:                           # the covariances ride in the same device->host copy
            covs = [self._cov(dts, gyros, accels, seg, seg_host, mm, init_cov) for mm in (False, True)]
            packed = torch.cat([packed] + [c.reshape(-1) for c in covs])
        if self.bias_jac:
            jacs = [self._jac(dts, gyros, accels, seg, seg_host, mm) for mm in (False, True)]
            packed = torch.cat([packed] + [j.reshape(-1) for j in jacs])
        host = packed.cpu()
        res, o = [], 0
        for rows in (n + 1, n):
            pos = host[o:o + rows * 3].view(rows, 3); o += rows * 3
            rot = host[o:o + rows * 4].view(rows, 4); o += rows * 4
            vel = host[o:o + rows * 3].view(rows, 3); o += rows * 3
            res.append([pos.contiguous(), pp.SO3(rot.contiguous()), [], vel.contiguous()])
        if self.prop_cov:
            for r, rows in zip(res, (n + 1, n)):
                r[2] = host[o:o + rows * 81].view(rows, 9, 9).contiguous(); o += rows * 81
        if self.bias_jac:
            pair = []
            for rows in (n + 1, n):
                pair.append(host[o:o + rows * 54].view(rows, 9, 6).contiguous()); o += rows * 54
            self.last_bias_jac = tuple(pair)
        return tuple(res[0]), tuple(res[1])

    def integrate(self, st, end, init=None, motion_mode=False, init_cov=None):
        """imu_integrator.py:69-164.  world mode: (end-st+1) rows incl. the initial state; motion mode: (end-st) rows.
        Host traffic per call: one H2D of the 10 initial-state values, one of the frame offsets, one D2H of the packed
        result (the reference: 3 D2H copies per frame).  ``prop_cov``: ``covs`` is the (rows, 9, 9) covariance of the rows
        (world mode: row 0 = ``init_cov``, None = zero; accumulated over the whole range in the body frame of its start;
        motion mode: every frame from zero), in the same copy."""
        b0, dts, gyros, accels = self._corrected(st, end)
        i10, seg_host, seg = self._start(st, end, b0, init, motion_mode)
        pos, rot, vel = ops.imu_preint(dts.contiguous(), gyros.contiguous(), accels.contiguous(), seg, seg_host,
                                       i10[0:3], i10[3:7], i10[7:10], self.gravity, motion_mode)
        cols = [pos, rot, vel]
        if self.prop_cov:
            cov = self._cov(dts, gyros, accels, seg, seg_host, motion_mode, init_cov)
            cols.append(cov.reshape(cov.shape[0], 81))
        if self.bias_jac:                           # rides in the same device->host copy, behind the covariance columns
            jac = self._jac(dts, gyros, accels, seg, seg_host, motion_mode)
            cols.append(jac.reshape(jac.shape[0], 54))
        out = torch.cat(cols, 1).cpu()
        if self.bias_jac:
            self.last_bias_jac = out[:, -54:].detach().reshape(-1, 9, 6).contiguous()
        covs = out[:, 10:91].detach().reshape(-1, 9, 9).contiguous() if self.prop_cov else []
        return out[:, 0:3].contiguous(), pp.SO3(out[:, 3:7].contiguous()), covs, out[:, 7:10].contiguous()

    def estimate_gyro_bias(self, st, end, ref_rots, weight=None):
        """Gyro bias of frames [st, end] from relative rotations the caller trusts (``ref_rots``: (end - st, 4) xyzw quaternions or an
        SO3, frame i -> i + 1: VO or PVGO-optimised), in closed form: the motion rows are integrated with the module's current
        ``gyro_bias`` subtracted (whatever ``optm_bias`` says; the denoiser is not run), their rotations and bias Jacobians give
        dbg = argmin sum_i w_i |Log(DR_i^T ref_i) - J_phig,i dbg|^2 (islam_imu_gyro_bias_solve).  Returns (``gyro_bias + dbg`` (3) and
        the 3x3 normal matrix H, both on the CPU in float64).  The module is not changed."""
        with torch.no_grad():
            seg_host, seg, dts, gyros, accels = self._window(st, end, self.gyro_bias)
            ref, weight = self._as_device(ref_rots, self.dtype), self._weight(weight)
            rot, jac = self._motion_rows(dts, gyros, accels, seg, seg_host, True)
            dbg, H, _ = ops.imu_gyro_bias_solve(jac, rot, ref, weight)
            res = torch.cat((self.gyro_bias.to(torch.float64) + dbg, H.reshape(9))).cpu()
        return res[0:3].contiguous(), res[3:12].view(3, 3).contiguous()

    def estimate_time_offset(self, st, end, ref_rots, weight=None, solve_bias=True, delta=None, rounds=4, gn_rounds=3):
        """Time offset between the camera's and the IMU's clock, with the gyro bias, of frames [st, end] from relative rotations the
        caller trusts (``ref_rots``: (end - st, 4) xyzw quaternions or an SO3 of the BODY, frame i -> i + 1: VO or PVGO-optimised,
        conjugated by the mount's rotation), by Gauss-Newton rounds of a closed-form solve (islam_imu_time_offset_solve).  Sign: an image
        stamped t was taken at t + T on the IMU's clock, so ADD T to the camera's stamps, i.e. move ``rgb2imu_sync`` by k samples (the
        rest, 0 <= T - k dt < dt, is below the sample spacing).  The state is T = k dt + tau (k whole samples, 0 <= tau < dt), starting
        at 0, and the module's ``gyro_bias``.  Each of the 1 + ``gn_rounds`` rounds slices the frames with their boundaries moved by k
        samples, subtracts the current bias (whatever ``optm_bias`` says; the denoiser is not run), integrates the motion rows with
        gravity 0 and their bias Jacobians, takes the boundary rates from the slice (the sample that starts at each boundary), moves the
        rotations by tau (islam_imu_time_shift), solves for (dbg, td) and updates bias += dbg, T += td.  The Jacobian of the un-shifted
        increment is used for the shifted one (the difference is first order in tau and only slows convergence).  Rows whose moved
        window or end sample leaves the stored stream get weight zero.  ``weight``: (end - st) per frame; ``solve_bias=False`` keeps the
        bias; ``delta`` / ``rounds``: the Huber rounds of every solve.  With ``gn_rounds > 0`` the sample spacing of the slice must be
        uniform to 1e-6 relative (``ValueError`` otherwise); ``gn_rounds = 0`` is the single linearised solve and accepts any spacing (k
        then counts samples of the slice's first spacing).  The first linearisation has to point the right way: roughly |T| below a
        quarter period of the motion.  Returns (T in seconds (a 0-d tensor), ``gyro_bias`` + the sum of dbg (3), the 4x4 normal matrix H
        of the last round in the order dbg, td, the residuals (end - st) of the last round, k), on the CPU in float64 (k: an int).  A
        constant angular rate leaves T undetermined: IslamHipError (ISLAM_ENOTPD).  The module is not changed."""
        sync = np.asarray(self.rgb2imu_sync[st:end + 1], dtype=np.int64)
        n, S = len(sync) - 1, int(self.dts.shape[0])
        ref = self._as_device(ref_rots, self.dtype)
        w0 = np.ones(n) if weight is None else np.asarray(weight, dtype=np.float64).reshape(n).copy()
        slice_dts = self.dts[int(sync[0]):int(sync[-1]) + 1, 0].to(torch.float64).cpu().numpy()
        dt = float(slice_dts[0])
        if gn_rounds > 0 and not np.all(np.abs(slice_dts - dt) <= 1e-6 * abs(dt)):
            raise ValueError('estimate_time_offset: the sample spacing of frames [%d, %d] is not uniform to 1e-6 (%.9g .. %.9g); only '
                             'gn_rounds=0, the single linearised solve, accepts that' % (st, end, slice_dts.min(), slice_dts.max()))
        T, k, tau = 0.0, 0, 0.0
        bias = self.gyro_bias.detach().to(torch.float64).cpu().numpy().copy()
        with torch.no_grad():
            for _ in range(1 + int(gn_rounds)):
                moved = sync + k
                inside = (moved[:-1] >= 0) & (moved[1:] <= S - 1)          # the window and the sample that starts at its end are stored
                w = torch.from_numpy(np.where(inside, w0, 0.0)).to(self.device)
                seg_host, seg, dts, gyros, accels = self._window(st, end, torch.from_numpy(bias).to(self.dtype).to(self.device), k=k)
                rot, jac = self._motion_rows(dts, gyros, accels, seg, seg_host, True)
                rate_start, rate_end = gyros[seg[:-1]].contiguous(), gyros[seg[1:]].contiguous()
                rot = ops.imu_time_shift(rot, rate_start, rate_end, tau)
                dbg, td, H, res, _ = ops.imu_time_offset_solve(jac, rot, ref, rate_start, rate_end, w, solve_bias, delta, rounds)
                host = torch.cat((dbg, td.reshape(1), H.reshape(16), res)).cpu()
                bias = bias + host[0:3].numpy()
                T = T + float(host[3])
                k = int(np.floor(T / dt))
                tau = T - k * dt
        return (torch.tensor(T, dtype=torch.float64), torch.from_numpy(bias), host[4:20].view(4, 4).contiguous(), host[20:20 + n].contiguous(), k)

    def _alignment_rows(self, st, end, use_cov):
        """The rows of the closed-form alignment solves over frames [st, end], on the device: (n, durations (n), dvel, dpos (n, 3) in the
        start-body frame of their frame, bias Jacobians (n, 9, 6), motion-mode covariances (n, 9, 9) or None).  The motion rows are
        integrated with gravity 0 and the module's current ``gyro_bias`` and ``accel_bias`` subtracted."""
        seg_host, seg, dts, gyros, accels = self._window(st, end, self.gyro_bias, self.accel_bias)
        n = len(seg_host) - 1
        init = torch.zeros(10, dtype=self.dtype, device=self.device)
        init[6] = 1.0
        world, motion, _ = ops.imu_preint_both(dts, gyros, accels, seg, seg_host, init[0:3], init[3:7], init[7:10], 0.0)
        # motion rows hold R0_i dv_i, R0_i dp_i with R0_i = row i of the world rotations from the identity (include/islam_hip.h)
        R0t = pp._qmat(world[1][:n].to(torch.float64)).transpose(-1, -2)
        dvel = (R0t @ motion[2].to(torch.float64).unsqueeze(-1)).squeeze(-1).to(self.dtype)
        dpos = (R0t @ motion[0].to(torch.float64).unsqueeze(-1)).squeeze(-1).to(self.dtype)
        # d_i = the sum of the frame's dt, in a fixed order: the frames padded to the longest one
        maxF = int(np.max(np.diff(seg_host))) if n > 0 else 0
        idx = seg[:-1, None] + torch.arange(max(maxF, 1), device=self.device)[None, :]
        inside = idx < seg[1:, None]
        dur = torch.where(inside, dts.to(torch.float64)[idx.clamp(max=max(int(dts.shape[0]) - 1, 0))], torch.zeros((), dtype=torch.float64,
                          device=self.device)).sum(1).to(self.dtype)
        jac = ops.imu_preint_bias_jac(dts, gyros, accels, seg, seg_host, True)
        cov = ops.imu_preint_cov(dts, gyros, accels, seg, seg_host, self.gyro_cov, self.acc_cov, True) if use_cov else None
        return n, dur, dvel, dpos, jac, cov

    def estimate_gravity_accel_bias(self, st, end, ref_rots, ref_pos, weight=None, use_cov=False, gravity_norm=None):
        """Gravity, accelerometer bias and velocities of frames [st, end] from world poses of the IMU body the caller trusts
        (``ref_rots``: (end - st + 1, 4) xyzw quaternions or an SO3, ``ref_pos``: (end - st + 1, 3); VO or PVGO-optimised, rgb2imu
        applied), in closed form (islam_imu_gravity_bias_solve).  The motion rows are integrated with gravity 0 and the module's
        current ``gyro_bias`` and ``accel_bias`` subtracted (whatever ``optm_bias`` says; the denoiser is not run) and brought into the
        start-body frame of their frame; their bias Jacobians and, with ``use_cov``, their motion-mode covariances (the module's
        ``gyro_cov`` / ``acc_cov``) enter the solve; the duration of a frame is the sum of its ``dt``.  ``weight``: (end - st - 1) per
        pair of consecutive frames; ``gravity_norm``: the known magnitude of gravity, None = free.  Returns (gravity (3) in the frame
        of the poses, ``accel_bias + b`` (3), velocities (end - st + 1, 3), the 6x6 normal matrix H), on the CPU in float64.  The
        gravity is the world acceleration (v' = R a + g), about (0, 0, -9.81) in a z-up world.  Run ``estimate_gyro_bias`` first: the
        gyro-bias sensitivity of the increments is not part of this solve.  The module is not changed."""
        rots, poss, weight = self._as_device(ref_rots, self.dtype), self._as_device(ref_pos, self.dtype), self._weight(weight)
        with torch.no_grad():
            n, dur, dvel, dpos, jac, cov = self._alignment_rows(st, end, use_cov)
            g, b, H, vel, _ = ops.imu_gravity_bias_solve(rots, poss, dur, dvel, dpos, jac, cov, weight, gravity_norm)
            res = torch.cat((g, self.accel_bias.to(torch.float64) + b, vel.reshape(-1), H.reshape(36))).cpu()
        o = 6 + 3 * (n + 1)
        return res[0:3].contiguous(), res[3:6].contiguous(), res[6:o].view(n + 1, 3).contiguous(), res[o:o + 36].view(6, 6).contiguous()

    def estimate_lever_arm(self, st, end, cam_rots, cam_pos, ext_rot, weight=None, use_cov=False, gravity_norm=None, solve_scale=False):
        """Lever arm of the camera-IMU mount (the translation of ``rgb2imu_pose``), gravity, accelerometer bias, velocities and, with
        ``solve_scale``, the metric scale of the positions, of frames [st, end] from world poses of the CAMERA (``cam_rots``:
        (end - st + 1, 4) xyzw quaternions or an SO3, ``cam_pos``: (end - st + 1, 3); VO, no rgb2imu applied; monocular positions may be
        up to a scale), in closed form (islam_imu_lever_scale_solve).  ``ext_rot``: (4) xyzw, the rotation of ``rgb2imu_pose``, e.g. the
        q of ``estimate_extrinsic_rotation``; the body rotations ``cam_rots (x) ext_rot^-1`` are formed in float64.  The rows are
        built exactly as ``estimate_gravity_accel_bias`` builds them, and ``weight``, ``use_cov`` and ``gravity_norm`` mean what they mean
        there.  Returns (gravity (3) in the frame of the poses, ``accel_bias + b`` (3), the lever arm t (3) in the body frame, the scale
        s (a 0-d tensor, exactly 1 unless ``solve_scale``), the velocities of the BODY (end - st + 1, 3), the 10x10 normal matrix H in the
        order g, b, t, s), on the CPU in float64; the body position of pose i is ``s cam_pos_i - R_i t``.  The lever arm needs rotation
        between the frames and the scale needs acceleration: a stream without them raises IslamHipError (ISLAM_ENOTPD).  Order of calls:
        ``estimate_extrinsic_rotation``, then ``estimate_gyro_bias`` on the camera rotations conjugated by q, then this.  The module is
        not changed."""
        cam, ext = self._as_device(cam_rots, torch.float64), self._as_device(ext_rot, torch.float64).reshape(4)
        poss, weight = self._as_device(cam_pos, self.dtype), self._weight(weight)
        with torch.no_grad():
            # R_i = Rc_i R_x^T: the quaternion product of cam_i and the conjugate of ext
            x, y, z, w = cam.unbind(-1)
            cx, cy, cz, cw = -ext[0], -ext[1], -ext[2], ext[3]
            rots = torch.stack((w * cx + x * cw + y * cz - z * cy, w * cy - x * cz + y * cw + z * cx, w * cz + x * cy - y * cx + z * cw,
                                w * cw - x * cx - y * cy - z * cz), -1).to(self.dtype)
            n, dur, dvel, dpos, jac, cov = self._alignment_rows(st, end, use_cov)
            g, b, t, s, H, vel, _ = ops.imu_lever_scale_solve(rots, poss, dur, dvel, dpos, jac, cov, weight, True, bool(solve_scale),
                                                              gravity_norm)
            res = torch.cat((g, self.accel_bias.to(torch.float64) + b, t, s.reshape(1), vel.reshape(-1), H.reshape(100))).cpu()
        o = 10 + 3 * (n + 1)
        return (res[0:3].contiguous(), res[3:6].contiguous(), res[6:9].contiguous(), res[9].clone(), res[10:o].view(n + 1, 3).contiguous(),
                res[o:o + 100].view(10, 10).contiguous())

    def estimate_extrinsic_rotation(self, st, end, cam_rots, weight=None, delta=None, rounds=4, min_gap=None):
        """Rotation of the camera-IMU mount from the relative rotations of frames [st, end], in closed form
        (islam_imu_extrinsic_rot_solve; the rotation calibration of VINS-Mono).  ``cam_rots``: (end - st, 4) xyzw quaternions or an SO3,
        the CAMERA's relative rotation over frame i -> i + 1 (VO, in the camera's own frame, no rgb2imu applied).  The motion rows are
        integrated exactly as ``estimate_gyro_bias`` does (the module's current ``gyro_bias`` subtracted whatever ``optm_bias`` says;
        the denoiser is not run) and their rotations DR_i enter with ``cam_rots``: q minimises sum_i w_i rho_i |DR_i (x) q - q (x) cam_i|^2
        over unit quaternions.  ``weight``: (end - st) per frame; ``delta``: Huber threshold on the angular residual in rad (None = no
        reweighting) for ``rounds`` reweighted solves.  Returns (q (4) xyzw, the eigenvalues (4) ascending, the angular residuals
        (end - st) under q), on the CPU in float64.  q is the rotation of ``rgb2imu_pose`` (T_IL: body motion = T_IL camera motion
        T_IL^-1).  The eigenvalues are the observability diagnosis: rotations about one axis only leave q undetermined and give
        eig[1] ~ eig[0] without an error; with ``min_gap`` a ``ValueError`` is raised when (eig[1] - eig[0]) / eig[3] < min_gap.
        A gyro-bias error perturbs q at first order (it rotates every DR_i), so the order of calls is: this first, then
        ``estimate_gyro_bias`` on the camera rotations conjugated by q (q (x) cam_i (x) q^-1), then ``estimate_lever_arm``, which gives
        the lever arm (the translation of T_IL) with gravity, accelerometer bias and velocities (``estimate_gravity_accel_bias`` is the
        solve for a known lever arm).  Out of scope: the joint refinement of rotation and gyro bias; the time offset between the two
        sensors is ``estimate_time_offset``'s.  The module is not changed."""
        with torch.no_grad():
            seg_host, seg, dts, gyros, accels = self._window(st, end, self.gyro_bias)
            n = len(seg_host) - 1
            cam, weight = self._as_device(cam_rots, self.dtype), self._weight(weight)
            rot, _ = self._motion_rows(dts, gyros, accels, seg, seg_host, False)
            q, eig, res, _ = ops.imu_extrinsic_rot_solve(rot, cam, weight, delta, rounds)
            host = torch.cat((q, eig, res)).cpu()
        q, eig, res = host[0:4].contiguous(), host[4:8].contiguous(), host[8:8 + n].contiguous()
        gap = float(eig[1] - eig[0]) / float(eig[3]) if float(eig[3]) > 0.0 else 0.0
        if min_gap is not None and not gap >= float(min_gap):
            raise ValueError('estimate_extrinsic_rotation: the rotations of frames [%d, %d] do not span more than one axis: '
                             '(eig1 - eig0) / eig3 = %.3g < min_gap = %.3g' % (st, end, gap, min_gap))
        return q, eig, res
