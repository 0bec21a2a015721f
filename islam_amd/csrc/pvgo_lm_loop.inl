// pvgo_lm_loop.inl -- part of the pvgo.hip translation unit (textually included there; not compiled on its own).
// The host loops of islam_pvgo_run_chain[_reproj|_robust|_info] (reference pvgo.py:168-180): run_chain_impl sets a ChainRun up and picks one
// of three drivers -- run_fused (trial_elim_kernel), run_small (the whole loop in one launch), run_staged (a launch per stage).
// All of them run ahead of the device behind the epoch gate and only poll the pinned verdicts.

// What a run's drivers share: the problem, the workspace and its double buffers, the parameter blocks the kernels take, the verdict
// block, the optional factors and where the outcome goes.
struct ChainRun {
    double *nodes, *vels;
    ChainData d;
    const islam_pvgo_params* prm;
    Workspace w;
    hipStream_t s;
    TRParams tr; LinWeights W;
    // Two linearisation buffers: trial_lin_kernel linearises at the trial point into the other buffer (the next
    // optimizer.step() if the trial is accepted -- the common case); on a reject the old buffer (with its cumulatively
    // damped diagonal) is simply kept.
    double *LIN[2], *HD[2], *HO[2], *RH[2], *RED[2];
    int nlb;                                // workgroups of linbuild_kernel / trial_lin_kernel
    unsigned* ticket;
    int fz_m, fz_P, fz_nwg;                 // level 0 as trial_elim_kernel takes it: segment length, segments, workgroups
    VerdictBlock vb;
    const islam_pvgo_reproj* reproj; ReprojDev rp; const RobustDev* robust;      // optional factors / kernels (nullptr: none)
    const double *info_vo, *info_imu;       // per-factor information, packed (21, N-1) / (18, N-1); both nullptr: the scalars of prm->w
    bool info_imu9;                         // info_imu is (45, N-1): one correlated 9x9 per link
    islam_pvgo_result* result; double* trace; int trace_cap;
    LinBufs lin(int b) const { return LinBufs{LIN[b], HD[b], HO[b], RH[b]}; }
    int* eflag_none() const { return w.flags + 6; }            // a word nobody sets
};

static ChainRun chain_run(double* nodes, double* vels, const ChainData& d, const islam_pvgo_params* prm, const Workspace& w, hipStream_t s) {
    ChainRun r{};
    r.nodes = nodes; r.vels = vels; r.d = d; r.prm = prm; r.w = w; r.s = s;
    r.tr = tr_params(prm);
    r.W = lin_weights(prm);
    r.LIN[0] = w.lin; r.LIN[1] = w.lin2; r.HD[0] = w.Hd; r.HD[1] = w.Hd2; r.HO[0] = w.Ho; r.HO[1] = w.Ho2;
    r.RH[0] = w.rhs; r.RH[1] = w.rhs2; r.RED[0] = w.red; r.RED[1] = w.red2;
    r.nlb = (d.N + LB_NODES - 1) / LB_NODES;
    r.ticket = reinterpret_cast<unsigned*>(w.flags + 2);
    return r;
}

// Per-factor information: directly behind a linbuild_kernel / trial_lin_kernel launch, under that launch's
// gate, info_build_kernel (info9_build_kernel for the correlated layout) overwrites HD[b], HO[b], RH[b] from the LIN[b] it just wrote.
// The stored diagonal stays undamped.
static void enqueue_info_build(const ChainRun& r, int b, Gate gate) {
    if (!r.info_imu) return;
    const auto kernel = r.info_imu9 ? info9_build_kernel : info_build_kernel;
    hipLaunchKernelGGL(kernel, dim3((r.d.N + 63) / 64), dim3(64), 0, r.s, r.LIN[b], r.d.dts, r.d.N, r.info_vo, r.info_imu, r.W.vmin, r.W.vmax,
                       r.HD[b], r.HO[b], r.RH[b], gate);
}

// red_ready: RED[b] already holds the reduction at (xn)
static void enqueue_linbuild(const ChainRun& r, const double* xn, const double* xv, int b, bool red_ready) {
    if (r.reproj && !red_ready) enqueue_reproj_reduce(xn, nullptr, r.d.N - 1, r.rp, r.RED[b], r.s);
    launch_linbuild(xn, xv, r.d, r.W, r.lin(b), r.w.loss_part, r.reproj ? r.RED[b] : (const double*)nullptr, r.rp, Gate{nullptr, 0.0}, r.robust,
                    r.s);
    enqueue_info_build(r, b, Gate{nullptr, 0.0});
}

// trial `seq` of iteration c (cur + dx -> tri) and the linearisation at the trial point into buffer 1 - c.pb
static void launch_trial_lin(const ChainRun& r, const IterCfg& c, double seq, Gate gate) {
    const Workspace& w = r.w;
    const int ob = 1 - c.pb;
    const auto kernel = r.robust ? trial_lin_kernel<true> : trial_lin_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(xcd_grid(r.nlb) + 1), dim3(LB_THREADS), LB_DYN_BYTES, r.s, c.cur_n, c.cur_v, w.dx, r.d.poses, r.d.drots,
                       r.d.dtrans, r.d.dvels, r.d.dts, r.LIN[c.pb], r.d.N, c.tri_n, c.tri_v, w.part, w.state, w.flags, r.ticket, r.tr,
                       r.vb.dev_slot(seq), seq, r.reproj ? r.RED[c.pb] : (const double*)nullptr, r.reproj ? r.RED[ob] : (const double*)nullptr,
                       r.rp, r.W, r.LIN[ob], r.HD[ob], r.HO[ob], r.RH[ob], gate, (int*)nullptr, r.robust ? *r.robust : RobustDev{});
}

// one pass of PyPose's inner `while self.last <= self.loss`: damped solve on buffer pb, then trial + linearisation at
// the trial point into buffer 1-pb; every kernel is gated on `epoch`
static int enqueue_iter(const ChainRun& r, const IterCfg& c, double seq, double epoch) {
    const Workspace& w = r.w;
    const Gate gate{w.state, epoch};
    int rc = enqueue_solve(w, r.HD[c.pb], r.HO[c.pb], r.RH[c.pb], w.state, 0.0, r.d.N, r.prm->seg_len, w.dx, r.s, nullptr, nullptr, gate);
    if (rc != ISLAM_OK) return rc;
    // reprojection factor at the trial point Exp(dx)*cur: its r^T r joins the trial loss, and it IS the reduction of
    // the next linearisation if the trial is accepted
    if (r.reproj) enqueue_reproj_reduce(c.cur_n, w.dx, r.d.N - 1, r.rp, r.RED[1 - c.pb], r.s, gate);
    launch_trial_lin(r, c, seq, gate);
    enqueue_info_build(r, 1 - c.pb, gate);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// the arguments of one trial_elim_kernel launch on iteration c
enum FusedMode {
    FUSED_FIRST,        // dx = nullptr: linearise at the initial iterate into buffer c.pb, sum the initial loss, eliminate level 0 of solve 1
    FUSED_TRIAL_ELIM,   // trial `seq`, linearisation at the trial point into buffer 1 - c.pb, level 0 of solve seq + 1
    FUSED_TRIAL_ONLY    // nothing follows an accepted trial: no node blocks, no elimination (7 us against trial_lin_kernel's 10.6)
};
static FusedArgs fused_args(const ChainRun& r, const IterCfg& c, FusedMode mode, double seq, int* eprev) {
    const Workspace& w = r.w;
    const bool first = mode == FUSED_FIRST;
    const int ob = first ? c.pb : 1 - c.pb;
    FusedArgs fa{};
    fa.nodes = c.cur_n; fa.vels = c.cur_v; fa.dx = first ? (const double*)nullptr : w.dx; fa.poses = r.d.poses; fa.drots = r.d.drots;
    fa.dtrans = r.d.dtrans; fa.dvels = r.d.dvels; fa.dts = r.d.dts; fa.lin = first ? (const double*)nullptr : r.LIN[c.pb]; fa.N = r.d.N;
    fa.nodes_t = c.tri_n; fa.vels_t = c.tri_v; fa.part = w.part; fa.st = w.state; fa.flags = w.flags; fa.ticket = r.ticket; fa.tr = r.tr;
    fa.report = first ? (double*)nullptr : r.vb.dev_slot(seq); fa.seq = seq; fa.W = r.W;
    fa.lin_o = r.LIN[ob]; fa.Hd_o = r.HD[ob]; fa.Ho_o = r.HO[ob]; fa.rhs_o = r.RH[ob];
    fa.dst = level_dst(w.lv[0], w.dx);
    fa.m = r.fz_m; fa.P = r.fz_P; fa.nwg = r.fz_nwg;
    fa.eflag = mode == FUSED_TRIAL_ONLY ? r.eflag_none() : w.flags + 4 + (((long long)seq + 1) & 1);      // (by the parity of the solve)
    fa.eflag_prev = eprev;
    fa.Ms = r.d.N - 1;
    fa.trial_only = mode == FUSED_TRIAL_ONLY ? 1 : 0;
    return fa;
}
static void launch_fused(const ChainRun& r, const FusedArgs& fa, Gate gate) {
    hipLaunchKernelGGL(trial_elim_kernel, dim3(xcd_grid(r.fz_nwg) + 1), dim3(FZ_THREADS), FZ_LDS_BYTES, r.s, fa, gate);
}

// levels 1 .. root and the down-sweep behind a level 0 that trial_elim_kernel eliminated (-> dx)
static int enqueue_upper_levels(const ChainRun& r, const SolvePlan& sp, Gate gate) {
    LevelSrc none{};
    none.level0 = 1;
    return enqueue_levels(r.w, sp, 0, none, nullptr, r.w.dx, r.w.flags, r.s, nullptr, nullptr, gate, true);
}

// ---- the fused loop (default): trial t, the linearisation at its trial point and the level-0 elimination of solve t+1 in
// ONE launch (trial_elim_kernel), under a speculated damping the deciding workgroup validates.  Plans it does not cover
// (one-sided levels, segments longer than FZ_MAXM, a single level), the reprojection factor, robust kernels, per-factor information and
// ISLAM_PVGO_NO_FUSE=1 take the launch-per-stage loop below.
static int run_fused(ChainRun& r, const SolvePlan& sp, int fz_nwg) {
    const Workspace& w = r.w;
    r.fz_m = sp.lv[0].m; r.fz_P = sp.lv[0].P; r.fz_nwg = fz_nwg;
    int rc = ensure_fused_lds();
    if (rc != ISLAM_OK) return rc;
    IterCfg A{0, r.nodes, r.vels, w.nodes_t, w.vels_t};       // the iteration whose verdict is awaited
    islam_pvgo_result t{};
    double epoch = 1.0;
    // the first solve: the same kernel in its `first` mode (dx = nullptr) linearises at the initial iterate, sums the initial loss
    // and eliminates level 0 with the initial damping -- linbuild_kernel + the launched level-0 kernel only on the fallback paths
    launch_fused(r, fused_args(r, A, FUSED_FIRST, 0.0, r.eflag_none()), Gate{w.state, epoch});
    if ((rc = enqueue_upper_levels(r, sp, Gate{w.state, epoch})) != ISLAM_OK) return rc;
    bool prev_fused = true;                                   // level 0 of solve `seq` ran inside the previous trial_elim_kernel
    for (;;) {
        const double seq = (double)(t.trials + 1);
        const IterCfg B{1 - A.pb, A.tri_n, A.tri_v, A.cur_n, A.cur_v};
        const Gate gate{w.state, epoch};
        // evaluates trial `seq` of iteration A (cur + dx -> tri); more: also eliminates level 0 of solve seq+1 and enqueues its upper
        // levels + down-sweep (-> dx)
        // (an accepted trial that would be the last optimizer step anyway -- StopOnPlateau's step limit -- needs no next solve)
        const bool more = t.steps + 1 < r.prm->max_steps;
        int* const eprev = prev_fused ? w.flags + 4 + ((long long)seq & 1) : r.eflag_none();
        launch_fused(r, fused_args(r, A, more ? FUSED_TRIAL_ELIM : FUSED_TRIAL_ONLY, seq, eprev), gate);
        if (!more) ISLAM_LAUNCH_CHECK();
        else if ((rc = enqueue_upper_levels(r, sp, gate)) != ISLAM_OK) return rc;
        volatile double* hs = r.vb.slot(seq);
        if ((rc = wait_verdict(hs, seq, r.s, "islam_pvgo_run_chain: no status from the device (trial %d)")) != ISLAM_OK) return rc;
        const int verdict = take_verdict(t, hs);
        if (verdict == 9) return fail(ISLAM_EHIP, "islam_pvgo_run_chain: the deciding workgroup of trial %d gave up waiting for the level's workgroups", t.trials);
        record_trace(r.trace, r.trace_cap, t.trials, verdict, hs);
        if (verdict == 0) {               // accepted, the speculated damping was right: solve seq+1 is already running
            A = B;
            prev_fused = true;
            continue;
        }
        epoch += 1.0;                     // any other verdict bumped the device epoch: the launches queued behind are no-ops
        if (verdict == 2) { A = B; break; }
        if (verdict == 4) { t.status = ISLAM_ENOTPD; break; }
        // the speculative level-0 elimination (if there was one) is void: clear its error word; the next solve runs on the
        // launched kernels from the linearisation in global memory
        if (more) ISLAM_HIP_CHECK(hipMemsetAsync(w.flags + 4 + (((long long)seq + 1) & 1), 0, sizeof(int), r.s));
        if (verdict == 5) A = B;          // accepted with another damping: the trial point's linearisation is in the other buffers
        if (verdict == 3) t.status = ISLAM_ENOTPD;    // "Linear solver failed. Breaking optimization step...": same iterate, same
                                                      // (undamped) linearisation, StopOnPlateau's plateau counter ends the loop
        // every solve keeps the stored diagonal undamped and applies the damping history of the current linearisation (LevelSrc::hist)
        LevelSrc src{};
        src.level0 = 1; src.Hd = r.HD[A.pb]; src.Ho = r.HO[A.pb]; src.rhs0 = r.RH[A.pb]; src.state = w.state; src.hist = 1;
        if ((rc = enqueue_levels(w, sp, 0, src, nullptr, w.dx, w.flags, r.s, nullptr, nullptr, Gate{w.state, epoch})) != ISLAM_OK) return rc;
        prev_fused = false;
    }
    if ((rc = copy_back_if_moved(r.nodes, r.vels, A.cur_n, A.cur_v, r.d.N, r.s)) != ISLAM_OK) return rc;
    *r.result = t;
    return ISLAM_OK;
}

// ---- small graphs (one segment, one block of links: the reference's own per-batch window of 9 nodes): the whole loop in ONE launch
static int run_small(ChainRun& r) {
    const Workspace& w = r.w;
    const int N = r.d.N;
    constexpr int SMALL_LDS = LB_DYN_BYTES + 2 * LDS_PER_WAVE * (int)sizeof(double);
    static bool small_lds_set[64] = {};
    int rc = ensure_dynamic_lds({(const void*)small_lm_kernel}, SMALL_LDS, small_lds_set);
    if (rc != ISLAM_OK) return rc;
    static thread_local double* host_trace = nullptr;       // pinned rows for the optional trace (3 per trial)
    constexpr int TRACE_ROWS = 1024;
    double* trace_dev = nullptr;
    if (r.trace && r.trace_cap > 0) {
        if (!host_trace) ISLAM_HIP_CHECK(hipHostMalloc((void**)&host_trace, 3 * TRACE_ROWS * sizeof(double), hipHostMallocMapped | hipHostMallocPortable));
        ISLAM_HIP_CHECK(hipHostGetDevicePointer((void**)&trace_dev, host_trace, 0));
    }
    SmallArgs sa{};
    sa.nodes = r.nodes; sa.vels = r.vels; sa.poses = r.d.poses; sa.drots = r.d.drots; sa.dtrans = r.d.dtrans; sa.dvels = r.d.dvels;
    sa.dts = r.d.dts; sa.N = N;
    sa.nodes_t = w.nodes_t; sa.vels_t = w.vels_t; sa.dx = w.dx;
    for (int i = 0; i < 2; ++i) { sa.LIN[i] = r.LIN[i]; sa.HD[i] = r.HD[i]; sa.HO[i] = r.HO[i]; sa.RH[i] = r.RH[i]; }
    sa.loss_part = w.loss_part; sa.st = w.state; sa.flags = w.flags; sa.tr = r.tr; sa.W = r.W;
    sa.dst = level_dst(w.lv[0], w.dx);
    sa.report = r.vb.dev; sa.trace = trace_dev; sa.trace_cap = std::min(r.trace_cap, TRACE_ROWS); sa.marker = 7.0;
    // two segments around a separator (ISLAM_SMALL_LM_ONE_SEGMENT=1: the one-segment sweep of rounds 3-5, A/B runs)
    const int m0 = (!env_is("ISLAM_SMALL_LM_ONE_SEGMENT", '1') && N >= 3) ? (N - 1) / 2 : 0;
    sa.m0 = m0;
    if (m0 > 0) {
        sa.P0 = (N + m0) / (m0 + 1);
        sa.n1 = N / (m0 + 1);
        sa.src1 = level_src_from(w.lv[0], sa.P0);
        sa.dst1 = level_dst(w.lv[1], w.lv[1].x);
    }
    hipLaunchKernelGGL(small_lm_kernel, dim3(1), dim3(LB_THREADS), SMALL_LDS, r.s, sa);
    ISLAM_LAUNCH_CHECK();
    volatile double* hs = r.vb.host;                         // (one verdict for the whole run, in slot 0, marked 7.0)
    if ((rc = wait_verdict(hs, sa.marker, r.s, "islam_pvgo_run_chain: no status from the device (small-graph loop)")) != ISLAM_OK) return rc;
    *r.result = islam_pvgo_result{(int)hs[13], (int)hs[11], (int)hs[10], hs[0], hs[2]};       // steps, trials, status, loss, damping
    if (r.trace && r.trace_cap > 0) {
        const int nt = std::min(r.result->trials, sa.trace_cap);
        for (int i = 0; i < 3 * nt; ++i) r.trace[i] = host_trace[i];
    }
    return ISLAM_OK;
}

// ---- the launch-per-stage loop: solve, trial + linearisation at the trial point, one iteration ahead of the verdicts
static int run_staged(ChainRun& r) {
    IterCfg A{0, r.nodes, r.vels, r.w.nodes_t, r.w.vels_t};   // the iteration whose verdict is awaited
    islam_pvgo_result t{};
    double epoch = 1.0;
    int rc = enqueue_iter(r, A, 1.0, epoch);
    if (rc != ISLAM_OK) return rc;
    for (;;) {
        const double seq = (double)(t.trials + 1);
        // run ahead: the next iteration under the assumption "trial accepted, loop continues" -- unless an accepted trial
        // would be the last optimizer step anyway (StopOnPlateau's step limit): nothing can follow it
        const IterCfg B{1 - A.pb, A.tri_n, A.tri_v, A.cur_n, A.cur_v};
        if (t.steps + 1 < r.prm->max_steps && (rc = enqueue_iter(r, B, seq + 1.0, epoch)) != ISLAM_OK) return rc;
        // wait for the verdict (poll the pinned status block; fall back to a stream sync after ~2 s)
        volatile double* hs = r.vb.slot(seq);
        if ((rc = wait_verdict(hs, seq, r.s, "islam_pvgo_run_chain: no status from the device (trial %d)")) != ISLAM_OK) return rc;
        const int verdict = take_verdict(t, hs);
        record_trace(r.trace, r.trace_cap, t.trials, verdict, hs);      // (this loop never sees verdict 5)
        if (verdict == 0) {               // accepted, continue: B is the iteration now in flight
            A = B;
            continue;
        }
        epoch += 1.0;                     // any other verdict bumped the device epoch: B's kernels are no-ops
        if (verdict == 1) {               // rejected: same iterate, same (cumulatively damped) linearisation
            if ((rc = enqueue_iter(r, A, seq + 1.0, epoch)) != ISLAM_OK) return rc;
            continue;
        }
        if (verdict == 2) { A = B; break; }      // accepted, StopOnPlateau says stop
        t.status = ISLAM_ENOTPD;          // "Linear solver failed. Breaking optimization step..."
        if (verdict == 4) break;
        // PyPose keeps looping through the scheduler (the plateau counter stops it): same iterate, new linearisation
        enqueue_linbuild(r, A.cur_n, A.cur_v, A.pb, true);
        if ((rc = enqueue_iter(r, A, seq + 1.0, epoch)) != ISLAM_OK) return rc;
    }
    if ((rc = copy_back_if_moved(r.nodes, r.vels, A.cur_n, A.cur_v, r.d.N, r.s)) != ISLAM_OK) return rc;
    *r.result = t;
    return ISLAM_OK;
}

// setup, the choice of the driver, the call
static int run_chain_impl(double* nodes, double* vels, const ChainData& d, const islam_pvgo_params* prm, const islam_pvgo_reproj* reproj,
                          const ReprojDev& rp, const Workspace& w, hipStream_t s, islam_pvgo_result* result, double* trace, int trace_cap,
                          const RobustDev* robust, const double* info_vo = nullptr, const double* info_imu = nullptr,
                          bool info_imu9 = false) {
    const int N = d.N;
    ChainRun r = chain_run(nodes, vels, d, prm, w, s);
    r.reproj = reproj; r.rp = rp; r.robust = robust; r.result = result; r.trace = trace; r.trace_cap = trace_cap;
    r.info_vo = info_vo; r.info_imu = info_imu; r.info_imu9 = info_imu9;
    const bool info = info_imu != nullptr;         // information lives in the launch-per-stage loop only
    int rc = r.vb.acquire();
    if (rc != ISLAM_OK) return rc;
    // device state and flags (flags[0] solver error, flags[2] ticket) initialised by a one-wave kernel: a host->device copy of a
    // stack array stalls the host for a staging round trip at the start of every run_pvgo
    if ((rc = enqueue_control_init(w, prm, s)) != ISLAM_OK) return rc;
    if ((rc = ensure_linbuild_lds()) != ISLAM_OK) return rc;
    SolvePlan sp;
    plan_levels(N, prm->seg_len, sp, solve_twisted());
    const bool no_fuse = env_is("ISLAM_PVGO_NO_FUSE", '1');      // (read per call: A/B tests)
    // (one workgroup of FZ_S segments per CU: the whole level must be resident at once)
    // (the deciding workgroup is one more block with the same LDS footprint: it is dispatched to XCD 0, which must keep a CU free
    // for it -- otherwise it starts when the first workgroup exits and the launch ends ~4 us late)
    const int fz_nwg = std::min(sp.lv[0].P, std::max(device_cus() - fz_spare_cus(), 1));
    // (small graphs -- the reference's own per-batch problem is 9 nodes, run_kitti.sh -- stay on the launch-per-stage loop: its launches
    // are cheaper than the fused kernel's fixed cost and a rejected trial costs no mis-speculated chain.  Measured per run_pvgo, fused /
    // launch-per-stage: N = 9 (18 trials) 1059 / 723 us, N = 65 206 / 190 us, N = 129 203 / 236 us, N = 513 443 / 508 us.)
    const bool fused = !no_fuse && !reproj && !robust && !info && N > 96 && sp.nl >= 2 && fused_plan_core(sp, sp.lv[0].P, fz_nwg) &&
                       prm->reject < STATE_DOUBLES - STATE_HIST - 1;
    if (fused) return run_fused(r, sp, fz_nwg);
    enqueue_linbuild(r, nodes, vels, 0, false);
    hipLaunchKernelGGL(control_begin_kernel, dim3(1), dim3(64), 0, s, w.loss_part, r.nlb, w.state, w.flags);
    const bool no_small = env_is("ISLAM_PVGO_NO_SMALL", '1');      // (read per call: A/B tests)
    // (one wave eliminates the window's nodes one after the other, ~2 us each: beyond a couple of dozen nodes the level tree of the
    // launch-per-stage loop is faster -- N = 65 takes 190 us per run there)
    constexpr int SMALL_MAX_N = 16;
    if (!no_small && !reproj && !robust && !info && N <= SMALL_MAX_N) return run_small(r);
    return run_staged(r);
}
