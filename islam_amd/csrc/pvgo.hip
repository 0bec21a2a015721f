// PVGO back-end on gfx950: SE(3) Levenberg-Marquardt over VO / IMU factors on a chain graph, fp64.
//
// Replaces (reference file:line under /root/reference):
//   pvgo.py:26-64    PoseVelGraph.forward        -> linearize_kernel / trial_kernel (residuals)
//   pvgo.py:168-180  pp.optim.LM + TrustRegion + StopOnPlateau loop -> islam_pvgo_run_chain
//   pvgo.py:67-78    vo_loss (+ PyPose backward)  -> vo_loss_{fwd,bwd}_kernel
//   pvgo.py:114-119  align_to                     -> align_kernel
//   PyPose (external, un-vendored): modjac/jacrev Jacobian, J^T W J, cholesky_ex/cholesky_solve,
//   LieTensor.add_ -- restated from its published algorithm (SURVEY.md section 8a box).
//
// Design: the reference materialises a dense (rows x 10N) Jacobian, a dense
// block_diag weight and a dense 10N x 10N normal matrix.  The graph is a chain, so the normal
// matrix is block-tridiagonal with 9x9 blocks [rho phi v] per node.  We
//   1. linearise per link (one lane per link, everything in registers),
//   2. build the 9x9 diagonal / coupling blocks per node (gather from the two adjacent links,
//      no atomics, deterministic),
//   3. factor with a partitioned ("spike") block LDL^T: the chain is cut into segments, each
//      segment's interior is eliminated onto its two separator nodes -- by two wavefronts that start
//      at the two ends and meet at the middle node (bt_eliminate_tw_kernel, "twisted"; the one-sided
//      bt_eliminate_kernel serves segment lengths the twisted path does not handle) -- one launch per level; the separators
//      form a ~6x smaller chain that is reduced the same way;
//      the root solve and the whole back-substitution run in ONE launch (bt_downsweep_kernel) with
//      per-segment ready words and write-through hand-off between levels.  Inside a wavefront one
//      lane owns one column of the augmented 9 x 28 matrix [S | U | F^T | g]; pivots are broadcast
//      with v_readlane, the 19x19 Schur update runs over all 64 lanes from an LDS copy,
//   4. apply the step on a trial copy, re-evaluate the loss and the trust-region ratio per link AND
//      linearise at the trial point for the next step in the same launch (trial_lin_kernel); one
//      extra workgroup waits for all partial sums, takes the LM / TrustRegion / StopOnPlateau decision
//      and writes a 128-byte verdict to pinned host memory,
//   5. the host enqueues one iteration ahead (every kernel is gated on an epoch the deciding lane
//      bumps on any verdict other than "accepted, continue") and only polls the verdicts.
// linearize_kernel / build_normal_kernel / trial_kernel / bt_top_kernel / bt_backsub_kernel are the
// stage-level versions behind the islam_pvgo_* entry points the sharded driver and the tests call.
//
// Layout of this translation unit: device parts, host helpers and planner, the loop drivers (single GPU, then sharded), ONE
// extern "C" block with every entry point, the marginal covariances (chains, then loop-closure graphs in band form).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "common.h"
#include "lie_dev.h"
#include "pvgo_internal.h"

using namespace islam;

namespace {

constexpr int LIN_C = 42;   // doubles per link record (component-major: lin[c*M + k])
constexpr int FAC = 252;    // 28 columns x 9 rows stored per eliminated node
constexpr int XS = 10;      // padded column stride of the LDS copies (16-byte aligned columns)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

#ifdef ISLAM_PROBE
__device__ long long islam_probe_buf[1024];
#define PROBE_AT(cond, slot) do { __builtin_amdgcn_sched_barrier(0); if (cond) islam_probe_buf[(slot)] = clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define PROBE_WALL(cond, slot) do { __builtin_amdgcn_sched_barrier(0); if (cond) islam_probe_buf[(slot)] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PROBE_AT(cond, slot) do { } while (0)
#define PROBE_WALL(cond, slot) do { } while (0)
#endif

// XCD-aware work mapping.  Workgroup b is observed to run on XCD b % 8 (MI355X_MICROARCH.md, dispatch section; speed
// only, never correctness).  Every kernel of the LM loop splits its node / link / segment range into 8 CONTIGUOUS parts,
// part x handled by the workgroups with b % 8 == x, so data produced for a stretch of the chain stays in the L2 of the XCD
// that consumes it in the next launch (the levels of the block solver hand ~4 KB per segment to each other).
// Launch with xcd_grid(total) workgroups; returns the logical index or -1 for the padding workgroups.
__host__ __device__ __forceinline__ int xcd_grid(int total) { return 8 * ((total + 7) / 8); }
__device__ __forceinline__ int xcd_index(int b, int total) {
    const int Q = (total + 7) / 8;
    const int s = (b & 7) * Q + (b >> 3);
    return s < total ? s : -1;
}

__device__ __forceinline__ double bcast(double v, int src) {   // src must be wave-uniform
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, src);
    hi = __builtin_amdgcn_readlane(hi, src);
    return __hiloint2double(hi, lo);
}

// Agent-coherent accesses (global_store / global_load with sc1: written through to / read from the level every XCD
// sees).  Data handed from one workgroup to another INSIDE a launch goes through these, so that publishing needs no
// release fence: an agent-scope release is a write-back walk of the XCD's whole L2 (microseconds when many waves do it).
__device__ __forceinline__ void st_coherent(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_coherent(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (the run-ahead gate -- struct Gate, gate_closed -- lives in pvgo_internal.h)

#include "pvgo_linearize.inl"   // link residuals, Jacobian blocks, normal equations, the sparse reprojection factor, linbuild_kernel
#include "pvgo_solver.inl"   // partitioned / twisted block-tridiagonal LDL^T
#include "pvgo_lm_kernels.inl"   // device side of the LM loop
#include "pvgo_general.inl"   // control kernels, retraction, arbitrary-topology assembly, vo_loss / imu_loss forward + backward, align_to
}  // namespace

// error path of a run (abandon_run): an epoch no enqueued kernel carries turns everything still queued into no-ops
__global__ void close_gate_kernel(double* __restrict__ st) {
    if (threadIdx.x == 0) st[14] = -1.0;
}

namespace {
#include "pvgo_host.inl"   // host side: planner, workspace, launchers, what the loop drivers and the entry points share
#include "pvgo_lm_loop.inl"   // the single-GPU LM loop: run_chain_impl and its three drivers

// validation, workspace and the error path shared by the islam_pvgo_run_chain_* entry points
int run_chain_entry(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                    const double* dvels, const double* dts, int N, const islam_pvgo_params* prm,
                    const islam_pvgo_reproj* reproj, const islam_pvgo_robust* robust, void* workspace,
                    size_t workspace_bytes, islam_pvgo_result* result, double* trace, int trace_cap, void* stream,
                    const double* info_vo = nullptr, const double* info_imu = nullptr, bool info_imu9 = false) {
    if (N < 2) return fail(ISLAM_EARG, "islam_pvgo_run_chain: N=%d < 2", N);
    if (!prm || !result) return fail(ISLAM_EARG, "islam_pvgo_run_chain: null params/result");
    if ((info_vo == nullptr) != (info_imu == nullptr))
        return fail(ISLAM_EARG, "islam_pvgo_run_chain_info%s: info_vo and info_imu must both be given or both be NULL", info_imu9 ? "9" : "");
    int rc;
    ReprojDev rp{};
    if (reproj && (rc = reproj_dev(reproj, rp)) != ISLAM_OK) return rc;
    RobustDev rb{};
    bool robust_on = false;
    if (robust && (rc = robust_dev(robust, rb, &robust_on)) != ISLAM_OK) return rc;
    Workspace w;
    rc = workspace_or_fail("islam_pvgo_run_chain: workspace %zu < %zu bytes", N, workspace, workspace_bytes, w);
    if (rc != ISLAM_OK) return rc;
    hipStream_t s = as_stream(stream);
    rc = run_chain_impl(nodes, vels, ChainData{poses, drots, dtrans, dvels, dts, N}, prm, reproj, rp, w, s, result, trace, trace_cap,
                        robust_on ? &rb : nullptr, info_vo, info_imu, info_imu9);
    return rc == ISLAM_OK ? rc : abandon_run(w.state, s, rc);
}

// validation, the memset and the two launches shared by islam_pvgo_assemble_dense / _scaled / _info (c_vo with EW_SCALED, info_vo with EW_INFO)
int assemble_dense_entry(const char* name, EdgeWeight mode, const double* Hd, const double* Ho, const double* rhs_chain, const double* vo,
                         const double* c_vo, const double* info_vo, const int64_t* edges, const int64_t* node_ptr,
                         const int64_t* node_adj, double w0, int N, int E, double* A, double* rhs, void* stream) {
    if (N < 2 || E < 0 || (E > 0 && ((mode == EW_SCALED && !c_vo) || (mode == EW_INFO && (!info_vo || !vo)))))
        return fail(ISLAM_EARG, "%s: N=%d E=%d, vo %p, c_vo %p, info_vo %p", name, N, E, (const void*)vo, (const void*)c_vo, (const void*)info_vo);
    const auto nodes_k = mode == EW_INFO ? dense_nodes_kernel<EW_INFO> : mode == EW_SCALED ? dense_nodes_kernel<EW_SCALED> : dense_nodes_kernel<EW_PLAIN>;
    const auto edges_k = mode == EW_INFO ? dense_edges_kernel<EW_INFO> : mode == EW_SCALED ? dense_edges_kernel<EW_SCALED> : dense_edges_kernel<EW_PLAIN>;
    hipStream_t s = as_stream(stream);
    ISLAM_HIP_CHECK(hipMemsetAsync(A, 0, (size_t)81 * N * N * sizeof(double), s));
    hipLaunchKernelGGL(nodes_k, dim3((N + 63) / 64), dim3(64), 0, s, Hd, Ho, rhs_chain, vo, c_vo, info_vo, node_ptr, node_adj, w0, N, E, A, rhs);
    if (E > 0) hipLaunchKernelGGL(edges_k, dim3((E + 63) / 64), dim3(64), 0, s, vo, c_vo, info_vo, edges, w0, N, E, A);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}
}  // namespace

#include "pvgo_sharded.inl"   // the sharded LM loop: ranges of a rank, gated stages, run_chain_sharded_fused

extern "C" {

void islam_pvgo_default_params(islam_pvgo_params* p) {
    p->w[0] = p->w[1] = p->w[2] = p->w[3] = 1.0;
    p->radius = 1e4;
    p->vmin = 1e-4;
    p->vmax = 1e32;
    p->high = 0.5; p->low = 1e-3; p->up = 2.0; p->down = 0.5; p->factor = 0.5; p->rmin = 1e-6; p->rmax = 1e16;
    p->reject = 16;
    p->max_steps = 10;
    p->patience = 3;
    p->decreasing = 1e-3;
    p->seg_len[0] = p->seg_len[1] = 0;
}

size_t islam_pvgo_workspace_bytes(int N) {
    if (N < 1) return 0;
    return carve(nullptr, N).bytes + 256;
}

int islam_pvgo_linearize(const double* nodes, const double* vels, const double* poses, const double* drots,
                         const double* dtrans, const double* dvels, const double* dts, int N, double* lin,
                         double* loss_part, void* stream) {
    if (N < 2) return fail(ISLAM_EARG, "islam_pvgo_linearize: N=%d < 2", N);
    const int M = N - 1, nblk = (M + 63) / 64;
    hipLaunchKernelGGL(linearize_kernel, dim3(nblk), dim3(64), 0, as_stream(stream), nodes, vels, poses, drots, dtrans,
                       dvels, dts, M, lin, loss_part);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_build_normal(const double* lin, const double* dts, int N, const double w[4], double vmin, double vmax,
                            double* Hd, double* Ho, double* rhs, void* stream) {
    if (N < 2) return fail(ISLAM_EARG, "islam_pvgo_build_normal: N=%d < 2", N);
    hipLaunchKernelGGL(build_normal_kernel<false>, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), lin, dts, N, w[0], w[1],
                       w[2], w[3], vmin, vmax, Hd, Ho, rhs, (const double*)nullptr);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_build_normal_scaled(const double* lin, const double* dts, int N, const double w[4], const double* c_imu,
                                   double vmin, double vmax, double* Hd, double* Ho, double* rhs, void* stream) {
    if (N < 2 || !c_imu) return fail(ISLAM_EARG, "islam_pvgo_build_normal_scaled: N=%d < 2 or null c_imu", N);
    hipLaunchKernelGGL(build_normal_kernel<true>, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), lin, dts, N, w[0], w[1],
                       w[2], w[3], vmin, vmax, Hd, Ho, rhs, c_imu);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// per-factor information matrices (pvgo.py:133-162,178): info_vo == NULL leaves the VO group out
int islam_pvgo_build_normal_info(const double* lin, const double* dts, int N, const double* info_vo, const double* info_imu, double vmin,
                                 double vmax, double* Hd, double* Ho, double* rhs, void* stream) {
    if (N < 2 || !lin || !dts || !info_imu || !Hd || !Ho || !rhs)
        return fail(ISLAM_EARG, "islam_pvgo_build_normal_info: N=%d < 2 or a null lin / dts / info_imu / output", N);
    hipLaunchKernelGGL(info_build_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), lin, dts, N, info_vo, info_imu, vmin, vmax, Hd,
                       Ho, rhs, Gate{nullptr, 0.0});
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

// one correlated 9x9 per link: info_imu9 (45, N-1)
int islam_pvgo_build_normal_info9(const double* lin, const double* dts, int N, const double* info_vo, const double* info_imu9, double vmin,
                                  double vmax, double* Hd, double* Ho, double* rhs, void* stream) {
    if (N < 2 || !lin || !dts || !info_imu9 || !Hd || !Ho || !rhs)
        return fail(ISLAM_EARG, "islam_pvgo_build_normal_info9: N=%d < 2 or a null lin / dts / info_imu9 / output", N);
    hipLaunchKernelGGL(info9_build_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), lin, dts, N, info_vo, info_imu9, vmin, vmax,
                       Hd, Ho, rhs, Gate{nullptr, 0.0});
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_solve_chain(double* Hd, const double* Ho, const double* rhs, double damping, int N, const int seg_len[2],
                           void* workspace, size_t workspace_bytes, double* dx, void* stream) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_solve_chain: N=%d < 1", N);
    Workspace w;
    int rc = workspace_or_fail("islam_pvgo_solve_chain: workspace %zu < %zu bytes", N, workspace, workspace_bytes, w);
    if (rc != ISLAM_OK) return rc;
    hipStream_t s = as_stream(stream);
    ISLAM_HIP_CHECK(hipMemsetAsync(w.flags, 0, 4 * sizeof(double), s));
    ISLAM_HIP_CHECK(hipMemsetAsync(w.ready, 0, w.ready_bytes, s));
    rc = enqueue_solve(w, Hd, Ho, rhs, nullptr, damping, N, seg_len, dx, s);
    if (rc != ISLAM_OK) return rc;
    int flag = 0;
    ISLAM_HIP_CHECK(hipMemcpyAsync(&flag, w.flags, sizeof(int), hipMemcpyDeviceToHost, s));
    ISLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (flag) return fail(ISLAM_ENOTPD, "islam_pvgo_solve_chain: non-positive pivot (matrix not positive definite)");
    return ISLAM_OK;
}

// Stream-ordered variant of islam_pvgo_solve_chain: enqueue only, no read-back and no synchronisation (an iterative method
// calls it hundreds of times with the same matrix).  islam_pvgo_solve_status() reports, after a stream synchronisation,
// whether ANY solve enqueued on this workspace since the last status call met a non-positive pivot.
int islam_pvgo_solve_chain_enqueue(double* Hd, const double* Ho, const double* rhs, double damping, int N, const int seg_len[2],
                                   void* workspace, size_t workspace_bytes, double* dx, void* stream) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_solve_chain_enqueue: N=%d < 1", N);
    Workspace w;
    const int rc = workspace_or_fail("islam_pvgo_solve_chain_enqueue: workspace %zu < %zu bytes", N, workspace, workspace_bytes, w);
    if (rc != ISLAM_OK) return rc;
    return enqueue_solve(w, Hd, Ho, rhs, nullptr, damping, N, seg_len, dx, as_stream(stream));
}

// 0: every solve since the last call was positive definite; ISLAM_ENOTPD otherwise.  Also (re)initialises the workspace's
// status and hand-off words: call it once BEFORE the first islam_pvgo_solve_chain_enqueue on a fresh workspace.
int islam_pvgo_solve_status(int N, void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 1 || workspace_bytes < islam_pvgo_workspace_bytes(N)) return fail(ISLAM_EARG, "islam_pvgo_solve_status: bad workspace");
    Workspace w = carve((void*)align_up((size_t)workspace), N);
    hipStream_t s = as_stream(stream);
    int flag = 0;
    ISLAM_HIP_CHECK(hipMemcpyAsync(&flag, w.flags, sizeof(int), hipMemcpyDeviceToHost, s));
    ISLAM_HIP_CHECK(hipStreamSynchronize(s));
    ISLAM_HIP_CHECK(hipMemsetAsync(w.flags, 0, 4 * sizeof(double), s));
    ISLAM_HIP_CHECK(hipMemsetAsync(w.ready, 0, w.ready_bytes, s));
    if (flag) return fail(ISLAM_ENOTPD, "islam_pvgo_solve_status: non-positive pivot (matrix not positive definite)");
    return ISLAM_OK;
}

// Profiling variant of islam_pvgo_solve_chain: HIP events around every launch of one solve, on the stream the
// kernels run on.  ms[i] = duration of launch i (eliminate level 0..L-1, then back-substitution L-2..0);
// plan[3*l+0..2] = (nodes, segment length, segments) of level l.  Returns the number of launches in *nlaunch.
int islam_pvgo_solve_chain_timed(double* Hd, const double* Ho, const double* rhs, double damping, int N,
                                 const int seg_len[2], void* workspace, size_t workspace_bytes, double* dx, float* ms,
                                 int* plan_out, int* nlaunch, void* stream) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_solve_chain_timed: N=%d < 1", N);
    Workspace w;
    int rc = workspace_or_fail("islam_pvgo_solve_chain_timed: workspace too small", N, workspace, workspace_bytes, w);
    if (rc != ISLAM_OK) return rc;
    hipStream_t s = as_stream(stream);
    ISLAM_HIP_CHECK(hipMemsetAsync(w.ready, 0, w.ready_bytes, s));
    hipEvent_t evs[2 * MAXL + 2];
    for (auto& e : evs) ISLAM_HIP_CHECK(hipEventCreate(&e));
    ISLAM_HIP_CHECK(hipMemsetAsync(w.flags, 0, 4 * sizeof(double), s));
    int ne = 0;
    rc = enqueue_solve(w, Hd, Ho, rhs, nullptr, damping, N, seg_len, dx, s, evs, &ne);
    if (rc != ISLAM_OK) return rc;
    ISLAM_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i + 1 < ne; ++i) ISLAM_HIP_CHECK(hipEventElapsedTime(&ms[i], evs[i], evs[i + 1]));
    for (auto& e : evs) (void)hipEventDestroy(e);
    SolvePlan sp;
    plan_levels(N, seg_len, sp, solve_twisted());
    write_plan(sp, plan_out);
    *nlaunch = ne - 1;
    return ISLAM_OK;
}

// Measurement hook (bench.py's roofline leg): exactly the level-0 up-sweep launch of islam_pvgo_solve_chain -- same
// kernel, grid and arguments -- and nothing else.  Hd's diagonal is damped in place like in a solve.
int islam_pvgo_eliminate_level0(double* Hd, const double* Ho, const double* rhs, double damping, int N, const int seg_len[2],
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_eliminate_level0: N=%d < 1", N);
    Workspace w;
    const int rc = workspace_or_fail("islam_pvgo_eliminate_level0: workspace too small", N, workspace, workspace_bytes, w);
    if (rc != ISLAM_OK) return rc;
    SolvePlan sp;
    if (plan_levels(N, seg_len, sp, solve_twisted()) < 2) return fail(ISLAM_EARG, "islam_pvgo_eliminate_level0: single-level problem");
    LevelSrc src{};
    src.level0 = 1; src.Hd = Hd; src.Ho = Ho; src.rhs0 = rhs; src.state = nullptr; src.damping_override = damping;
    const int rc_l = launch_eliminate(sp.lv[0], sp.twisted != 0, src, level_dst(w.lv[0], w.lv[0].x), w.flags, as_stream(stream), Gate{nullptr, 0.0});
    if (rc_l != ISLAM_OK) return rc_l;
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_plan(int N, const int seg_len[2], int* plan9) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_plan: N=%d < 1", N);
    SolvePlan sp;
    const int nl = shard_plan(N, seg_len, sp);
    write_plan(sp, plan9);
    return nl;
}

int islam_pvgo_shard_ranges(int N, const int seg_len[2], int world, int rank, int* out) {
    SolvePlan sp;
    const int nl = shard_plan(N, seg_len, sp);
    ShardRanges R;
    if (nl < 2 || shard_ranges(sp, world, rank, R) != 0)
        return fail(ISLAM_EARG, "islam_pvgo_shard_ranges: N=%d cannot be split over %d ranks (rank %d)", N, world, rank);
    out[0] = R.xl;
    out[1] = sp.lv[R.xl].P;
    for (int l = 0; l < MAXL; ++l) { out[2 + 2 * l] = R.seg0[l]; out[3 + 2 * l] = R.nseg[l]; }
    return ISLAM_OK;
}

int islam_pvgo_shard_upsweep(double* Hd, const double* Ho, const double* rhs, double damping, int N, const int seg_len[2], int world,
                             int rank, int node0, void* workspace, size_t workspace_bytes, double* exchange, int* flags,
                             void* stream) {
    return shard_upsweep_gated(Hd, Ho, rhs, damping, nullptr, N, seg_len, world, rank, node0, workspace, workspace_bytes, exchange, true, flags,
                               Gate{nullptr, 0.0}, as_stream(stream));
}

int islam_pvgo_shard_downsweep(const double* exchange, int N, const int seg_len[2], int world, int rank, int node0, void* workspace,
                               size_t workspace_bytes, double* dx, int* flags, void* stream) {
    return shard_downsweep_gated(exchange, N, seg_len, world, rank, node0, workspace, workspace_bytes, dx, flags, Gate{nullptr, 0.0},
                                 as_stream(stream));
}

// Trial step on M links (nodes/vels/dx hold M+1 rows): writes nodes_t/vels_t (M+1 rows) and part (2 per 64-link block:
// sum r^2 at the trial point, sum JD.(2R+JD)).  Same kernel islam_pvgo_run_chain launches.
int islam_pvgo_trial(const double* nodes, const double* vels, const double* dx, const double* poses, const double* drots,
                     const double* dtrans, const double* dvels, const double* dts, const double* lin, int M, double* nodes_t,
                     double* vels_t, double* part, void* stream) {
    return trial_gated(nodes, vels, dx, poses, drots, dtrans, dvels, dts, lin, M, M, nodes_t, vels_t, part, nullptr, nullptr, nullptr, 0,
                       Gate{nullptr, 0.0}, as_stream(stream));
}

int islam_pvgo_retract(const double* nodes, const double* vels, const double* dx, double sign, int N, double* nodes_out,
                       double* vels_out, void* stream) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_retract: N=%d < 1", N);
    hipLaunchKernelGGL(retract_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), nodes, vels, dx, sign, N,
                       nodes_out, vels_out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_linearize_edges(const double* nodes, const int64_t* edges, const double* poses, int E, double* out,
                               void* stream) {
    if (E < 1) return fail(ISLAM_EARG, "islam_pvgo_linearize_edges: E=%d < 1", E);
    hipLaunchKernelGGL(vo_edge_linearize_kernel, dim3((E + 63) / 64), dim3(64), 0, as_stream(stream), nodes, edges, poses, E, out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_assemble_dense(const double* Hd, const double* Ho, const double* rhs_chain, const double* vo,
                              const int64_t* edges, const int64_t* node_ptr, const int64_t* node_adj, double w0, int N, int E,
                              double* A, double* rhs, void* stream) {
    return assemble_dense_entry("islam_pvgo_assemble_dense", EW_PLAIN, Hd, Ho, rhs_chain, vo, nullptr, nullptr, edges, node_ptr, node_adj, w0, N, E, A, rhs, stream);
}

int islam_pvgo_assemble_dense_scaled(const double* Hd, const double* Ho, const double* rhs_chain, const double* vo,
                                     const double* c_vo, const int64_t* edges, const int64_t* node_ptr,
                                     const int64_t* node_adj, double w0, int N, int E, double* A, double* rhs, void* stream) {
    return assemble_dense_entry("islam_pvgo_assemble_dense_scaled", EW_SCALED, Hd, Ho, rhs_chain, vo, c_vo, nullptr, edges, node_ptr, node_adj, w0, N, E, A, rhs, stream);
}

int islam_pvgo_assemble_dense_info(const double* Hd, const double* Ho, const double* rhs_chain, const double* vo, const double* info_vo,
                                   const int64_t* edges, const int64_t* node_ptr, const int64_t* node_adj, int N, int E, double* A,
                                   double* rhs, void* stream) {
    return assemble_dense_entry("islam_pvgo_assemble_dense_info", EW_INFO, Hd, Ho, rhs_chain, vo, nullptr, info_vo, edges, node_ptr, node_adj, 0.0, N, E, A, rhs, stream);
}

int islam_pvgo_band_assemble(double* Hd, double* Ho, double* rhs, const double* vo, const double* c_vo, const double* info_vo,
                             const int64_t* edges, const int64_t* node_ptr, const int64_t* node_adj, double w0, int N, int E,
                             const int64_t* off_idx, int K, int64_t* io, int64_t* jo, double* So, void* stream) {
    if (N < 2 || E < 1 || K < 0 || K > E || !Hd || !Ho || !rhs || !vo || !edges || !node_ptr || !node_adj || (c_vo && info_vo) ||
        (K > 0 && (!off_idx || !io || !jo || !So)))
        return fail(ISLAM_EARG, "islam_pvgo_band_assemble: N=%d E=%d K=%d, a null array, or both c_vo and info_vo", N, E, K);
    const dim3 grid((std::max(N, K) + 63) / 64), block(64);
    hipStream_t s = as_stream(stream);
    const auto kernel = info_vo ? band_assemble_kernel<EW_INFO> : c_vo ? band_assemble_kernel<EW_SCALED> : band_assemble_kernel<EW_PLAIN>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, Hd, Ho, rhs, vo, c_vo, info_vo, edges, node_ptr, node_adj, w0, N, E, off_idx, K, io, jo, So);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_band_matvec(const double* Hd, const double* Ho, const double* p, const int64_t* off_ptr, const int64_t* off_adj,
                           const int64_t* io, const int64_t* jo, const double* So, int N, int K, double* y, void* stream) {
    if (N < 2 || N > 200000000 /* 9 N + 255 fits an int */ || K < 0 || !Hd || !Ho || !p || !y || p == y || (K > 0 && (!off_ptr || !off_adj || !io || !jo || !So)))
        return fail(ISLAM_EARG, "islam_pvgo_band_matvec: N=%d K=%d, a null array, or y aliasing p", N, K);
    hipLaunchKernelGGL(band_matvec_kernel, dim3((9 * N + 255) / 256), dim3(256), 0, as_stream(stream), Hd, Ho, p, off_ptr, off_adj, io, jo,
                       So, N, K, y);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_robust_weights(const double* vo, int E, const double* lin, int M, const islam_pvgo_robust* robust, double* c_vo,
                              double* c_imu, double* rho_part, void* stream) {
    if (E < 0 || M < 0 || E + M < 1 || !robust || !rho_part || (E > 0 && !vo) || (M > 0 && !lin))
        return fail(ISLAM_EARG, "islam_pvgo_robust_weights: E=%d M=%d or a null input", E, M);
    RobustDev rb{};
    const int rc = robust_dev(robust, rb);
    if (rc != ISLAM_OK) return rc;
    const int n = std::max(E, M);
    hipLaunchKernelGGL(robust_weights_kernel, dim3((n + 63) / 64), dim3(64), 0, as_stream(stream), vo, E, lin, M, rb, c_vo, c_imu,
                       rho_part);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_vo_loss_fwd(const double* nodes, const int64_t* edges, const double* poses, int E, double* err6,
                           double* trans_loss, double* rot_loss, void* stream) {
    if (E < 1) return fail(ISLAM_EARG, "islam_pvgo_vo_loss_fwd: E=%d < 1", E);
    hipLaunchKernelGGL(vo_loss_fwd_kernel, dim3((E + 63) / 64), dim3(64), 0, as_stream(stream), nodes, edges, poses, E,
                       err6, trans_loss, rot_loss);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_vo_loss_bwd(const double* poses, const double* err6, const double* g_trans, const double* g_rot, int E,
                           double* grad_poses, void* stream) {
    if (E < 1) return fail(ISLAM_EARG, "islam_pvgo_vo_loss_bwd: E=%d < 1", E);
    hipLaunchKernelGGL(vo_loss_bwd_kernel, dim3((E + 63) / 64), dim3(64), 0, as_stream(stream), poses, err6, g_trans,
                       g_rot, E, grad_poses);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_align(const double* nodes, const double* vels, const double* target7, int N, double* nodes_out,
                     double* vels_out, void* stream) {
    if (N < 1) return fail(ISLAM_EARG, "islam_pvgo_align: N=%d < 1", N);
    hipLaunchKernelGGL(align_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), nodes, vels, target7, N,
                       nodes_out, vels_out);
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_reproj_reduce(const double* nodes, const double* dx, int N, const islam_pvgo_reproj* reproj, double* red,
                             void* stream) {
    if (N < 2 || !reproj) return fail(ISLAM_EARG, "islam_pvgo_reproj_reduce: N=%d < 2 or null reproj", N);
    ReprojDev rp{};
    int rc = reproj_dev(reproj, rp);
    if (rc != ISLAM_OK) return rc;
    enqueue_reproj_reduce(nodes, dx, N - 1, rp, red, as_stream(stream));
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

int islam_pvgo_run_chain(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                         const double* dvels, const double* dts, int N, const islam_pvgo_params* prm, void* workspace,
                         size_t workspace_bytes, islam_pvgo_result* result, double* trace, int trace_cap, void* stream) {
    return run_chain_entry(nodes, vels, poses, drots, dtrans, dvels, dts, N, prm, nullptr, nullptr, workspace, workspace_bytes, result,
                           trace, trace_cap, stream);
}

int islam_pvgo_run_chain_reproj(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                                const double* dvels, const double* dts, int N, const islam_pvgo_params* prm,
                                const islam_pvgo_reproj* reproj, void* workspace, size_t workspace_bytes,
                                islam_pvgo_result* result, double* trace, int trace_cap, void* stream) {
    return run_chain_entry(nodes, vels, poses, drots, dtrans, dvels, dts, N, prm, reproj, nullptr, workspace, workspace_bytes, result,
                           trace, trace_cap, stream);
}

// robust kernels: the launch-per-stage loop with linbuild_robust_kernel / trial_lin_robust_kernel
int islam_pvgo_run_chain_robust(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                                const double* dvels, const double* dts, int N, const islam_pvgo_params* prm,
                                const islam_pvgo_robust* robust, void* workspace, size_t workspace_bytes,
                                islam_pvgo_result* result, double* trace, int trace_cap, void* stream) {
    return run_chain_entry(nodes, vels, poses, drots, dtrans, dvels, dts, N, prm, nullptr, robust, workspace, workspace_bytes, result,
                           trace, trace_cap, stream);
}

// per-factor information matrices: the launch-per-stage loop with info_build_kernel behind every linearisation
int islam_pvgo_run_chain_info(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                              const double* dvels, const double* dts, int N, const islam_pvgo_params* prm, const double* info_vo,
                              const double* info_imu, void* workspace, size_t workspace_bytes, islam_pvgo_result* result, double* trace,
                              int trace_cap, void* stream) {
    return run_chain_entry(nodes, vels, poses, drots, dtrans, dvels, dts, N, prm, nullptr, nullptr, workspace, workspace_bytes, result,
                           trace, trace_cap, stream, info_vo, info_imu);
}

// the same loop with one correlated 9x9 per link: info9_build_kernel behind every linearisation
int islam_pvgo_run_chain_info9(double* nodes, double* vels, const double* poses, const double* drots, const double* dtrans,
                               const double* dvels, const double* dts, int N, const islam_pvgo_params* prm, const double* info_vo,
                               const double* info_imu9, void* workspace, size_t workspace_bytes, islam_pvgo_result* result, double* trace,
                               int trace_cap, void* stream) {
    return run_chain_entry(nodes, vels, poses, drots, dtrans, dvels, dts, N, prm, nullptr, nullptr, workspace, workspace_bytes, result,
                           trace, trace_cap, stream, info_vo, info_imu9, true);
}

// Measurement hook (bench.py's roofline leg): the LM loop's dominant launch, trial_elim_kernel, exactly as islam_pvgo_run_chain
// launches it in its steady state -- after one linearisation and one damped solve of the given problem (so that `dx` and the old
// linearisation are real), `launches` back-to-back launches between ONE pair of HIP events on `stream`; *us_per_launch = their
// average period.  info[0..2] = (level-0 segment length, segments, workgroups).  ISLAM_EARG when the fused loop does not apply
// to this problem size (islam_pvgo_run_chain then runs the launch-per-stage loop).
int islam_pvgo_trial_elim_burst(const double* nodes, const double* vels, const double* poses, const double* drots, const double* dtrans,
                                const double* dvels, const double* dts, int N, const islam_pvgo_params* prm, void* workspace,
                                size_t workspace_bytes, int launches, float* us_per_launch, int* info, void* stream) {
    if (N < 2 || !prm || !us_per_launch || launches < 1) return fail(ISLAM_EARG, "islam_pvgo_trial_elim_burst: bad argument");
    Workspace w;
    int rc = workspace_or_fail("islam_pvgo_trial_elim_burst: workspace too small", N, workspace, workspace_bytes, w);
    if (rc != ISLAM_OK) return rc;
    SolvePlan sp;
    plan_levels(N, prm->seg_len, sp, solve_twisted());
    // (unlike run_chain_impl: always 16 spare CUs, whatever ISLAM_FZ_SPARE says, and no lower bound on N -- the hook measures the
    // launch wherever the kernel can run)
    const int fz_nwg = std::min(sp.lv[0].P, std::max(device_cus() - 16, 1));
    if (!(sp.nl >= 2 && fused_plan_core(sp, sp.lv[0].P, fz_nwg)))
        return fail(ISLAM_EARG, "islam_pvgo_trial_elim_burst: the fused loop does not cover N=%d", N);
    hipStream_t s = as_stream(stream);
    if ((rc = ensure_linbuild_lds()) != ISLAM_OK) return rc;
    if ((rc = ensure_fused_lds()) != ISLAM_OK) return rc;
    // (the kernel only reads the current iterate; no verdict block: nobody waits for these trials)
    ChainRun r = chain_run(const_cast<double*>(nodes), const_cast<double*>(vels), ChainData{poses, drots, dtrans, dvels, dts, N}, prm, w, s);
    r.fz_m = sp.lv[0].m; r.fz_P = sp.lv[0].P; r.fz_nwg = fz_nwg;
    ISLAM_HIP_CHECK(hipMemsetAsync(w.ready, 0, w.ready_bytes, s));
    hipLaunchKernelGGL(control_init_kernel, dim3(1), dim3(64), 0, s, w.state, w.flags, prm->radius, prm->down, (uint4*)nullptr, 0u);
    enqueue_linbuild(r, nodes, vels, 0, false);
    hipLaunchKernelGGL(control_begin_kernel, dim3(1), dim3(64), 0, s, w.loss_part, r.nlb, w.state, w.flags);
    LevelSrc src{};
    src.level0 = 1; src.Hd = w.Hd; src.Ho = w.Ho; src.rhs0 = w.rhs; src.state = w.state; src.hist = 1;
    rc = enqueue_levels(w, sp, 0, src, nullptr, w.dx, w.flags, s, nullptr, nullptr);
    if (rc != ISLAM_OK) return rc;
    const IterCfg c{0, r.nodes, r.vels, w.nodes_t, w.vels_t};
    const FusedArgs fa = fused_args(r, c, FUSED_TRIAL_ELIM, 1.0, r.eflag_none());
    const Gate open{nullptr, 0.0};
    for (int i = 0; i < 3; ++i) launch_fused(r, fa, open);
    hipEvent_t e0, e1;
    ISLAM_HIP_CHECK(hipEventCreate(&e0));
    ISLAM_HIP_CHECK(hipEventCreate(&e1));
    ISLAM_HIP_CHECK(hipStreamSynchronize(s));
    ISLAM_HIP_CHECK(hipEventRecord(e0, s));
    for (int i = 0; i < launches; ++i) launch_fused(r, fa, open);
    ISLAM_HIP_CHECK(hipEventRecord(e1, s));
    ISLAM_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0.f;
    ISLAM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *us_per_launch = ms * 1e3f / (float)launches;
    if (info) { info[0] = fa.m; info[1] = fa.P; info[2] = fa.nwg; }
    ISLAM_LAUNCH_CHECK();
    return ISLAM_OK;
}

}  // extern "C"

#include "pvgo_marginals.inl"   // marginal covariances: partitioned selected inversion
#include "pvgo_band_cov.inl"   // marginal covariances of loop-closure graphs: Woodbury correction on the band form
