// pvgo_general.inl -- part of the pvgo.hip translation unit (textually included there; not compiled on its own).
// control kernels, retraction, arbitrary-topology assembly, vo_loss / imu_loss forward + backward, align_to (reference pvgo.py:67-119)
// state <- [damping = 1 / radius, radius, down, run-ahead epoch 1], everything else and the four flag words zero
// ready16 != nullptr: the down-sweep's ready words are zeroed by the same launch (n16 16-byte items over the whole grid) -- the separate
// fill launch in front of every run_pvgo cost ~2.5 us of the run
__global__ __launch_bounds__(256) void control_init_kernel(double* __restrict__ st, int* __restrict__ flags, double radius, double down,
                                                           uint4* __restrict__ ready16 = nullptr, unsigned n16 = 0) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        if (t < STATE_DOUBLES) st[t] = (t == 2 || t == STATE_HIST) ? 1.0 / radius : t == 3 ? radius : t == 4 ? down : (t == 14 || t == 15) ? 1.0 : 0.0;     // [15]: first guess "radius kept"
        if (t < 8) flags[t] = 0;
    }
    for (unsigned i = blockIdx.x * 256u + t; i < n16; i += gridDim.x * 256u) ready16[i] = uint4{0u, 0u, 0u, 0u};
}

__global__ __launch_bounds__(64) void control_begin_kernel(const double* __restrict__ loss_part, int nblk,
                                                            double* __restrict__ st, int* flags) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) s += loss_part[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) {
        st[0] = s;                                         // self.loss of the very first optimizer.step()
        st[1] = s;                                         // self.last = self.loss
        st[8] = 0.0;
        st[11] = 1.0;
        st[12] = 0.0;
        st[13] = 0.0;
        flags[0] = 0;
    }
}

__global__ __launch_bounds__(64) void retract_kernel(const double* __restrict__ nodes, const double* __restrict__ vels,
                                                      const double* __restrict__ dx, double sign, int N,
                                                      double* __restrict__ nodes_o, double* __restrict__ vels_o) {
    int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= N) return;
    const double* d = dx + (size_t)k * 9;
    SE3<double> X = se3_mul(se3_exp(sign * ld3(d), sign * ld3(d + 3)), se3_load(nodes + 7 * k));
    se3_store(X, nodes_o + 7 * k);
    V3<double> v = ld3(vels + 3 * k) + sign * ld3(d + 6);
    vels_o[3 * k] = v.x; vels_o[3 * k + 1] = v.y; vels_o[3 * k + 2] = v.z;
}

// VO factor of an ARBITRARY edge (i, j) (loop closures; pvgo.py:36-39): residual e = Log(P^-1 Xi^-1 Xj) and the blocks
// G, C of d e / d delta_j = [[G, C],[0, G]] (d e / d delta_i = -that).  out: (24, E) component-major.
__global__ __launch_bounds__(64) void vo_edge_linearize_kernel(const double* __restrict__ nodes, const int64_t* __restrict__ edges,
                                                                const double* __restrict__ poses, int E, double* __restrict__ out) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    SE3<double> Xi = se3_load(nodes + 7 * edges[2 * e]), Xj = se3_load(nodes + 7 * edges[2 * e + 1]);
    SE3<double> pre;
    V3<double> rho, phi;
    M3<double> G, C;
    vo_link(Xi, Xj, se3_load(poses + 7 * e), pre, rho, phi, G, C);
    double rec[24];
    rec[0] = rho.x; rec[1] = rho.y; rec[2] = rho.z; rec[3] = phi.x; rec[4] = phi.y; rec[5] = phi.z;
    m3_store(G, rec + 6);
    m3_store(C, rec + 15);
#pragma unroll
    for (int c = 0; c < 24; ++c) out[(size_t)c * E + e] = rec[c];
}

// ---- general topology: the normal pieces S = A_e^T W A_e, g = A_e^T W e of one VO edge, the ONE place that weights an edge; the
// dense and the band assembly below both sum what edge_pieces returns ----
enum EdgeWeight { EW_PLAIN, EW_SCALED, EW_INFO };   // w0 | w0 c_vo[e] (robust multiplier) | Omega0_e of info_vo (21,E)

__device__ __forceinline__ PoseNormal edge_normal(const double* __restrict__ vo, int E, int e) {      // unweighted
    double rec[24];
#pragma unroll
    for (int c = 0; c < 24; ++c) rec[c] = vo[(size_t)c * E + e];
    const V3<double> er{rec[0], rec[1], rec[2]}, ep{rec[3], rec[4], rec[5]};
    const M3<double> G = m3_load(rec + 6), C = m3_load(rec + 15);
    const M3<double> Gt = transpose(G), Ct = transpose(C);
    PoseNormal o;
    o.Srr = Gt * G;
    o.Srp = Gt * C;
    o.Spp = Ct * C + o.Srr;
    o.gr = Gt * er;
    o.gp = Ct * er + Gt * ep;
    return o;
}

template <EdgeWeight MODE>
__device__ __forceinline__ PoseNormal edge_pieces(const double* __restrict__ vo, const double* __restrict__ c_vo,
                                                  const double* __restrict__ info_vo, double w0, int E, int e) {
    if constexpr (MODE == EW_INFO) {
        const double* r = vo + e;
        const size_t ld = (size_t)E;
        return info_vo_normal(info_vo + e, ld, lin_m3(r, ld, 6), lin_m3(r, ld, 15), lin_v3(r, ld, 0), lin_v3(r, ld, 3));
    } else {
        const PoseNormal en = edge_normal(vo, E, e);
        double we = w0;
        if constexpr (MODE == EW_SCALED) we = w0 * c_vo[e];
        PoseNormal o;
        o.Srr = we * en.Srr; o.Srp = we * en.Srp; o.Spp = we * en.Spp; o.gr = we * en.gr; o.gp = we * en.gp;
        return o;
    }
}

// Robust multipliers of a general-topology linearisation (islam_pvgo_robust_weights): lane k takes VO edge k (rows 0-5 of vo)
// and link k (velocity rows 36-38, rotation 24-26, translation-velocity 39-41 of lin); one partial sum of rho per workgroup
__global__ __launch_bounds__(64) void robust_weights_kernel(const double* __restrict__ vo, int E, const double* __restrict__ lin, int M,
                                                             RobustDev rb, double* __restrict__ c_vo, double* __restrict__ c_imu,
                                                             double* __restrict__ rho_part) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    double l = 0.0, c;
    if (k < E) {
        const V3<double> er = lin_v3(vo + k, E, 0), ep = lin_v3(vo + k, E, 3);
        l += robust_rho(rb.kind[0], rb.delta[0], dot(er, er) + dot(ep, ep), c);
        if (c_vo) c_vo[k] = c;
    }
    if (k < M) {
        const int rows[3] = {36, 24, 39};
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const V3<double> r = lin_v3(lin + k, M, rows[g]);
            l += robust_rho(rb.kind[g + 1], rb.delta[g + 1], dot(r, r), c);
            if (c_imu) c_imu[(size_t)g * M + k] = c;
        }
    }
    l = wave_sum(l);
    if (threadIdx.x == 0) rho_part[blockIdx.x] = l;
}

// add a 3x3 block into a row-major matrix of leading dimension ld (fixed indices: the operands stay in registers)
__device__ __forceinline__ void add3x3(double* p, size_t ld, M3<double> a) {
    p[0] += a.a00; p[1] += a.a01; p[2] += a.a02;
    p[ld] += a.a10; p[ld + 1] += a.a11; p[ld + 2] += a.a12;
    p[2 * ld] += a.a20; p[2 * ld + 1] += a.a21; p[2 * ld + 2] += a.a22;
}
// p (row-major, leading dimension ld) -= [[Srr, Srp], [Srp^T, Spp]] (sign = -1) or += (sign = +1)
__device__ __forceinline__ void add6x6(double* p, size_t ld, double sign, M3<double> Srr, M3<double> Srp, M3<double> Spp) {
    add3x3(p, ld, sign * Srr); add3x3(p + 3, ld, sign * Srp); add3x3(p + 3 * ld, ld, sign * transpose(Srp)); add3x3(p + 3 * ld + 3, ld, sign * Spp);
}
// block (i, j) -= a, block (j, i) -= a^T, atomically
__device__ __forceinline__ void sub3x3_atomic(double* ij, double* ji, size_t ld, M3<double> a) {
    atomicAdd(&ij[0], -a.a00); atomicAdd(&ij[1], -a.a01); atomicAdd(&ij[2], -a.a02);
    atomicAdd(&ij[ld], -a.a10); atomicAdd(&ij[ld + 1], -a.a11); atomicAdd(&ij[ld + 2], -a.a12);
    atomicAdd(&ij[2 * ld], -a.a20); atomicAdd(&ij[2 * ld + 1], -a.a21); atomicAdd(&ij[2 * ld + 2], -a.a22);
    atomicAdd(&ji[0], -a.a00); atomicAdd(&ji[ld], -a.a01); atomicAdd(&ji[2 * ld], -a.a02);
    atomicAdd(&ji[1], -a.a10); atomicAdd(&ji[ld + 1], -a.a11); atomicAdd(&ji[2 * ld + 1], -a.a12);
    atomicAdd(&ji[2], -a.a20); atomicAdd(&ji[ld + 2], -a.a21); atomicAdd(&ji[2 * ld + 2], -a.a22);
}

// ---- dense A (9N x 9N, zeroed by the caller) from block pieces, no dense J (islam_pvgo_assemble_dense / _scaled / _info) ----
// one lane per node: diagonal block + right-hand side (fixed summation order: the node's edge ends in CSR order), both triangles of
// the chain coupling
template <EdgeWeight MODE>
__global__ __launch_bounds__(64) void dense_nodes_kernel(const double* __restrict__ Hd, const double* __restrict__ Ho,
                                                          const double* __restrict__ rhs_chain, const double* __restrict__ vo,
                                                          const double* __restrict__ c_vo, const double* __restrict__ info_vo,
                                                          const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ node_adj,
                                                          double w0, int N, int E, double* __restrict__ A, double* __restrict__ rhs) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= N) return;
    const size_t ld = (size_t)9 * N;
    const M3<double> Z{0, 0, 0, 0, 0, 0, 0, 0, 0};
    M3<double> Srr = Z, Srp = Z, Spp = Z;
    V3<double> gr{0, 0, 0}, gp{0, 0, 0};
    for (int64_t a = node_ptr[k]; a < node_ptr[k + 1]; ++a) {
        const int64_t code = node_adj[a];
        const PoseNormal en = edge_pieces<MODE>(vo, c_vo, info_vo, w0, E, (int)(code >> 1));
        Srr = Srr + en.Srr; Srp = Srp + en.Srp; Spp = Spp + en.Spp;
        if (code & 1) { gr = gr + en.gr; gp = gp + en.gp; } else { gr = gr - en.gr; gp = gp - en.gp; }
    }
    double* d = A + (size_t)9 * k * ld + 9 * k;
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
        for (int c = 0; c < 9; ++c) d[r * ld + c] = Hd[(size_t)k * 81 + r * 9 + c];
    add6x6(d, ld, 1.0, Srr, Srp, Spp);
    const double* rc = rhs_chain + (size_t)k * 9;
    double* b = rhs + (size_t)k * 9;
    b[0] = rc[0] - gr.x; b[1] = rc[1] - gr.y; b[2] = rc[2] - gr.z;
    b[3] = rc[3] - gp.x; b[4] = rc[4] - gp.y; b[5] = rc[5] - gp.z;
    b[6] = rc[6]; b[7] = rc[7]; b[8] = rc[8];
    if (k < N - 1) {
        double* up = A + (size_t)9 * k * ld + 9 * (k + 1);
        double* lo = A + (size_t)9 * (k + 1) * ld + 9 * k;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double v = Ho[(size_t)k * 81 + r * 9 + c];
                up[r * ld + c] = v;
                lo[c * ld + r] = v;
            }
    }
}

// one lane per edge: block (i, j) -= S, block (j, i) -= S^T of an arbitrary edge (i, j); atomics, because parallel edges share a node pair
template <EdgeWeight MODE>
__global__ __launch_bounds__(64) void dense_edges_kernel(const double* __restrict__ vo, const double* __restrict__ c_vo,
                                                          const double* __restrict__ info_vo, const int64_t* __restrict__ edges,
                                                          double w0, int N, int E, double* __restrict__ A) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const int64_t i = edges[2 * e], j = edges[2 * e + 1];
    if (i == j) return;
    const PoseNormal en = edge_pieces<MODE>(vo, c_vo, info_vo, w0, E, e);
    const size_t ld = (size_t)9 * N;
    double* ij = A + (size_t)9 * i * ld + 9 * j;
    double* ji = A + (size_t)9 * j * ld + 9 * i;
    sub3x3_atomic(ij, ji, ld, en.Srr);
    sub3x3_atomic(ij + 3, ji + 3 * ld, ld, en.Srp);
    sub3x3_atomic(ij + 3 * ld, ji + 3, ld, transpose(en.Srp));
    sub3x3_atomic(ij + 3 * ld + 3, ji + 3 * ld + 3, ld, en.Spp);
}

// ---- band + off-band form of the same normal equations (islam_pvgo_band_assemble / _matvec) ----
// a 3x3 block of a row-major 6x6 matrix
__device__ __forceinline__ void store3x3_ld6(M3<double> a, double* p) {
    p[0] = a.a00; p[1] = a.a01; p[2] = a.a02; p[6] = a.a10; p[7] = a.a11; p[8] = a.a12; p[12] = a.a20; p[13] = a.a21; p[14] = a.a22;
}

// Lane t < N, node t: walks the node's edge ends in CSR order (the order of dense_nodes_kernel) and adds, in place, every edge's S
// to the pose block of Hd[t], its gradient to rhs[t] (-g at the edge's first node, +g at its second; rhs = -J^T W r) and -S to Ho[t]
// for every edge whose other end is node t + 1, whichever way it points (S is symmetric): all of Ho[t] comes from this one lane, so
// parallel edges accumulate in a fixed order and no atomic is needed.  Lane t < K, off-band edge off_idx[t]: its ends and its S.
template <EdgeWeight MODE>
__global__ __launch_bounds__(64) void band_assemble_kernel(double* __restrict__ Hd, double* __restrict__ Ho, double* __restrict__ rhs,
                                                            const double* __restrict__ vo, const double* __restrict__ c_vo,
                                                            const double* __restrict__ info_vo, const int64_t* __restrict__ edges,
                                                            const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ node_adj,
                                                            double w0, int N, int E, const int64_t* __restrict__ off_idx, int K,
                                                            int64_t* __restrict__ io, int64_t* __restrict__ jo, double* __restrict__ So) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    const M3<double> Z{0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (t < N) {
        M3<double> Srr = Z, Srp = Z, Spp = Z, Orr = Z, Orp = Z, Opp = Z;
        V3<double> gr{0, 0, 0}, gp{0, 0, 0};
        for (int64_t a = node_ptr[t]; a < node_ptr[t + 1]; ++a) {
            const int64_t code = node_adj[a];
            const int e = (int)(code >> 1);
            const PoseNormal en = edge_pieces<MODE>(vo, c_vo, info_vo, w0, E, e);
            Srr = Srr + en.Srr; Srp = Srp + en.Srp; Spp = Spp + en.Spp;
            if (code & 1) { gr = gr + en.gr; gp = gp + en.gp; } else { gr = gr - en.gr; gp = gp - en.gp; }
            if (edges[2 * e + 1 - (int)(code & 1)] == (int64_t)t + 1) { Orr = Orr + en.Srr; Orp = Orp + en.Srp; Opp = Opp + en.Spp; }
        }
        add6x6(Hd + (size_t)t * 81, 9, 1.0, Srr, Srp, Spp);
        if (t < N - 1) add6x6(Ho + (size_t)t * 81, 9, -1.0, Orr, Orp, Opp);
        double* b = rhs + (size_t)t * 9;
        b[0] -= gr.x; b[1] -= gr.y; b[2] -= gr.z; b[3] -= gp.x; b[4] -= gp.y; b[5] -= gp.z;
    }
    if (t < K) {
        const int e = (int)off_idx[t];
        io[t] = edges[2 * e];
        jo[t] = edges[2 * e + 1];
        const PoseNormal en = edge_pieces<MODE>(vo, c_vo, info_vo, w0, E, e);
        double* s = So + (size_t)t * 36;
        store3x3_ld6(en.Srr, s); store3x3_ld6(en.Srp, s + 3); store3x3_ld6(transpose(en.Srp), s + 18); store3x3_ld6(en.Spp, s + 21);
    }
}

// y = A p of the band + off-band form, one launch, nine lanes per node: lane (k, r) forms row r of node k,
//   y[k][r] = Hd[k][r][:] . p[k] + Ho[k][r][:] . p[k+1] + Ho[k-1][:][r] . p[k-1] - sum over the node's off-band edge ends So[t][r][:] . p[other end]
// (r < 6 for the last term).  The nine lanes of a node read the 81 doubles of a block between them, so a wavefront's loads cover one
// contiguous stretch of Hd and of Ho; Ho[k] is read by nodes k and k + 1, neighbours in the same wavefront but for one node in seven.
// off_ptr (N+1), off_adj: CSR of the off-band edge ends per node, entry = 2 * t + end: a fixed order, no atomics.
__global__ __launch_bounds__(256) void band_matvec_kernel(const double* __restrict__ Hd, const double* __restrict__ Ho,
                                                           const double* __restrict__ p, const int64_t* __restrict__ off_ptr,
                                                           const int64_t* __restrict__ off_adj, const int64_t* __restrict__ io,
                                                           const int64_t* __restrict__ jo, const double* __restrict__ So, int N, int K,
                                                           double* __restrict__ y) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int k = t / 9, r = t - 9 * k;
    if (k >= N) return;
    const double* pk = p + (size_t)k * 9;
    const double* hd = Hd + (size_t)k * 81 + r * 9;
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) acc += hd[c] * pk[c];
    if (k < N - 1) {
        const double* ho = Ho + (size_t)k * 81 + r * 9;
#pragma unroll
        for (int c = 0; c < 9; ++c) acc += ho[c] * pk[9 + c];
    }
    if (k > 0) {
        const double* ho = Ho + (size_t)(k - 1) * 81 + r;
#pragma unroll
        for (int c = 0; c < 9; ++c) acc += ho[c * 9] * pk[c - 9];
    }
    if (K > 0 && r < 6) {
        double off = 0.0;
        for (int64_t a = off_ptr[k]; a < off_ptr[k + 1]; ++a) {
            const int64_t code = off_adj[a];
            const int64_t te = code >> 1;
            const double* po = p + (size_t)((code & 1) ? io[te] : jo[te]) * 9;
            const double* s = So + (size_t)te * 36 + r * 6;
#pragma unroll
            for (int c = 0; c < 6; ++c) off += s[c] * po[c];
        }
        acc -= off;
    }
    y[t] = acc;
}

__global__ __launch_bounds__(64) void vo_loss_fwd_kernel(const double* __restrict__ nodes, const int64_t* __restrict__ edges,
                                                          const double* __restrict__ poses, int E, double* __restrict__ err6,
                                                          double* __restrict__ tl, double* __restrict__ rl) {
    int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    SE3<double> Xi = se3_load(nodes + 7 * edges[2 * e]), Xj = se3_load(nodes + 7 * edges[2 * e + 1]);
    SE3<double> P = se3_load(poses + 7 * e);
    V3<double> rho, phi;
    se3_log(se3_mul(se3_mul(se3_inv(P), se3_inv(Xi)), Xj), rho, phi);
    double* o = err6 + 6 * (size_t)e;
    o[0] = rho.x; o[1] = rho.y; o[2] = rho.z; o[3] = phi.x; o[4] = phi.y; o[5] = phi.z;
    tl[e] = dot(rho, rho);
    rl[e] = dot(phi, phi);
}

// PyPose autograd: g_E = g_e Jl^-1(e) ; g_P = -g_E Ad(P^-1), stored as a 7-vector with a trailing 0
__global__ __launch_bounds__(64) void vo_loss_bwd_kernel(const double* __restrict__ poses, const double* __restrict__ err6,
                                                          const double* __restrict__ g_trans, const double* __restrict__ g_rot,
                                                          int E, double* __restrict__ grad) {
    int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const double* er = err6 + 6 * (size_t)e;
    V3<double> rho = ld3(er), phi = ld3(er + 3);
    V3<double> gr = (2.0 * g_trans[e]) * rho, gp = (2.0 * g_rot[e]) * phi;
    M3<double> Ji = so3_Jl_inv(phi);
    M3<double> Q = se3_Q(rho, phi);
    // row-vector times Jl^-1 = [[Ji, -Ji Q Ji],[0, Ji]]
    V3<double> a = tmul(Ji, gr);
    V3<double> b = tmul(Ji, gp) - tmul(Ji, tmul(Q, a));
    SE3<double> Pi = se3_inv(se3_load(poses + 7 * e));
    M3<double> R = qmat(Pi.q);
    // row-vector times Ad(Pi) = [[R, [t]x R],[0, R]]
    V3<double> o0 = tmul(R, a);
    V3<double> o1 = tmul(R, tmul(skew(Pi.t), a)) + tmul(R, b);
    double* g = grad + 7 * (size_t)e;
    g[0] = -o0.x; g[1] = -o0.y; g[2] = -o0.z; g[3] = -o1.x; g[4] = -o1.y; g[5] = -o1.z; g[6] = 0.0;
}

__global__ __launch_bounds__(64) void align_kernel(const double* __restrict__ nodes, const double* __restrict__ vels,
                                                    const double* __restrict__ target, int N, double* __restrict__ nodes_o,
                                                    double* __restrict__ vels_o) {
    int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= N) return;
    SE3<double> T = se3_load(target), S = se3_load(nodes);
    SE3<double> rel = se3_mul(T, se3_inv(S));
    Q4<double> rq = qmul(T.q, qinv(S.q));
    se3_store(se3_mul(rel, se3_load(nodes + 7 * k)), nodes_o + 7 * k);
    V3<double> v = qact(rq, ld3(vels + 3 * k));
    vels_o[3 * k] = v.x; vels_o[3 * k + 1] = v.y; vels_o[3 * k + 2] = v.z;
}

