// pvgo_linearize.inl -- part of the pvgo.hip translation unit (textually included there; not compiled on its own).
// link residuals, Jacobian blocks, normal equations, the sparse reprojection factor, linbuild_kernel (reference pvgo.py:26-64, dense_ba.py:276-305)
// ------------------------------------------------------------------------------------------
// residuals of one link (pvgo.py:36-51); also returns what the Jacobian needs
struct LinkRes {
    V3<double> erho, ephi, er, rv, rt;
    SE3<double> pre;      // P^-1 * Xi^-1
    Q4<double> rpre;      // dR^-1 * Ri^-1
    M3<double> Ji;        // Jl^-1(ephi), as se3_log formed it
};

// The pose-graph (VO) factor of one link or edge, stated ONCE for every kernel that linearises it (linearize_kernel, linbuild_kernel,
// trial_lin_kernel, small_lm_kernel, phase B of trial_elim_kernel, vo_edge_linearize_kernel): the same statements in the same order
// are what keeps their linearisations bit-identical.
// residual e = [erho, ephi] = Log(P^-1 Xi^-1 Xj), with pre = P^-1 Xi^-1 and Ji = Jl^-1(ephi)
__device__ __forceinline__ void vo_residual(SE3<double> Xi, SE3<double> Xj, SE3<double> P, SE3<double>& pre, V3<double>& erho,
                                            V3<double>& ephi, M3<double>& Ji) {
    pre = se3_mul(se3_inv(P), se3_inv(Xi));
    se3_log(se3_mul(pre, Xj), erho, ephi, Ji);
}
// d e / d delta_j = Jl^-1(e) Ad(pre) = [[G, C],[0, G]]:  G = Ji R,  C = Ji ([t]x R - Q G)   (d e / d delta_i = -that)
__device__ __forceinline__ void vo_jacobians(const SE3<double>& pre, V3<double> erho, V3<double> ephi, const M3<double>& Ji,
                                             M3<double>& G, M3<double>& C) {
    const M3<double> R = qmat(pre.q);
    G = Ji * R;
    C = Ji * (skew(pre.t) * R - se3_Q(erho, ephi) * G);
}
// both at once: (erho, ephi, G, C) of the link; pre is handed back for the callers that go on from it
__device__ __forceinline__ void vo_link(SE3<double> Xi, SE3<double> Xj, SE3<double> P, SE3<double>& pre, V3<double>& erho,
                                        V3<double>& ephi, M3<double>& G, M3<double>& C) {
    M3<double> Ji;
    vo_residual(Xi, Xj, P, pre, erho, ephi, Ji);
    vo_jacobians(pre, erho, ephi, Ji, G, C);
}

__device__ __forceinline__ LinkRes link_residuals(SE3<double> Xi, SE3<double> Xj, V3<double> vi, V3<double> vj,
                                                  SE3<double> P, Q4<double> dR, V3<double> dp, V3<double> dv,
                                                  double dt) {
    LinkRes o;
    vo_residual(Xi, Xj, P, o.pre, o.erho, o.ephi, o.Ji);
    o.rv = dv - (vj - vi);
    o.rpre = qmul(qinv(dR), qinv(Xi.q));
    o.er = so3_log(qmul(o.rpre, Xj.q));
    o.rt = (Xj.t - Xi.t) - (dt * vi + dp);
    return o;
}

__device__ __forceinline__ V3<double> ld3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ Q4<double> ld4(const double* p) { return {p[0], p[1], p[2], p[3]}; }
// components c.. of one record of a component-major array (`lin` (42,M), `vo` (24,E)): r = array + record index, ld = record count
__device__ __forceinline__ V3<double> lin_v3(const double* r, size_t ld, int c) {
    return {r[c * ld], r[(c + 1) * ld], r[(c + 2) * ld]};
}
__device__ __forceinline__ M3<double> lin_m3(const double* r, size_t ld, int c) {
    return {r[c * ld], r[(c + 1) * ld], r[(c + 2) * ld], r[(c + 3) * ld], r[(c + 4) * ld], r[(c + 5) * ld],
            r[(c + 6) * ld], r[(c + 7) * ld], r[(c + 8) * ld]};
}

// one lane per link: residuals + Jacobian blocks G, C (A = [[G, C],[0, G]]) and B
__global__ __launch_bounds__(64) void linearize_kernel(const double* __restrict__ nodes, const double* __restrict__ vels,
                                                        const double* __restrict__ poses, const double* __restrict__ drots,
                                                        const double* __restrict__ dtrans, const double* __restrict__ dvels,
                                                        const double* __restrict__ dts, int M, double* __restrict__ lin,
                                                        double* __restrict__ loss_part) {
    int k = blockIdx.x * 64 + threadIdx.x;
    double sq = 0.0;
    if (k < M) {
        SE3<double> Xi = se3_load(nodes + 7 * k), Xj = se3_load(nodes + 7 * (k + 1));
        LinkRes r = link_residuals(Xi, Xj, ld3(vels + 3 * k), ld3(vels + 3 * (k + 1)), se3_load(poses + 7 * k),
                                   ld4(drots + 4 * k), ld3(dtrans + 3 * k), ld3(dvels + 3 * k), dts[k]);
        // d pgerr / d delta_j = Jl^-1(e) Ad(pre) = [[Ji R, Ji([t]x R - Q Ji R)],[0, Ji R]]
        M3<double> G, C;
        vo_jacobians(r.pre, r.erho, r.ephi, r.Ji, G, C);
        M3<double> B = so3_Jl_inv(r.er) * qmat(r.rpre);
        double rec[LIN_C];
        rec[0] = r.erho.x; rec[1] = r.erho.y; rec[2] = r.erho.z;
        rec[3] = r.ephi.x; rec[4] = r.ephi.y; rec[5] = r.ephi.z;
        m3_store(G, rec + 6);
        m3_store(C, rec + 15);
        rec[24] = r.er.x; rec[25] = r.er.y; rec[26] = r.er.z;
        m3_store(B, rec + 27);
        rec[36] = r.rv.x; rec[37] = r.rv.y; rec[38] = r.rv.z;
        rec[39] = r.rt.x; rec[40] = r.rt.y; rec[41] = r.rt.z;
#pragma unroll
        for (int c = 0; c < LIN_C; ++c) lin[(size_t)c * M + k] = rec[c];
        sq = dot(r.erho, r.erho) + dot(r.ephi, r.ephi) + dot(r.rv, r.rv) + dot(r.er, r.er) + dot(r.rt, r.rt);
    }
    sq = wave_sum(sq);
    if (threadIdx.x == 0) loss_part[blockIdx.x] = sq;
}

struct LinkNormal {       // weighted per-link normal-equation pieces
    M3<double> Srr, Srp, Spp;   // pose-pose block S = [[Srr, Srp],[Srp^T, Spp]]
    V3<double> gr, gp;          // J_j^T W r, pose part
    V3<double> rv, rt;
};

__device__ __forceinline__ LinkNormal link_normal(const double* __restrict__ lin, int M, int k, double w0, double w1,
                                                  double w2, double w3) {
    double rec[LIN_C];
#pragma unroll
    for (int c = 0; c < LIN_C; ++c) rec[c] = lin[(size_t)c * M + k];
    V3<double> er{rec[0], rec[1], rec[2]}, ep{rec[3], rec[4], rec[5]}, eR{rec[24], rec[25], rec[26]};
    M3<double> G = m3_load(rec + 6), C = m3_load(rec + 15), B = m3_load(rec + 27);
    M3<double> Gt = transpose(G), Ct = transpose(C), Bt = transpose(B);
    M3<double> GtG = Gt * G;
    LinkNormal o;
    o.rv = {rec[36], rec[37], rec[38]};
    o.rt = {rec[39], rec[40], rec[41]};
    o.Srr = w0 * GtG + w3 * m3_identity<double>();
    o.Srp = w0 * (Gt * C);
    o.Spp = w0 * (Ct * C + GtG) + w2 * (Bt * B);
    o.gr = w0 * (Gt * er) + w3 * o.rt;
    o.gp = w0 * (Ct * er + Gt * ep) + w2 * (Bt * eR);
    return o;
}

__device__ __forceinline__ void put3x3(double* H, int r0, int c0, M3<double> a) {
    H[(r0 + 0) * 9 + c0 + 0] = a.a00; H[(r0 + 0) * 9 + c0 + 1] = a.a01; H[(r0 + 0) * 9 + c0 + 2] = a.a02;
    H[(r0 + 1) * 9 + c0 + 0] = a.a10; H[(r0 + 1) * 9 + c0 + 1] = a.a11; H[(r0 + 1) * 9 + c0 + 2] = a.a12;
    H[(r0 + 2) * 9 + c0 + 0] = a.a20; H[(r0 + 2) * 9 + c0 + 1] = a.a21; H[(r0 + 2) * 9 + c0 + 2] = a.a22;
}

// the tail of every chain build: node block Hd[k] (row-major 9x9, order [rho, phi, v]) from its six upper blocks with the nine diagonal
// entries clamped (A.diagonal().clamp_(min, max)), and rhs[k] = -g.  (The three clamped blocks by value, the rest by reference, the
// addresses formed where they are used: in this form info9_build_kernel keeps its 434 VGPRs without a spill.)
__device__ __forceinline__ void store_node(M3<double> Hrr, const M3<double>& Hrp, const M3<double>& Hrv, M3<double> Hpp,
                                           const M3<double>& Hpv, M3<double> Hvv, const V3<double>& gr, const V3<double>& gp,
                                           const V3<double>& gv, double vmin, double vmax, double* __restrict__ Hd,
                                           double* __restrict__ rhs, int k) {
    const auto clamp = [&](double v) { return fmin(fmax(v, vmin), vmax); };
    Hrr.a00 = clamp(Hrr.a00); Hrr.a11 = clamp(Hrr.a11); Hrr.a22 = clamp(Hrr.a22);
    Hpp.a00 = clamp(Hpp.a00); Hpp.a11 = clamp(Hpp.a11); Hpp.a22 = clamp(Hpp.a22);
    Hvv.a00 = clamp(Hvv.a00); Hvv.a11 = clamp(Hvv.a11); Hvv.a22 = clamp(Hvv.a22);
    double* h = Hd + (size_t)k * 81;
    put3x3(h, 0, 0, Hrr); put3x3(h, 0, 3, Hrp); put3x3(h, 0, 6, Hrv);
    put3x3(h, 3, 0, transpose(Hrp)); put3x3(h, 3, 3, Hpp); put3x3(h, 3, 6, Hpv);
    put3x3(h, 6, 0, transpose(Hrv)); put3x3(h, 6, 3, transpose(Hpv)); put3x3(h, 6, 6, Hvv);
    double* b = rhs + (size_t)k * 9;
    b[0] = -gr.x; b[1] = -gr.y; b[2] = -gr.z; b[3] = -gp.x; b[4] = -gp.y; b[5] = -gp.z;
    b[6] = -gv.x; b[7] = -gv.y; b[8] = -gv.z;
}

// one lane per node: gather the two adjacent links into Hd[k], Ho[k] (coupling k -> k+1), rhs[k] = -J^T W r
// SCALED: w1, w2, w3 of link k are multiplied by its robust multipliers c_imu[0..2][k] (islam_pvgo_build_normal_scaled)
template <bool SCALED>
__global__ __launch_bounds__(64) void build_normal_kernel(const double* __restrict__ lin, const double* __restrict__ dts,
                                                           int N, double w0, double w1, double w2, double w3, double vmin,
                                                           double vmax, double* __restrict__ Hd, double* __restrict__ Ho,
                                                           double* __restrict__ rhs, const double* __restrict__ c_imu) {
    int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= N) return;
    const int M = N - 1;
    const M3<double> Z{0, 0, 0, 0, 0, 0, 0, 0, 0};
    const M3<double> I = m3_identity<double>();
    M3<double> Hrr = Z, Hrp = Z, Hpp = Z;
    V3<double> gr{0, 0, 0}, gp{0, 0, 0}, gv{0, 0, 0};
    double hvv = 0.0, hrv = 0.0;
    auto wl = [&](double w, int g, int l) { if constexpr (SCALED) return w * c_imu[(size_t)g * M + l]; else return w; };
    if (k > 0) {                       // link k-1, this node is its "j" end
        const double w1l = wl(w1, 0, k - 1);
        LinkNormal L = link_normal(lin, M, k - 1, w0, w1l, wl(w2, 1, k - 1), wl(w3, 2, k - 1));
        Hrr = Hrr + L.Srr; Hrp = Hrp + L.Srp; Hpp = Hpp + L.Spp;
        gr = gr + L.gr; gp = gp + L.gp;
        gv = gv - w1l * L.rv;
        hvv += w1l;
    }
    double* o = Ho + (size_t)k * 81;
    if (k < M) {                       // link k, this node is its "i" end
        const double w1l = wl(w1, 0, k), w3l = wl(w3, 2, k);
        LinkNormal L = link_normal(lin, M, k, w0, w1l, wl(w2, 1, k), w3l);
        double dt = dts[k];
        Hrr = Hrr + L.Srr; Hrp = Hrp + L.Srp; Hpp = Hpp + L.Spp;
        gr = gr - L.gr; gp = gp - L.gp;
        gv = gv + w1l * L.rv - (w3l * dt) * L.rt;
        hvv += w1l + w3l * dt * dt;
        hrv = w3l * dt;
        put3x3(o, 0, 0, -1.0 * L.Srr); put3x3(o, 0, 3, -1.0 * L.Srp); put3x3(o, 0, 6, Z);
        put3x3(o, 3, 0, -1.0 * transpose(L.Srp)); put3x3(o, 3, 3, -1.0 * L.Spp); put3x3(o, 3, 6, Z);
        put3x3(o, 6, 0, (-w3l * dt) * I); put3x3(o, 6, 3, Z); put3x3(o, 6, 6, (-w1l) * I);
    }
    store_node(Hrr, Hrp, hrv * I, Hpp, Z, hvv * I, gr, gp, gv, vmin, vmax, Hd, rhs, k);
}

// ------------------------------------------------------------------------------------------
// Per-factor information matrices (pvgo.py:133-162 hands PyPose one matrix per factor).  Packed once per run:
// info_vo (21, E) = the upper triangle of each 6x6 Omega0 in row-major order of the triangle, info_imu (18, M) = the 6-entry upper
// triangles [00 01 02 11 12 22] of [velocity | rotation | translation-velocity]; both component-major like `lin`, so a wavefront's
// loads coalesce.  Everything below stays in M3 / V3 values: no per-lane array, no scratch.
__device__ __forceinline__ M3<double> sym3_ld(const double* __restrict__ p, size_t ld) {
    const double a = p[0], b = p[ld], c = p[2 * ld], d = p[3 * ld], e = p[4 * ld], f = p[5 * ld];
    return {a, b, c, b, d, e, c, e, f};
}
__device__ __forceinline__ M3<double> sym_part(M3<double> a) { return 0.5 * (a + transpose(a)); }

// A^T Omega0 A and A^T Omega0 e of one VO factor, A = [[G, C],[0, G]], from the 3x3 blocks of Omega0 = [[Waa, Wab],[Wab^T, Wbb]]
// (entry c of the packed triangle at w[c * ld]).  The two diagonal blocks are symmetrised: X^T (W X) is symmetric only up to rounding.
struct PoseNormal { M3<double> Srr, Srp, Spp; V3<double> gr, gp; };      // the pose-block pieces of one factor: S and J_j^T W r
__device__ __forceinline__ PoseNormal info_vo_normal(const double* __restrict__ w, size_t ld, M3<double> G, M3<double> C, V3<double> er,
                                                 V3<double> ep) {
    const M3<double> Waa{w[0], w[ld], w[2 * ld], w[ld], w[6 * ld], w[7 * ld], w[2 * ld], w[7 * ld], w[11 * ld]};
    const M3<double> Wab{w[3 * ld], w[4 * ld], w[5 * ld], w[8 * ld], w[9 * ld], w[10 * ld], w[12 * ld], w[13 * ld], w[14 * ld]};
    const M3<double> Wbb = sym3_ld(w + 15 * ld, ld);
    const M3<double> Gt = transpose(G), Ct = transpose(C), Wba = transpose(Wab);
    const M3<double> X1 = Waa * G, X2 = Waa * C + Wab * G;          // (Omega0 A) top row
    const M3<double> X4 = Wba * C + Wbb * G;                        // (Omega0 A) bottom right
    const V3<double> u = Waa * er + Wab * ep, v = Wba * er + Wbb * ep;
    PoseNormal o;
    o.Srr = sym_part(Gt * X1);
    o.Srp = Gt * X2;
    o.Spp = sym_part(Ct * X2 + Gt * X4);
    o.gr = Gt * u;
    o.gp = Ct * u + Gt * v;
    return o;
}
// the VO group of link k (6x6 Omega0) from the chain's `lin`
__device__ __forceinline__ PoseNormal info_link_vo(const double* __restrict__ lin, int M, int k, const double* __restrict__ info_vo) {
    const double* r = lin + k;
    const size_t ld = (size_t)M;
    return info_vo_normal(info_vo + k, ld, lin_m3(r, ld, 6), lin_m3(r, ld, 15), lin_v3(r, ld, 0), lin_v3(r, ld, 3));
}

struct InfoLink {         // per-link normal-equation pieces under information matrices
    M3<double> Srr, Srp, Spp;   // pose-pose block S
    M3<double> W1, W3;          // Omega1, Omega3
    V3<double> gr, gp;          // pose gradient
    V3<double> g1, g3;          // Omega1 rv, Omega3 rt
};

// info_vo == nullptr: no VO group (the general-topology callers add the VO factors per edge themselves)
__device__ __forceinline__ InfoLink info_link(const double* __restrict__ lin, int M, int k, const double* __restrict__ info_vo,
                                              const double* __restrict__ info_imu) {
    const double* r = lin + k;
    const size_t ld = (size_t)M;
    const M3<double> B = lin_m3(r, ld, 27);
    const V3<double> eR = lin_v3(r, ld, 24), rv = lin_v3(r, ld, 36), rt = lin_v3(r, ld, 39);
    const double* wi = info_imu + k;
    const M3<double> W2 = sym3_ld(wi + 6 * ld, ld);
    InfoLink o;
    o.W1 = sym3_ld(wi, ld);
    o.W3 = sym3_ld(wi + 12 * ld, ld);
    const M3<double> W2B = W2 * B;
    o.Srr = o.W3;
    o.Spp = sym_part(transpose(B) * W2B);
    o.g1 = o.W1 * rv;
    o.g3 = o.W3 * rt;
    o.gr = o.g3;
    o.gp = tmul(W2B, eR);                                           // B^T Omega2 er (Omega2 symmetric)
    if (info_vo) {
        const PoseNormal q = info_link_vo(lin, M, k, info_vo);
        o.Srr = o.Srr + q.Srr; o.Srp = q.Srp; o.Spp = o.Spp + q.Spp;
        o.gr = o.gr + q.gr; o.gp = o.gp + q.gp;
    } else {
        o.Srp = M3<double>{0, 0, 0, 0, 0, 0, 0, 0, 0};
    }
    return o;
}

// build_normal_kernel with one information matrix per factor: A = sum J^T Omega J, rhs = -sum J^T Omega r, the same gather (link k-1,
// then link k), the same clamp.  A closed gate makes it a no-op (the LM loop enqueues it behind linbuild_kernel / trial_lin_kernel,
// over the buffers that launch filled).
__global__ __launch_bounds__(64) void info_build_kernel(const double* __restrict__ lin, const double* __restrict__ dts, int N,
                                                         const double* __restrict__ info_vo, const double* __restrict__ info_imu,
                                                         double vmin, double vmax, double* __restrict__ Hd, double* __restrict__ Ho,
                                                         double* __restrict__ rhs, Gate gate) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= N || gate_closed(gate)) return;
    const int M = N - 1;
    const M3<double> Z{0, 0, 0, 0, 0, 0, 0, 0, 0};
    M3<double> Hrr = Z, Hrp = Z, Hpp = Z, Hvv = Z, Hrv = Z;
    V3<double> gr{0, 0, 0}, gp{0, 0, 0}, gv{0, 0, 0};
    if (k > 0) {                       // link k-1, this node is its "j" end
        const InfoLink L = info_link(lin, M, k - 1, info_vo, info_imu);
        Hrr = Hrr + L.Srr; Hrp = Hrp + L.Srp; Hpp = Hpp + L.Spp;
        gr = gr + L.gr; gp = gp + L.gp;
        gv = gv - L.g1;
        Hvv = Hvv + L.W1;
    }
    if (k < M) {                       // link k, this node is its "i" end
        const InfoLink L = info_link(lin, M, k, info_vo, info_imu);
        const double dt = dts[k];
        Hrr = Hrr + L.Srr; Hrp = Hrp + L.Srp; Hpp = Hpp + L.Spp;
        gr = gr - L.gr; gp = gp - L.gp;
        gv = gv + L.g1 - dt * L.g3;
        Hvv = Hvv + L.W1 + (dt * dt) * L.W3;
        Hrv = dt * L.W3;
        double* o = Ho + (size_t)k * 81;
        put3x3(o, 0, 0, -1.0 * L.Srr); put3x3(o, 0, 3, -1.0 * L.Srp); put3x3(o, 0, 6, Z);
        put3x3(o, 3, 0, -1.0 * transpose(L.Srp)); put3x3(o, 3, 3, -1.0 * L.Spp); put3x3(o, 3, 6, Z);
        put3x3(o, 6, 0, -1.0 * Hrv); put3x3(o, 6, 3, Z); put3x3(o, 6, 6, -1.0 * L.W1);
    }
    store_node(Hrr, Hrp, Hrv, Hpp, Z, Hvv, gr, gp, gv, vmin, vmax, Hd, rhs, k);   // (Hrv = dt Omega3 is symmetric)
}

// ------------------------------------------------------------------------------------------
// Correlated IMU information: ONE 9x9 Omega per link on the stacked residual r9 = [rv; er; rt], packed as
// info_imu9 (45, M) = its upper triangle in row-major order of the triangle, component-major.  With J_j = [[0,0,-I],[0,B,0],[I,0,0]]
// (rows v, r, t; columns rho, phi, v) and J_i = -J_j - dt E, E = I at (t rows, v columns), everything a link adds follows from
// P = J_j^T Omega J_j and its rho row [P_rr, P_rp, P_rv] = Omega_t. J_j:
//   Hd[j] += P;   Hd[i] += P + dt (column v += [P_rr; P_rp^T; P_rv^T], row v += its transpose) + dt^2 P_rr on v-v;
//   Ho[k] = -P, row v -= dt [P_rr, P_rp, P_rv];   g_j = J_j^T y,  g_i = -g_j - dt [0; 0; y_t],  y = Omega r9.
constexpr int tri9(int r, int c) { return r * 9 - r * (r - 1) / 2 + (c - r); }       // r <= c

struct InfoLink9 {        // the IMU part of one link: the upper blocks of P in node order [rho, phi, v], and J_j^T Omega r9
    M3<double> Prr, Prp, Prv, Ppp, Ppv, Pvv;
    V3<double> gr, gp, gv;
};

__device__ __forceinline__ InfoLink9 info_link9(const double* __restrict__ lin, int M, int k, const double* __restrict__ info_imu9) {
    const double* r = lin + k;
    const double* w = info_imu9 + k;
    const size_t ld = (size_t)M;
    auto W = [&](int a, int b) { return w[tri9(a, b) * ld]; };
    auto symblk = [&](int o) {
        const double a = W(o, o), b = W(o, o + 1), c = W(o, o + 2), d = W(o + 1, o + 1), e = W(o + 1, o + 2), f = W(o + 2, o + 2);
        return M3<double>{a, b, c, b, d, e, c, e, f};
    };
    auto offblk = [&](int a, int b) {
        return M3<double>{W(a, b), W(a, b + 1), W(a, b + 2), W(a + 1, b), W(a + 1, b + 1), W(a + 1, b + 2),
                          W(a + 2, b), W(a + 2, b + 1), W(a + 2, b + 2)};
    };
    const M3<double> B = lin_m3(r, ld, 27);
    const V3<double> eR = lin_v3(r, ld, 24), rv = lin_v3(r, ld, 36), rt = lin_v3(r, ld, 39);
    const M3<double> Wvv = symblk(0), Wrr = symblk(3), Wtt = symblk(6);
    const M3<double> Wvr = offblk(0, 3), Wvt = offblk(0, 6), Wrt = offblk(3, 6);
    const M3<double> Bt = transpose(B);
    InfoLink9 o;
    o.Prr = Wtt;
    o.Prp = transpose(Wrt) * B;                                     // Omega_tr B
    o.Prv = -1.0 * transpose(Wvt);                                  // -Omega_tv
    o.Ppp = sym_part(Bt * (Wrr * B));
    o.Ppv = -1.0 * (Bt * transpose(Wvr));                           // -B^T Omega_rv
    o.Pvv = Wvv;
    const V3<double> yv = Wvv * rv + Wvr * eR + Wvt * rt;
    const V3<double> yr = tmul(Wvr, rv) + Wrr * eR + Wrt * rt;
    o.gr = tmul(Wvt, rv) + tmul(Wrt, eR) + Wtt * rt;                // y_t
    o.gp = tmul(B, yr);
    o.gv = -yv;
    return o;
}

// info_build_kernel for the correlated form: the same gather (link k-1 as its j end, then link k as its i end), the same outputs, gate
// and clamp.  One lane per node; Ho[k] is stored as soon as link k is formed.  No atomics, no waits: a second call gives the same bits.
__global__ __launch_bounds__(64) void info9_build_kernel(const double* __restrict__ lin, const double* __restrict__ dts, int N,
                                                          const double* __restrict__ info_vo, const double* __restrict__ info_imu9,
                                                          double vmin, double vmax, double* __restrict__ Hd, double* __restrict__ Ho,
                                                          double* __restrict__ rhs, Gate gate) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= N || gate_closed(gate)) return;
    const int M = N - 1;
    const M3<double> Z{0, 0, 0, 0, 0, 0, 0, 0, 0};
    M3<double> Hrr = Z, Hrp = Z, Hrv = Z, Hpp = Z, Hpv = Z, Hvv = Z;
    V3<double> gr{0, 0, 0}, gp{0, 0, 0}, gv{0, 0, 0};
    // (sched_barrier between the IMU and the VO part of a link: left to itself the scheduler issues every load of both up front and
    // runs out of registers; in this order the peak is one part's operands plus the accumulators)
    if (k > 0) {                       // link k-1, this node is its "j" end
        const InfoLink9 L = info_link9(lin, M, k - 1, info_imu9);
        Hrr = L.Prr; Hrp = L.Prp; Hrv = L.Prv; Hpp = L.Ppp; Hpv = L.Ppv; Hvv = L.Pvv;
        gr = L.gr; gp = L.gp; gv = L.gv;
        __builtin_amdgcn_sched_barrier(0);
        if (info_vo) {
            const PoseNormal q = info_link_vo(lin, M, k - 1, info_vo);
            Hrr = Hrr + q.Srr; Hrp = Hrp + q.Srp; Hpp = Hpp + q.Spp;
            gr = gr + q.gr; gp = gp + q.gp;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (k < M) {                       // link k, this node is its "i" end
        const double dt = dts[k];
        double* o = Ho + (size_t)k * 81;
        M3<double> Srr, Srp, Spp;                                   // the pose block: IMU part, then the VO group
        V3<double> lr, lp;
        {
            const InfoLink9 L = info_link9(lin, M, k, info_imu9);
            put3x3(o, 0, 6, -1.0 * L.Prv); put3x3(o, 3, 6, -1.0 * L.Ppv);                     // the v row and column are IMU only
            put3x3(o, 6, 0, -1.0 * (transpose(L.Prv) + dt * L.Prr)); put3x3(o, 6, 3, -1.0 * (transpose(L.Ppv) + dt * L.Prp));
            put3x3(o, 6, 6, -1.0 * (L.Pvv + dt * L.Prv));
            Hrv = Hrv + (L.Prv + dt * L.Prr);
            Hpv = Hpv + (L.Ppv + dt * transpose(L.Prp));
            Hvv = Hvv + (L.Pvv + dt * (L.Prv + transpose(L.Prv)) + (dt * dt) * L.Prr);
            gv = gv - L.gv - dt * L.gr;
            Srr = L.Prr; Srp = L.Prp; Spp = L.Ppp; lr = L.gr; lp = L.gp;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (info_vo) {
            const PoseNormal q = info_link_vo(lin, M, k, info_vo);
            Srr = Srr + q.Srr; Srp = Srp + q.Srp; Spp = Spp + q.Spp;
            lr = lr + q.gr; lp = lp + q.gp;
        }
        put3x3(o, 0, 0, -1.0 * Srr); put3x3(o, 0, 3, -1.0 * Srp);
        put3x3(o, 3, 0, -1.0 * transpose(Srp)); put3x3(o, 3, 3, -1.0 * Spp);
        Hrr = Hrr + Srr; Hrp = Hrp + Srp; Hpp = Hpp + Spp;
        gr = gr - lr; gp = gp - lp;
    }
    store_node(Hrr, Hrp, Hrv, Hpp, Hpv, Hvv, gr, gp, gv, vmin, vmax, Hd, rhs, k);
}

// ------------------------------------------------------------------------------------------
// Sparse reprojection factor (pvgo.py:53-61 + dense_ba.py:276-305).  Link k: T = C^-1 (X_k^-1 X_{k+1}) C,
// err_j = pixel(K, T^-1 P_j) - target_j.  Under the left perturbation T <- Exp(eta) T:  d p'/d eta = R_T^T [-I, [P]x], so
// with a = (f/z) R^T[row] - (f c/z^2) R^T[2]:  d err / d eta = [-a, a x P].  Node perturbations enter through
// eta = +-Ad(C^-1 X_k^-1) delta (same +/- pattern as the VO factor), applied per link in linbuild / trial.
struct ReprojDev {
    const double* points;
    const double* targets;
    int K;
    double fx, fy, cx, cy;
    SE3<double> C;
    double weight;
    int compat_first;
};
constexpr int RP_REC = ISLAM_REPROJ_REC;    // 21 (J^T J upper) + 6 (J^T r) + 1 (r^T r), padded to 32
constexpr int RP_NSUM = 28;

// one workgroup per link, lanes stride over the keypoints; fixed-order reduction (bit-reproducible)
__global__ __launch_bounds__(256) void reproj_reduce_kernel(const double* __restrict__ nodes, const double* __restrict__ dx,
                                                             int M, ReprojDev rp, double* __restrict__ red, Gate gate) {
    extern __shared__ __attribute__((aligned(16))) double sw[];   // blockDim.x rows of RP_NSUM + 1 doubles
    const int L = xcd_index(blockIdx.x, M);
    if (L < 0 || gate_closed(gate)) return;
    SE3<double> Xi = se3_load(nodes + 7 * L), Xj = se3_load(nodes + 7 * (L + 1));
    if (dx) {
        const double* di = dx + (size_t)L * 9;
        Xi = se3_mul(se3_exp(ld3(di), ld3(di + 3)), Xi);
        Xj = se3_mul(se3_exp(ld3(di + 9), ld3(di + 12)), Xj);
    }
    SE3<double> motion = se3_mul(se3_inv(Xi), Xj);
    const bool frozen = rp.compat_first && L == 0;              // pvgo.py:57: motion[0] = 0.1 (all seven entries)
    if (frozen) motion = {{0.1, 0.1, 0.1}, {0.1, 0.1, 0.1, 0.1}};
    const SE3<double> Tinv = se3_inv(se3_mul(se3_mul(se3_inv(rp.C), motion), rp.C));
    const M3<double> Rm = qmat(Tinv.q);
    const V3<double> r0{Rm.a00, Rm.a01, Rm.a02}, r1{Rm.a10, Rm.a11, Rm.a12}, r2{Rm.a20, Rm.a21, Rm.a22};
    double acc[RP_NSUM];
#pragma unroll
    for (int i = 0; i < RP_NSUM; ++i) acc[i] = 0.0;
    const double* P0 = rp.points + (size_t)L * rp.K * 3;
    const double* T0 = rp.targets + (size_t)L * rp.K * 2;
    for (int j = threadIdx.x; j < rp.K; j += blockDim.x) {
        const V3<double> P = ld3(P0 + 3 * j);
        const V3<double> p = qact(Tinv.q, P) + Tinv.t;
        double den = fmax(fabs(p.z), 2.2250738585072014e-308);     // homo2cart: |z| clamped to finfo.tiny, sign kept
        den = p.z >= 0.0 ? den : -den;
        const double ru = (rp.fx * p.x + rp.cx * p.z) / den - T0[2 * j];
        const double rv = (rp.fy * p.y + rp.cy * p.z) / den - T0[2 * j + 1];
        const double iz = 1.0 / den;
        const V3<double> au = (rp.fx * iz) * r0 - (rp.fx * p.x * iz * iz) * r2;
        const V3<double> av = (rp.fy * iz) * r1 - (rp.fy * p.y * iz * iz) * r2;
        const V3<double> cu = cross(au, P), cv = cross(av, P);
        const double ju[6] = {-au.x, -au.y, -au.z, cu.x, cu.y, cu.z};
        const double jv[6] = {-av.x, -av.y, -av.z, cv.x, cv.y, cv.z};
        int o = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[o++] += ju[a] * ju[b] + jv[a] * jv[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += ju[a] * ru + jv[a] * rv;
        acc[27] += ru * ru + rv * rv;
    }
    // 28 sums over the workgroup through LDS (row stride 29: conflict-free), added in thread order by 28 lanes: a shuffle
    // reduction of a double is two ds_bpermute per step -- 28 x 6 x 2 of them cost more than the keypoint loop
#pragma unroll
    for (int i = 0; i < RP_NSUM; ++i) sw[threadIdx.x * (RP_NSUM + 1) + i] = acc[i];
    __syncthreads();
    if (threadIdx.x < RP_REC) {
        double s = 0.0;
        if (threadIdx.x < RP_NSUM) {
            const int nt = blockDim.x;
            for (int t = 0; t < nt; ++t) s += sw[t * (RP_NSUM + 1) + threadIdx.x];
            if (frozen && threadIdx.x < 27) s = 0.0;            // a constant residual: no Jacobian
        }
        red[(size_t)L * RP_REC + threadIdx.x] = s;
    }
}

// per-link pieces of the reprojection factor in node coordinates: A = M^T S M, g = M^T b with M = Ad(C^-1 X_i^-1)
struct ReprojLink { M3<double> Arr, Arp, App; V3<double> gr, gp; };

__device__ __forceinline__ M3<double> sym_from(const double* u, int r0, int c0) {   // 3x3 sub-block of a packed upper 6x6
    auto at = [&](int r, int c) { if (r > c) { int t = r; r = c; c = t; } return u[r * 6 - r * (r - 1) / 2 + (c - r)]; };
    return {at(r0, c0), at(r0, c0 + 1), at(r0, c0 + 2), at(r0 + 1, c0), at(r0 + 1, c0 + 1), at(r0 + 1, c0 + 2),
            at(r0 + 2, c0), at(r0 + 2, c0 + 1), at(r0 + 2, c0 + 2)};
}

__device__ __forceinline__ void reproj_adjoint(const ReprojDev& rp, SE3<double> Xi, M3<double>& R, M3<double>& T) {
    const SE3<double> Y = se3_mul(se3_inv(rp.C), se3_inv(Xi));
    R = qmat(Y.q);
    T = skew(Y.t) * R;
}

__device__ __forceinline__ ReprojLink reproj_link(const double* __restrict__ rec, const ReprojDev& rp, SE3<double> Xi) {
    double u[RP_NSUM];
#pragma unroll
    for (int i = 0; i < RP_NSUM; ++i) u[i] = rec[i];
    const M3<double> Saa = sym_from(u, 0, 0), Sab = sym_from(u, 0, 3), Sbb = sym_from(u, 3, 3);
    const V3<double> ba{u[21], u[22], u[23]}, bb{u[24], u[25], u[26]};
    M3<double> R, T;
    reproj_adjoint(rp, Xi, R, T);
    const M3<double> Rt = transpose(R), Tt = transpose(T);
    const M3<double> X1 = Saa * T + Sab * R;                    // (S M) top-right
    const M3<double> X2 = transpose(Sab) * T + Sbb * R;         // (S M) bottom-right
    ReprojLink o;
    o.Arr = Rt * (Saa * R);
    o.Arp = Rt * X1;
    o.App = Tt * X1 + Rt * X2;
    o.gr = tmul(R, ba);
    o.gp = tmul(T, ba) + tmul(R, bb);
    return o;
}

// Fused linearise + build (what the LM loop launches): a workgroup of 64 lanes linearises 64 consecutive links (the
// first one is a halo shared with the previous workgroup), hands the weighted per-link pieces over through LDS and builds
// the blocks of its 63 nodes.  Same arithmetic as linearize_kernel + build_normal_kernel, one launch, no re-read of `lin`.
#ifndef ISLAM_LB_NODES
#define ISLAM_LB_NODES 63
#endif
constexpr int LB_NODES = ISLAM_LB_NODES;   // nodes per workgroup of linbuild / trial_lin (<= 63: lane 0 = the link shared with the previous block)
constexpr int LB_THREADS = 256;       // wave 0 linearises the links; waves 0-2 build Hd / Ho / rhs; all four copy out
constexpr int LB_DYN_BYTES = (2 * LB_NODES * 81 + LB_NODES * 9) * (int)sizeof(double);
constexpr int LB_REC = 41;          // Srr 9 | Srp 9 | Spp 9 | gr 3 | gp 3 | rv 3 | rt 3 | dt 1, +1 pad

struct LinWeights { double w0, w1, w2, w3, vmin, vmax; };

// Robust kernels of the four factor groups (VO, velocity, IMU rotation, translation-velocity): islam_pvgo_robust by value.
// rho(s) of the unweighted squared norm s of one factor's residual, c = rho'(s) (PyPose's pp.optim.kernel + FastTriggs).
struct RobustDev { int kind[4]; double delta[4]; };
constexpr int LB_REC_ROBUST = 43;   // LB_REC + c1 w1 | c3 w3 (the weights nodes_build_copy applies), +1 pad: odd row stride

__device__ __forceinline__ double robust_rho(int kind, double delta, double s, double& c) {
    if (kind == ISLAM_ROBUST_HUBER) {
        const double d2 = delta * delta;
        if (s <= d2) { c = 1.0; return s; }
        const double r = sqrt(s);
        c = delta / r;
        return 2.0 * delta * r - d2;
    }
    if (kind == ISLAM_ROBUST_CAUCHY) {
        const double d2 = delta * delta;
        const double u = s / d2;
        c = 1.0 / (1.0 + u);
        return d2 * log1p(u);
    }
    c = 1.0;
    return s;
}

// sum of rho over the four factors of one link and their multipliers c[4] (residuals: erho, ephi | rv | er | rt)
__device__ __forceinline__ double robust_link(const RobustDev& rb, V3<double> erho, V3<double> ephi, V3<double> rv, V3<double> er,
                                              V3<double> rt, double c[4]) {
    double l = robust_rho(rb.kind[0], rb.delta[0], dot(erho, erho) + dot(ephi, ephi), c[0]);
    l += robust_rho(rb.kind[1], rb.delta[1], dot(rv, rv), c[1]);
    l += robust_rho(rb.kind[2], rb.delta[2], dot(er, er), c[2]);
    l += robust_rho(rb.kind[3], rb.delta[3], dot(rt, rt), c[3]);
    return l;
}

// Jacobian blocks of one link at its residuals: d pgerr / d delta_j = [[G, C],[0, G]], d imuroterr / d phi_j = B
__device__ __forceinline__ void link_jacobians(const LinkRes& r, M3<double>& G, M3<double>& C, M3<double>& B) {
    vo_jacobians(r.pre, r.erho, r.ephi, r.Ji, G, C);
    B = so3_Jl_inv(r.er) * qmat(r.rpre);
}

// lin record of link L (component-major) + the weighted per-link pieces handed to the node builders through LDS
__device__ __forceinline__ void link_emit(const LinkRes& r, const M3<double>& G, const M3<double>& C, const M3<double>& B,
                                          double dt, int L, int M, bool owns, const LinWeights& W, double* __restrict__ lin,
                                          double* __restrict__ o, const double* __restrict__ red, const ReprojDev& rp,
                                          SE3<double> Xi) {
    if (owns) {                                               // the halo link belongs to the previous workgroup
        double rec[LIN_C];
        rec[0] = r.erho.x; rec[1] = r.erho.y; rec[2] = r.erho.z;
        rec[3] = r.ephi.x; rec[4] = r.ephi.y; rec[5] = r.ephi.z;
        m3_store(G, rec + 6);
        m3_store(C, rec + 15);
        rec[24] = r.er.x; rec[25] = r.er.y; rec[26] = r.er.z;
        m3_store(B, rec + 27);
        rec[36] = r.rv.x; rec[37] = r.rv.y; rec[38] = r.rv.z;
        rec[39] = r.rt.x; rec[40] = r.rt.y; rec[41] = r.rt.z;
#pragma unroll
        for (int c = 0; c < LIN_C; ++c) lin[(size_t)c * M + L] = rec[c];
    }
    const M3<double> Gt = transpose(G), Ct = transpose(C), Bt = transpose(B);
    const M3<double> GtG = Gt * G;
    M3<double> Srr = W.w0 * GtG + W.w3 * m3_identity<double>();
    M3<double> Srp = W.w0 * (Gt * C);
    M3<double> Spp = W.w0 * (Ct * C + GtG) + W.w2 * (Bt * B);
    V3<double> gr = W.w0 * (Gt * r.erho) + W.w3 * r.rt;
    V3<double> gp = W.w0 * (Ct * r.erho + Gt * r.ephi) + W.w2 * (Bt * r.er);
    if (red) {                                                // 5th residual: same +/- coupling pattern as the VO factor
        const ReprojLink q = reproj_link(red + (size_t)L * RP_REC, rp, Xi);
        Srr = Srr + rp.weight * q.Arr; Srp = Srp + rp.weight * q.Arp; Spp = Spp + rp.weight * q.App;
        gr = gr + rp.weight * q.gr; gp = gp + rp.weight * q.gp;
    }
    m3_store(Srr, o);
    m3_store(Srp, o + 9);
    m3_store(Spp, o + 18);
    o[27] = gr.x; o[28] = gr.y; o[29] = gr.z; o[30] = gp.x; o[31] = gp.y; o[32] = gp.z;
    o[33] = r.rv.x; o[34] = r.rv.y; o[35] = r.rv.z; o[36] = r.rt.x; o[37] = r.rt.y; o[38] = r.rt.z; o[39] = dt;
}

// After the link pieces are in `sl` (workgroup barrier done by the caller): waves 0-2 build Hd / Ho / rhs of the
// workgroup's 63 nodes in LDS (node k = links k-1 in slot lane and k in slot lane+1), then all waves copy the three
// contiguous ranges out with lane-contiguous addresses (a lane-per-node store of a 9x9 block touches 64 cache lines).
// (REC == LB_REC_ROBUST: the velocity and translation-velocity weights are per link, c w1 at [40] and c w3 at [41] of its record)
template <int REC>
__device__ __forceinline__ void nodes_build_copy(const double (*sl)[REC], double* __restrict__ lb_out, int blk, int N,
                                                 const LinWeights& W, double* __restrict__ Hd, double* __restrict__ Ho,
                                                 double* __restrict__ rhs) {
    constexpr bool per_link = REC == LB_REC_ROBUST;
    double* const oHd = lb_out;
    double* const oHo = lb_out + LB_NODES * 81;
    double* const oR = lb_out + 2 * LB_NODES * 81;
    const int M = N - 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blk * LB_NODES + lane;
    const int cnt = min(LB_NODES, N - blk * LB_NODES);             // nodes of this workgroup
    const double w1 = W.w1, w3 = W.w3;
    if (lane < cnt && wave < 3) {
        const M3<double> Z{0, 0, 0, 0, 0, 0, 0, 0, 0};
        const M3<double> I = m3_identity<double>();
        const double* a0 = sl[lane];
        const double* a1 = sl[lane + 1];
        auto w1_of = [&](const double* a) { if constexpr (per_link) return a[40]; else return w1; };
        auto w3_of = [&](const double* a) { if constexpr (per_link) return a[41]; else return w3; };
        if (wave == 0) {                                            // Hd
            M3<double> Hrr = Z, Hrp = Z, Hpp = Z;
            double hvv = 0.0, hrv = 0.0;
            if (k > 0) {
                Hrr = Hrr + m3_load(a0); Hrp = Hrp + m3_load(a0 + 9); Hpp = Hpp + m3_load(a0 + 18);
                hvv += w1_of(a0);
            }
            if (k < M) {
                const double dt = a1[39];
                Hrr = Hrr + m3_load(a1); Hrp = Hrp + m3_load(a1 + 9); Hpp = Hpp + m3_load(a1 + 18);
                hvv += w1_of(a1) + w3_of(a1) * dt * dt;
                hrv = w3_of(a1) * dt;
            }
            double h[81];
            put3x3(h, 0, 0, Hrr); put3x3(h, 0, 3, Hrp); put3x3(h, 0, 6, hrv * I);
            put3x3(h, 3, 0, transpose(Hrp)); put3x3(h, 3, 3, Hpp); put3x3(h, 3, 6, Z);
            put3x3(h, 6, 0, hrv * I); put3x3(h, 6, 3, Z); put3x3(h, 6, 6, hvv * I);
#pragma unroll
            for (int d = 0; d < 9; ++d) h[d * 10] = fmin(fmax(h[d * 10], W.vmin), W.vmax);   // A.diagonal().clamp_(min, max)
#pragma unroll
            for (int e = 0; e < 81; ++e) oHd[lane * 81 + e] = h[e];
        } else if (wave == 1) {                                     // Ho (coupling k -> k+1); the last node has none
            if (k < M) {
                const M3<double> Srr = m3_load(a1), Srp = m3_load(a1 + 9), Spp = m3_load(a1 + 18);
                const double dt = a1[39];
                double o[81];
                put3x3(o, 0, 0, -1.0 * Srr); put3x3(o, 0, 3, -1.0 * Srp); put3x3(o, 0, 6, Z);
                put3x3(o, 3, 0, -1.0 * transpose(Srp)); put3x3(o, 3, 3, -1.0 * Spp); put3x3(o, 3, 6, Z);
                put3x3(o, 6, 0, (-w3_of(a1) * dt) * I); put3x3(o, 6, 3, Z); put3x3(o, 6, 6, (-w1_of(a1)) * I);
#pragma unroll
                for (int e = 0; e < 81; ++e) oHo[lane * 81 + e] = o[e];
            }
        } else {                                                    // rhs = -J^T W r
            V3<double> gr{0, 0, 0}, gp{0, 0, 0}, gv{0, 0, 0};
            if (k > 0) {
                gr = gr + ld3(a0 + 27); gp = gp + ld3(a0 + 30);
                gv = gv - w1_of(a0) * ld3(a0 + 33);
            }
            if (k < M) {
                const double dt = a1[39];
                gr = gr - ld3(a1 + 27); gp = gp - ld3(a1 + 30);
                gv = gv + w1_of(a1) * ld3(a1 + 33) - (w3_of(a1) * dt) * ld3(a1 + 36);
            }
            double* bb = oR + lane * 9;
            bb[0] = -gr.x; bb[1] = -gr.y; bb[2] = -gr.z; bb[3] = -gp.x; bb[4] = -gp.y; bb[5] = -gp.z;
            bb[6] = -gv.x; bb[7] = -gv.y; bb[8] = -gv.z;
        }
    }
    __syncthreads();
    const size_t node0 = (size_t)blk * LB_NODES;
    const int nHd = cnt * 81, nHo = min(cnt, M - blk * LB_NODES) * 81, nR = cnt * 9;
    for (int e = threadIdx.x; e < nHd; e += LB_THREADS) Hd[node0 * 81 + e] = oHd[e];
    for (int e = threadIdx.x; e < nHo; e += LB_THREADS) Ho[node0 * 81 + e] = oHo[e];
    for (int e = threadIdx.x; e < nR; e += LB_THREADS) rhs[node0 * 9 + e] = oR[e];
}

// ROBUST: wave 0 also forms s_k and c_k of the link's four factors in registers, sums rho into loss_part and hands c-scaled
// pieces (and c w1, c w3) to the node builders; the default instantiation is the plain least-squares kernel.
template <bool ROBUST>
__global__ __launch_bounds__(LB_THREADS) void linbuild_kernel(const double* __restrict__ nodes, const double* __restrict__ vels,
                                                               const double* __restrict__ poses, const double* __restrict__ drots,
                                                               const double* __restrict__ dtrans, const double* __restrict__ dvels,
                                                               const double* __restrict__ dts, int N, LinWeights W,
                                                               double* __restrict__ lin, double* __restrict__ loss_part,
                                                               double* __restrict__ Hd, double* __restrict__ Ho,
                                                               double* __restrict__ rhs, const double* __restrict__ red,
                                                               ReprojDev rp, Gate gate, RobustDev rb) {
    constexpr int REC = ROBUST ? LB_REC_ROBUST : LB_REC;
    __shared__ double sl[64][REC];
    extern __shared__ __attribute__((aligned(16))) double lb_out[];   // staged Hd (63x81) | Ho (63x81) | rhs (63x9)
    const int M = N - 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int blk = xcd_index(blockIdx.x, (N + LB_NODES - 1) / LB_NODES);
    if (blk < 0 || gate_closed(gate)) return;
    const int L = blk * LB_NODES - 1 + lane;                  // link handled by this lane (wave 0)
    if (wave == 0) {
        double sq = 0.0;
        if (L >= 0 && L < M && lane <= LB_NODES) {
            const SE3<double> Xi = se3_load(nodes + 7 * L), Xj = se3_load(nodes + 7 * (L + 1));
            const double dt = dts[L];
            const LinkRes r = link_residuals(Xi, Xj, ld3(vels + 3 * L), ld3(vels + 3 * (L + 1)), se3_load(poses + 7 * L),
                                             ld4(drots + 4 * L), ld3(dtrans + 3 * L), ld3(dvels + 3 * L), dt);
            M3<double> G, C, B;
            link_jacobians(r, G, C, B);
            const bool owns = lane > 0 || blk == 0;
            if constexpr (ROBUST) {
                double c[4];
                const double rho = robust_link(rb, r.erho, r.ephi, r.rv, r.er, r.rt, c);
                if (owns) sq = rho + (red ? red[(size_t)L * RP_REC + 27] : 0.0);
                const LinWeights Wl{W.w0 * c[0], W.w1 * c[1], W.w2 * c[2], W.w3 * c[3], W.vmin, W.vmax};
                link_emit(r, G, C, B, dt, L, M, owns, Wl, lin, sl[lane], red, rp, Xi);
                sl[lane][40] = Wl.w1;
                sl[lane][41] = Wl.w3;
            } else {
                if (owns) {
                    sq = dot(r.erho, r.erho) + dot(r.ephi, r.ephi) + dot(r.rv, r.rv) + dot(r.er, r.er) + dot(r.rt, r.rt);
                    if (red) sq += red[(size_t)L * RP_REC + 27];
                }
                link_emit(r, G, C, B, dt, L, M, owns, W, lin, sl[lane], red, rp, Xi);
            }
        }
        sq = wave_sum(sq);
        if (lane == 0) loss_part[blk] = sq;
    }
    __syncthreads();
    nodes_build_copy(sl, lb_out, blk, N, W, Hd, Ho, rhs);
}
