// The term sum of the closed-form IMU solves ("The shared term sum"): a pair kernel stores NT terms per pair
// by term (terms[q P + i]; a pair that takes no part stores zeros), and one workgroup adds them up in an order that depends on the
// number of pairs alone, so a second call gives the same bits.  More than REACH pairs: a partial-sum launch first, one workgroup per
// REACH pairs, and the solve kernel sums the partial sums the same way.  No atomics, no workgroup waits for another.  A solve of this
// family is a pair kernel, a thin __global__ around partial_sum<NT> and a solve kernel that starts with block_sum<NT>; on the host it is
// check_entry, then run_rounds with the three launches of its own: the rounds, the partial-sum launch and the status are run_rounds'.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"

namespace islam {
namespace tsum {

constexpr int BLOCK = 256;
constexpr int REACH = 4 * BLOCK;      // pairs one workgroup sums
constexpr int HEAD = 32;              // doubles in front of the terms: the two status words first, the rest is the solve's own
constexpr int EST = 4;                // the last round's estimate in the head (doubles 4 .. 7), behind the two status words

// tot[q] = sum over c in [c0, c1) of src[q ld + c], in an order that depends on c1 - c0 alone: lane-strided partial sums, a shuffle
// tree inside every wave, the four waves in order.  Ends on a barrier: every lane may read tot afterwards.
template <int NT>
__device__ __forceinline__ void block_sum(const double* __restrict__ src, size_t ld, size_t c0, size_t c1, double* wsum, double* tot) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = 0.0;
    for (size_t c = c0 + tid; c < c1; c += BLOCK)
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] += src[(size_t)q * ld + c];
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1)
#pragma unroll
        for (int q = 0; q < NT; ++q) acc[q] += __shfl_down(acc[q], sft, 64);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NT; ++q) wsum[wv * NT + q] = acc[q];
    __syncthreads();
    if (tid < NT) tot[tid] = ((wsum[tid] + wsum[NT + tid]) + wsum[2 * NT + tid]) + wsum[3 * NT + tid];
    __syncthreads();
}

// The body of a partial-sum kernel (grid = partial_blocks(P), block = BLOCK): partial[q nblocks + b] = the sum of block b's REACH pairs.
template <int NT>
__device__ __forceinline__ void partial_sum(const double* __restrict__ terms, int P, int nblocks, double* __restrict__ partial) {
    __shared__ double wsum[4 * NT], tot[NT];
    const size_t c0 = (size_t)blockIdx.x * REACH;
    const size_t c1 = c0 + REACH < (size_t)P ? c0 + REACH : (size_t)P;
    block_sum<NT>(terms, (size_t)P, c0, c1, wsum, tot);
    if (threadIdx.x < NT) partial[(size_t)threadIdx.x * nblocks + blockIdx.x] = tot[threadIdx.x];
}

inline int partial_blocks(int P) { return P > REACH ? (P + REACH - 1) / REACH : 0; }

// The scratch of a solve over P pairs of nt terms: HEAD doubles | terms (nt x P) | partial (nt x blocks).
struct Scratch {
    int* status;                      // two words at the front of the head: solve failed (0 / 1), pairs excluded
    double* head;
    double* est;                      // the last round's estimate, which the next round's pair kernel reweights by
    double* terms;
    double* partial;
    int blocks;                       // workgroups of the partial-sum launch, 0 = no such launch
    const double* src;                // what the solve kernel sums: the partial sums if there are any, else the terms
    int count;                        // their number, which is also their leading dimension

    Scratch(void* scratch, int nt, int P)
        : status(reinterpret_cast<int*>(scratch)), head(reinterpret_cast<double*>(scratch)), est(head + EST), terms(head + HEAD),
          partial(terms + (size_t)nt * P), blocks(partial_blocks(P)), src(blocks > 0 ? partial : terms), count(blocks > 0 ? blocks : P) {}

    static size_t bytes(int nt, int P) { return sizeof(double) * (HEAD + (size_t)nt * P + (size_t)nt * partial_blocks(P)); }
};

// The end of a solve call: the launch check, the two status words to the host, the stream drained.  ISLAM_OK, or the HIP error's code.
inline int read_status(const int* status, hipStream_t s, int (&host)[2]) {
    ISLAM_LAUNCH_CHECK();
    host[0] = host[1] = 0;
    ISLAM_HIP_CHECK(hipMemcpyAsync(host, status, sizeof(host), hipMemcpyDeviceToHost, s));
    ISLAM_HIP_CHECK(hipStreamSynchronize(s));
    return ISLAM_OK;
}

// What the entry points of the family check alike, under the entry point's name; one that has no Huber rounds leaves delta and rounds out.
inline int check_entry(const char* name, int rows, int dtype, double delta = 0.0, int rounds = 0) {
    if (rows < 0) return fail(ISLAM_EARG, "%s: rows=%d", name, rows);
    if (dtype != ISLAM_F64 && dtype != ISLAM_F32) return fail(ISLAM_EARG, "%s: dtype %d", name, dtype);
    if (!(delta >= 0.0) || !std::isfinite(delta))
        return fail(ISLAM_EARG, "%s: delta %g (0 = no reweighting, > 0 = the Huber threshold in rad)", name, delta);
    if (rounds < 0) return fail(ISLAM_EARG, "%s: rounds=%d", name, rounds);
    return ISLAM_OK;
}

// The launches of a solve over P pairs and the end of its call.  The first solve and, with delta > 0, `rounds` reweighted ones; every
// round is row(prev) (the pair kernel; prev = the estimate of the round before in the scratch head, NULL in the first), the partial-sum
// kernel `partial` when there are more than REACH pairs, and solve(first, last) (the one-workgroup solve kernel).  tail() enqueues
// what reads the final estimate (residuals, velocities), under its own condition.  Returns the number of excluded pairs, not_pd(excluded)
// (the solve's own ISLAM_ENOTPD message) when the solve kernel reports a failure, or the HIP error's code.
template <class Row, class Solve, class Tail, class NotPd>
int run_rounds(const Scratch& sc, int P, void (*partial)(const double*, int, int, double*), double delta, int rounds, hipStream_t s, Row row,
               Solve solve, Tail tail, NotPd not_pd) {
    const int K = delta > 0.0 ? rounds : 0;
    for (int r = 0; r <= K; ++r) {
        if (P > 0) row(r > 0 ? (const double*)sc.est : (const double*)nullptr);
        if (sc.blocks > 0) hipLaunchKernelGGL(partial, dim3(sc.blocks), dim3(BLOCK), 0, s, (const double*)sc.terms, P, sc.blocks, sc.partial);
        solve(r == 0 ? 1 : 0, r == K ? 1 : 0);
    }
    tail();
    int host[2];
    if (const int rc = read_status(sc.status, s, host)) return rc;
    return host[0] != 0 ? not_pd(host[1]) : host[1];
}

}  // namespace tsum
}  // namespace islam
