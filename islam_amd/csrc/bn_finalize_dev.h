// The train-mode BatchNorm finaliser, once: per-block partial sums [nrows][2][C] (sum, sum of squares per channel) -> [scale | shift] and
// the running statistics of nn.BatchNorm2d.  One workgroup of THREADS threads = (THREADS / C) slices of the rows x C channels
// (C <= 256); a slice walks its rows in groups of four (four independent loads in flight per accumulator pair), slices are combined in
// slice order in double: deterministic, and the same bits for every kernel that calls it -- conv_mfma.hip's bn_finalize_kernel and
// conv_nhwc.hip's fold_finalize_kernel / finalize_rows_kernel, which differ only in how a row value is fetched.
#pragma once
#include <hip/hip_runtime.h>

namespace islam {

// row(b, j, c): the float at [b + j / 2][j % 2][c], j = 0 .. 7 -- the j-th value of the group of four rows that starts at row b (given as
// base and offset so that a plain load can form its address as ((size_t)b * 2 + j) * C + c, one 64-bit base per group).  Every thread of the workgroup calls this (it contains a barrier).  num_batches_tracked
// and anything a kernel does around the finalisation stay with the kernel.
template <int THREADS, class Row>
__device__ __forceinline__ void bn_finalize_block(Row&& row, int nrows, int C, double count, const float* weight, const float* bias,
                                                  float* running_mean, float* running_var, double momentum, double eps, float* scale_shift) {
    __shared__ double ls[THREADS], lq[THREADS];
    const int nsl = THREADS / C, c = threadIdx.x % C, sl = threadIdx.x / C;
    double s = 0.0, q = 0.0;
    if (sl < nsl) {
        const int per = (nrows + nsl - 1) / nsl, b0 = sl * per, b1 = min(nrows, b0 + per);
        int b = b0;
        for (; b + 4 <= b1; b += 4) {
            const float s0 = row(b, 0, c), q0 = row(b, 1, c), s1 = row(b, 2, c), q1 = row(b, 3, c);
            const float s2 = row(b, 4, c), q2 = row(b, 5, c), s3 = row(b, 6, c), q3 = row(b, 7, c);
            s += ((double)s0 + (double)s1) + ((double)s2 + (double)s3);
            q += ((double)q0 + (double)q1) + ((double)q2 + (double)q3);
        }
        for (; b < b1; ++b) {
            s += (double)row(b, 0, c);
            q += (double)row(b, 1, c);
        }
    }
    ls[threadIdx.x] = s;
    lq[threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x < C) {
        s = 0.0;
        q = 0.0;
        for (int k = 0; k < nsl; ++k) { s += ls[k * C + c]; q += lq[k * C + c]; }
        const double mean = s / count;
        const double var = fmax(q / count - mean * mean, 0.0);
        const double sc = (double)weight[c] / sqrt(var + eps);
        scale_shift[c] = (float)sc;
        scale_shift[C + c] = (float)((double)bias[c] - mean * sc);
        if (running_mean) {
            const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
            running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
            running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unb);
        }
    }
}

}  // namespace islam
