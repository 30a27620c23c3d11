// regression.hip -- the REGRESSION task on the device: the tanh output of the models, the reference's CCCLoss
// (base/loss_function.py:6-24) with its gradient, and the per-video moments behind RMSE / Pearson's r / Lin's CCC
// (base/logger.py:213-246,314-351).
//
// Everything here is a few 10^4 elements at most, so the arithmetic is double throughout: the only fp32 rounding is the one
// that stores a result.  Every sum has a fixed shape (strided partials per thread, __shfl_down over the 64 lanes of a wave,
// then a fixed tree over the block's four waves in LDS), so two calls on the same input give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"

namespace cer {

constexpr int REG_THREADS = 256, REG_WAVES = REG_THREADS / 64;

// Sum of v[k] over the block's 256 threads, for K values at once; every thread returns with the totals in v.
// `lds` holds K * REG_WAVES doubles and may be reused right after the call.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
        if (lane == 0) lds[k * REG_WAVES + wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double *w = lds + k * REG_WAVES;
        v[k] = (w[0] + w[1]) + (w[2] + w[3]);
    }
    __syncthreads();
}

__global__ void tanh_fwd_kernel(const float *__restrict__ x, float *__restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    // |x| >= 20: 1 - tanh(x) < 2^-56, so the double result is already 1; written out so that it does not hang on libm
    y[i] = fabsf(v) >= 20.f ? copysignf(1.f, v) : (float)tanh((double)v);
}

__global__ void tanh_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ y, float *__restrict__ dx, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double t = (double)y[i];
    dx[i] = (float)((double)dy[i] * (1.0 - t * t));
}

// One block per column (b, d) of gold / pred [B][L][D]: element j sits at ((b * L + j) * D + d).
__global__ __launch_bounds__(REG_THREADS) void ccc_column_kernel(const float *__restrict__ gold, const float *__restrict__ pred,
                                                                 float *__restrict__ dpred, double *__restrict__ col_ws, int L,
                                                                 int D, double N) {
    __shared__ double lds[3 * REG_WAVES];
    const int col = blockIdx.x, b = col / D, d = col - b * D, tid = threadIdx.x;
    const size_t base = (size_t)b * L * D + d;
    const double n = (double)L;
    double s[2] = {0.0, 0.0};
    for (int j = tid; j < L; j += REG_THREADS) {
        const size_t i = base + (size_t)j * D;
        s[0] += (double)gold[i];
        s[1] += (double)pred[i];
    }
    block_sum<2>(s, lds);
    const double gm = s[0] / n, pm = s[1] / n;
    double c[3] = {0.0, 0.0, 0.0};
    for (int j = tid; j < L; j += REG_THREADS) {
        const size_t i = base + (size_t)j * D;
        const double dg = (double)gold[i] - gm, dp = (double)pred[i] - pm;
        c[0] += dg * dp;
        c[1] += dg * dg;
        c[2] += dp * dp;
    }
    block_sum<3>(c, lds);
    const double S = c[0], m = gm - pm;
    const double Q = c[1] / (n - 1.0) + c[2] / (n - 1.0) + m * m;   // L = 1: 0 / 0, NaN like torch.var(unbiased=True)
    if (tid == 0) col_ws[col] = n - 2.0 * S / Q;
    if (!dpred) return;
    const double k = 2.0 * S / (Q * Q);
    for (int j = tid; j < L; j += REG_THREADS) {
        const size_t i = base + (size_t)j * D;
        const double dg = (double)gold[i] - gm, dp = (double)pred[i] - pm;
        dpred[i] = (float)((-2.0 * dg / Q + k * (2.0 * dp / (n - 1.0) - 2.0 * m / n)) / N);
    }
}

// The column terms in index order (B * D of them: tens), then the mean.
__global__ void ccc_finish_kernel(const double *__restrict__ col_ws, int cols, double N, float *__restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (int c = 0; c < cols; ++c) s += col_ws[c];
    *loss = (float)(s / N);
}

// One block per video: rows [off[v], off[v+1]) of pred / label.
__global__ __launch_bounds__(REG_THREADS) void regression_moments_kernel(const float *__restrict__ pred,
                                                                         const float *__restrict__ label,
                                                                         const int *__restrict__ off,
                                                                         double *__restrict__ moments) {
    __shared__ double lds[4 * REG_WAVES];
    const int v = blockIdx.x, r0 = off[v], r1 = off[v + 1], tid = threadIdx.x;
    const double n = (double)(r1 - r0);
    double s[2] = {0.0, 0.0};
    for (int r = r0 + tid; r < r1; r += REG_THREADS) {
        s[0] += (double)pred[r];
        s[1] += (double)label[r];
    }
    block_sum<2>(s, lds);
    const double pm = s[0] / n, lm = s[1] / n;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = r0 + tid; r < r1; r += REG_THREADS) {
        const double p = (double)pred[r], l = (double)label[r];
        const double dp = p - pm, dl = l - lm, e = p - l;
        c[0] += dp * dp;
        c[1] += dl * dl;
        c[2] += dp * dl;
        c[3] += e * e;
    }
    block_sum<4>(c, lds);
    if (tid != 0) return;
    double *o = moments + (size_t)v * 8;
    o[0] = n; o[1] = pm; o[2] = lm; o[3] = c[0]; o[4] = c[1]; o[5] = c[2]; o[6] = c[3]; o[7] = 0.0;
}

}  // namespace cer

using namespace cer;

#define ST ((hipStream_t)stream)

extern "C" int cer_tanh_fwd(const float *x, float *y, size_t n, void *stream) {
    if (!x || !y || n == 0) return cer_set_error(CER_ERR_INVALID_ARG, "tanh_fwd: bad argument");
    CER_LAUNCH(tanh_fwd_kernel, dim3(cer_blocks(n, 256)), dim3(256), 0, ST, x, y, n);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_tanh_bwd(const float *dy, const float *y, float *dx, size_t n, void *stream) {
    if (!dy || !y || !dx || n == 0) return cer_set_error(CER_ERR_INVALID_ARG, "tanh_bwd: bad argument");
    CER_LAUNCH(tanh_bwd_kernel, dim3(cer_blocks(n, 256)), dim3(256), 0, ST, dy, y, dx, n);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_ccc_loss(const float *gold, const float *pred, float *loss, float *dpred, double *col_ws, int B, int L, int D,
                            void *stream) {
    if (!gold || !pred || !loss || !col_ws || B <= 0 || L <= 0 || D <= 0)
        return cer_set_error(CER_ERR_INVALID_ARG, "ccc_loss: bad argument");
    if ((long long)B * D > 0x7fffffffLL) return cer_set_error(CER_ERR_INVALID_ARG, "ccc_loss: B * D exceeds the grid");
    const double N = (double)B * (double)L * (double)D;
    CER_LAUNCH(ccc_column_kernel, dim3(B * D), dim3(REG_THREADS), 0, ST, gold, pred, dpred, col_ws, L, D, N);
    CER_HIP_CHECK(hipGetLastError());
    CER_LAUNCH(ccc_finish_kernel, dim3(1), dim3(64), 0, ST, col_ws, B * D, N, loss);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_regression_moments(const float *pred, const float *label, const int *video_offsets, int V, int R,
                                      double *moments, void *stream) {
    if (!pred || !label || !video_offsets || !moments || V <= 0 || R < V)
        return cer_set_error(CER_ERR_INVALID_ARG, "regression_moments: bad argument");
    CER_LAUNCH(regression_moments_kernel, dim3(V), dim3(REG_THREADS), 0, ST, pred, label, video_offsets, moments);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
