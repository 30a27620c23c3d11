// feature_norm.hip -- the reference's per-component standardisation of the vggish and bert rows (base/dataset.py:516-539,
// transforms.Normalize(mean, std) around every modality but video and logmel; the statistics of base/dataset.py:272-325).
//
// feature_moments_kernel: acc[0][c] += sum_m x[m][c], acc[1][c] += sum_m x[m][c]^2, in float64.  One thread owns one column
// and walks the rows in ascending order; a wave reads 256 contiguous bytes of a row.  The sum of a column is a chain of float64
// adds whose order is the row order and nothing else: the block size, the grid, the unroll and the split of the rows over
// calls change no bit (the accumulator is read at the start of a call and written at its end, and the calls of a stream are
// ordered).  There is no atomic, no LDS and no reduction across threads.  x * x of two fp32 values has 48 significant bits and
// is exact in float64, so whether the compiler contracts acc + x * x into an FMA changes nothing either.  The price is
// parallelism: C threads in C / 64 waves, each with FM_UNROLL loads in flight; the pass is meant to run behind the encoder
// that made the rows (DESIGN.md section 9 has the measured times).
//
// standardize_rows_kernel: out = (x - mean) / std elementwise in float4, one IEEE subtraction and one correctly rounded IEEE
// division per element (hipcc's default for `/` on fp32: v_div_scale / v_div_fmas / v_div_fixup with denormals kept, not
// v_rcp times the numerator).  That is torch's tensor.sub_(mean).div_(std) bit for bit, subnormal quotients included.  out may
// be x: every element is read and written by the same thread.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"

namespace cer {

constexpr int FM_THREADS = 64, FM_UNROLL = 16, FM_MAX_C = 1 << 20;
constexpr int SR_THREADS = 256, SR_MAX_BLOCKS = 2048;

__global__ __launch_bounds__(FM_THREADS) void feature_moments_kernel(const float *__restrict__ rows, int M, int C,
                                                                     double *__restrict__ acc) {
    const int c = blockIdx.x * FM_THREADS + threadIdx.x;
    if (c >= C) return;
    double s1 = acc[c], s2 = acc[C + c];
    const float *p = rows + c;
    int m = 0;
    for (; m + FM_UNROLL <= M; m += FM_UNROLL) {
        float v[FM_UNROLL];
#pragma unroll
        for (int u = 0; u < FM_UNROLL; ++u) v[u] = p[(size_t)(m + u) * C];
#pragma unroll
        for (int u = 0; u < FM_UNROLL; ++u) {
            const double d = (double)v[u];
            s1 += d;
            s2 += d * d;
        }
    }
    for (; m < M; ++m) {
        const double d = (double)p[(size_t)m * C];
        s1 += d;
        s2 += d * d;
    }
    acc[c] = s1;
    acc[C + c] = s2;
}

__global__ __launch_bounds__(SR_THREADS) void standardize_rows_kernel(const float4 *x, int n4, int cols4,
                                                                      const float4 *__restrict__ mean,
                                                                      const float4 *__restrict__ std, float4 *out) {
    for (int i = blockIdx.x * SR_THREADS + threadIdx.x; i < n4; i += gridDim.x * SR_THREADS) {
        const int c = i % cols4;
        const float4 v = x[i], mu = mean[c], sd = std[c];
        float4 r;
        r.x = (v.x - mu.x) / sd.x;
        r.y = (v.y - mu.y) / sd.y;
        r.z = (v.z - mu.z) / sd.z;
        r.w = (v.w - mu.w) / sd.w;
        out[i] = r;
    }
}

}  // namespace cer

using namespace cer;

extern "C" int cer_feature_moments_update(const float *rows, int64_t M, int C, double *acc, void *stream) {
    if (!rows || !acc) return cer_set_error(CER_ERR_INVALID_ARG, "feature_moments_update: null pointer");
    if (M < 1) return cer_set_error(CER_ERR_INVALID_ARG, "feature_moments_update: M = %lld rows: must be >= 1", (long long)M);
    if (C < 1 || C > FM_MAX_C)
        return cer_set_error(CER_ERR_INVALID_ARG, "feature_moments_update: C = %d columns outside [1, %d]", C, FM_MAX_C);
    if (M > 0x7fffffffLL / C)
        return cer_set_error(CER_ERR_INVALID_ARG, "feature_moments_update: M * C = %lld * %d is not below 2^31", (long long)M, C);
    if (((uintptr_t)rows & 3) || ((uintptr_t)acc & 7))
        return cer_set_error(CER_ERR_INVALID_ARG, "feature_moments_update: rows must be 4-byte and acc 8-byte aligned");
    CER_LAUNCH(feature_moments_kernel, dim3(cer_blocks((size_t)C, FM_THREADS)), dim3(FM_THREADS), 0, (hipStream_t)stream, rows,
               (int)M, C, acc);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_standardize_rows(const float *x, int64_t M, int C, const float *mean, const float *std, float *out,
                                    void *stream) {
    if (!x || !mean || !std || !out) return cer_set_error(CER_ERR_INVALID_ARG, "standardize_rows: null pointer");
    if (M < 1) return cer_set_error(CER_ERR_INVALID_ARG, "standardize_rows: M = %lld rows: must be >= 1", (long long)M);
    if (C < 4 || C > FM_MAX_C || C % 4)
        return cer_set_error(CER_ERR_INVALID_ARG, "standardize_rows: C = %d columns: must be a multiple of 4 in [4, %d]", C,
                             FM_MAX_C);
    if (M > 0x7fffffffLL / C)
        return cer_set_error(CER_ERR_INVALID_ARG, "standardize_rows: M * C = %lld * %d is not below 2^31", (long long)M, C);
    if (((uintptr_t)x | (uintptr_t)mean | (uintptr_t)std | (uintptr_t)out) & 15)
        return cer_set_error(CER_ERR_INVALID_ARG, "standardize_rows: x, mean, std and out must be 16-byte aligned");
    const int n4 = (int)(M * C / 4);
    const unsigned blocks = cer_blocks((size_t)n4, SR_THREADS);
    CER_LAUNCH(standardize_rows_kernel, dim3(blocks < SR_MAX_BLOCKS ? blocks : SR_MAX_BLOCKS), dim3(SR_THREADS), 0,
               (hipStream_t)stream, reinterpret_cast<const float4 *>(x), n4, C / 4, reinterpret_cast<const float4 *>(mean),
               reinterpret_cast<const float4 *>(std), reinterpret_cast<float4 *>(out));
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
