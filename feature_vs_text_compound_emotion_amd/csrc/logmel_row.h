// logmel_row.h -- one row of the VGGish log-mel, shared by the offline kernels (encoders.hip) and the streaming kernel
// (logmel_stream.hip): 400 samples -> periodic Hann -> |512-point DFT| (257 bins, direct, LDS twiddle table) -> 257x64 mel
// product -> log(x + offset), float64 throughout and rounded to fp32 at the store.
//
// INVARIANT.  Everything that decides a bit of the row is here and here only: the window, the twiddles, the order of the sums
// over n and over k, the magnitude, the log and the rounding.  A caller supplies where sample n comes from (a functor that
// returns it as a double in [-1, 1)) and where the 64 floats go.  So a row computed from a ring is the same bits as the row the
// offline kernel computes from the same 400 samples.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cer {

constexpr int LM_WIN = 400, LM_HOP = 160, LM_FFT = 512, LM_BINS = 257, LM_MEL = 64;
constexpr int LM_THREADS = 256;

__device__ __forceinline__ double lm_sample(int16_t v) { return (double)v / 32768.0; }
__device__ __forceinline__ double lm_sample(double v) { return v; }   // already in [-1, 1): the resampler's output

// One block of LM_THREADS threads per row.  sample(n), 0 <= n < 400: the row's n-th sample; out_row: its 64 floats.
template <class Sample>
__device__ __forceinline__ void logmel_row(const Sample &sample, const double *__restrict__ mel, float log_offset,
                                           float *__restrict__ out_row) {
    __shared__ double xs[LM_WIN];
    __shared__ double cs[LM_FFT], sn[LM_FFT];
    __shared__ double mag[LM_BINS + 3];
    const int tid = threadIdx.x;
    for (int n = tid; n < LM_WIN; n += LM_THREADS) {
        const double w = 0.5 - 0.5 * cospi(2.0 * (double)n / (double)LM_WIN);
        xs[n] = sample(n) * w;
    }
    for (int j = tid; j < LM_FFT; j += LM_THREADS) {
        double s, c;
        sincospi(2.0 * (double)j / (double)LM_FFT, &s, &c);
        cs[j] = c;
        sn[j] = s;
    }
    __syncthreads();
    for (int k = tid; k < LM_BINS; k += LM_THREADS) {
        double re = 0.0, im = 0.0;
        for (int n = 0; n < LM_WIN; ++n) {
            const int j = (k * n) & (LM_FFT - 1);
            re += xs[n] * cs[j];
            im -= xs[n] * sn[j];
        }
        mag[k] = sqrt(re * re + im * im);
    }
    __syncthreads();
    if (tid < LM_MEL) {
        double acc = 0.0;
        for (int k = 0; k < LM_BINS; ++k) acc += mag[k] * mel[k * LM_MEL + tid];
        out_row[tid] = (float)log(acc + (double)log_offset);
    }
}

}  // namespace cer
