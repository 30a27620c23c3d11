// resample_row.h -- the polyphase sum of the PCM resampler, shared by the offline kernel (encoders.hip) and the streaming
// kernels (logmel_stream.hip):
//
//   out[i] = sum_j taps[r][j] * x[q - J + j],   q = (r0 + i M) div L,   r = (r0 + i M) mod L,   J = (T - 2) / 2
//
// where x is the channel mean of the int16 PCM / 32768 at the input rate.  Float64 throughout.
//
// INVARIANT.  Everything that decides a bit of an output is here and here only: the channel mix (sum over the channels of
// p[ch] / 32768.0, then / C, in that order), the fill of the block's RS_WIN-sample LDS window, and the accumulation
// acc += taps[r][j] * x[q - J + j] in the order j = 0 .. T - 1 across the windows.  A caller supplies where input sample k
// comes from (a functor that returns it as a double, zero where the signal has none) and where the output goes.  So an output
// computed from a ring of mixed samples is the same bits as the one the offline kernel computes from the same PCM, however
// the outputs are split over blocks and windows: every output is one chain of T multiply-adds in one order.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace cer {

constexpr int RS_BLOCK = 256, RS_WIN = 2048;

// One input-rate sample: the mean of the C interleaved channels at p, in [-1, 1).
__device__ __forceinline__ double rs_mix(const int16_t *__restrict__ p, int C) {
    double v = 0.0;
    for (int ch = 0; ch < C; ++ch) v += (double)p[ch] / 32768.0;
    v /= (double)C;
    return v;
}

// One block of RS_BLOCK threads computes outputs i_first .. i_last (at most RS_BLOCK of them) of one signal; thread t returns
// output i_first + t (threads past i_last shadow the last output; the caller stores nothing for them).  input(k): input sample
// k on the axis on which output i sits at (r0 + i M) / L.  The block's outputs read one contiguous run of inputs; it goes
// through LDS RS_WIN samples at a time, so the LDS need does not grow with M / L or T, and every thread still adds its taps in
// the order j = 0 .. T - 1.  Every thread of the block must call this (it holds barriers).
template <class Input>
__device__ __forceinline__ double resample_block(const Input &input, const double *__restrict__ taps, int L, int M, int T,
                                                 long long r0, long long i_first, long long i_last) {
    __shared__ double xs[RS_WIN];
    const int tid = threadIdx.x;
    const long long n = i_first + tid;
    const long long nl = n <= i_last ? n : i_last;
    const long long J = (T - 2) / 2;
    const long long k0 = (r0 + i_first * M) / L - J;                 // first input the block reads
    const long long span = (r0 + i_last * M) / L - J + T - k0;       // ... and how many
    const long long d = (r0 + nl * M) / L - J - k0;                  // this thread's first input, relative to k0
    const double *row = taps + (size_t)((r0 + nl * M) % L) * T;
    double acc = 0.0;
    for (long long w = 0; w < span; w += RS_WIN) {
        const int fill = (int)(span - w < RS_WIN ? span - w : RS_WIN);
        for (int i = tid; i < fill; i += RS_BLOCK) xs[i] = input(k0 + w + i);
        __syncthreads();
        const long long j_lo = w > d ? w - d : 0, j_hi = w + fill - d < T ? w + fill - d : T;
        for (long long j = j_lo; j < j_hi; ++j) acc += row[j] * xs[d + j - w];
        __syncthreads();
    }
    return acc;
}

}  // namespace cer
