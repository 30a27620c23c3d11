// encoders.hip -- front ends of the audio and text encoders.
//
//  * log-mel: int16 PCM -> /32768 -> edge pad -> 400-sample periodic-Hann frames (hop 160) ->
//    |512-point DFT| -> 257x64 HTK mel matrix -> log(x + 0.01)
//    (reference abaw5_pre_processing/base/vggish/mel_features.py:75-114,207-236,
//     vggish_input.py:84-98).  The reference computes this in float64 numpy; the kernel keeps
//    float64 for the DFT and the mel product (MI355X has a full-rate fp64 vector pipe and the
//    whole front end is ~11 MFLOP per clip), and rounds to fp32 only at the output, exactly
//    where the reference casts for the VGGish input.
//  * resampling: interleaved int16 PCM at any rate -> channel mean -> edge pad -> band-limited sinc interpolation to
//    16 kHz through a host-built polyphase tap table (what resampy.resample does for the reference,
//    vggish_input.py:51-56), float64 throughout; its output feeds the float64 instantiation of the log-mel.
//  * example framing: gather 96-frame windows at host-computed start rows (the reference's
//    fractional hop uses Python's round-half-to-even, vggish_input.py:77-81 / my_frame).
//  * BERT embeddings: word + position + token-type gather fused with LayerNorm(eps 1e-12).
#include <math.h>

#include "cer_internal.h"
#include "logmel_row.h"
#include "resample_row.h"

namespace cer {

// Sample n of frame `frame` of one clip, with np.pad(..., 'edge') read by clamping the index.
template <typename T>
struct lm_clip_sample {
    const T *src;   // the clip's num_samples samples
    int first, num_samples;
    __device__ __forceinline__ double operator()(int n) const {
        int idx = first + n;
        idx = idx < num_samples ? idx : num_samples - 1;
        return lm_sample(src[idx]);
    }
};

// One block per STFT frame; the row itself is logmel_row (logmel_row.h), shared with the streaming kernel.
template <typename T>
__global__ __launch_bounds__(LM_THREADS) void logmel_kernel(const T *__restrict__ pcm, int num_samples, int frames_per_clip,
                                                            const double *__restrict__ mel, float log_offset,
                                                            float *__restrict__ out) {
    const int clip = blockIdx.y, frame = blockIdx.x;
    const lm_clip_sample<T> sample = {pcm + (size_t)clip * num_samples, frame * LM_HOP, num_samples};
    logmel_row(sample, mel, log_offset, out + ((size_t)clip * frames_per_clip + frame) * LM_MEL);
}

// Input sample k of one clip: the channel mean (rs_mix) for 0 <= k < S, the last of those for S <= k < S + pad (np.pad 'edge',
// read by clamping the index like logmel_kernel) and zero outside.
struct rs_clip_input {
    const int16_t *src;   // the clip's S frames of C interleaved channels
    int S, C;
    long long padded;     // S + pad
    __device__ __forceinline__ double operator()(long long k) const {
        if (k < 0 || k >= padded) return 0.0;
        return rs_mix(src + (size_t)(k < S ? k : S - 1) * C, C);
    }
};

// out[c][n] = sum_j taps[r][j] * x[c][q - J + j] with q = (n M) div L, r = (n M) mod L, J = (T - 2) / 2, x as rs_clip_input
// has it.  One thread per output, 256 consecutive outputs per block; the sum itself is resample_block (resample_row.h),
// shared with the streaming kernel.
__global__ __launch_bounds__(RS_BLOCK) void resample_pcm_kernel(const int16_t *__restrict__ pcm, int S, int C, int pad,
                                                                const double *__restrict__ taps, int L, int M, int T,
                                                                int n_out, double *__restrict__ out) {
    const int clip = blockIdx.y;
    const long long n_first = (long long)blockIdx.x * RS_BLOCK;
    const long long n_last = (n_first + RS_BLOCK < n_out ? n_first + RS_BLOCK : (long long)n_out) - 1;
    const long long n = n_first + threadIdx.x;
    const rs_clip_input input = {pcm + (size_t)clip * S * C, S, C, (long long)S + pad};
    const double acc = resample_block(input, taps, L, M, T, 0, n_first, n_last);
    if (n <= n_last) out[(size_t)clip * n_out + n] = acc;
}

// examples[c][e][f][:] = logmel[c][starts[e] + f][:]
__global__ void frame_examples_kernel(const float4 *__restrict__ logmel, const int *__restrict__ starts,
                                      float4 *__restrict__ out, int clips, int frames_per_clip, int n_examples,
                                      int win) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)clips * n_examples * win * (LM_MEL / 4);
    if (idx >= total) return;
    const int c4 = (int)(idx % (LM_MEL / 4));
    size_t t = idx / (LM_MEL / 4);
    const int f = (int)(t % win); t /= win;
    const int e = (int)(t % n_examples);
    const int c = (int)(t / n_examples);
    out[idx] = logmel[((size_t)c * frames_per_clip + starts[e] + f) * (LM_MEL / 4) + c4];
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave per token: e = word[id] + pos[p] + type[tt]; y = LN(e) * gamma + beta.
__global__ void bert_embed_ln_kernel(const long long *__restrict__ ids, const float *__restrict__ word,
                                     const float *__restrict__ pos, const float *__restrict__ type,
                                     const float *__restrict__ gamma, const float *__restrict__ beta,
                                     float *__restrict__ y, int tokens, int S, int Hd, int vocab, float eps) {
    const int tok = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tok >= tokens) return;
    long long id = ids[tok];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const float *w = word + (size_t)id * Hd, *pp = pos + (size_t)(tok % S) * Hd;
    float s = 0.f;
    for (int c = lane; c < Hd; c += 64) s += w[c] + pp[c] + type[c];
    const float mu = wave_sum_f(s) / (float)Hd;
    s = 0.f;
    for (int c = lane; c < Hd; c += 64) { const float d = w[c] + pp[c] + type[c] - mu; s += d * d; }
    const float rstd = rsqrtf(wave_sum_f(s) / (float)Hd + eps);
    for (int c = lane; c < Hd; c += 64) y[(size_t)tok * Hd + c] = (w[c] + pp[c] + type[c] - mu) * rstd * gamma[c] + beta[c];
}

__global__ void add_inplace_kernel(float4 *__restrict__ y, const float4 *__restrict__ x, size_t n4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 a = y[i], b = x[i];
    y[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

}  // namespace cer

using namespace cer;

extern "C" int cer_logmel_num_frames(int num_samples, int pad_samples) {
    const long long n = (long long)num_samples + pad_samples;
    return n < LM_WIN ? 0 : (int)(1 + (n - LM_WIN) / LM_HOP);
}

extern "C" int cer_logmel_fwd(const int16_t *pcm, int clips, int num_samples, int pad_samples, const double *mel_matrix,
                              float log_offset, float *logmel, void *stream) {
    const int frames = cer_logmel_num_frames(num_samples, pad_samples);
    if (!pcm || !mel_matrix || !logmel || clips <= 0 || num_samples <= 0 || pad_samples < 0 || frames <= 0)
        return cer_set_error(CER_ERR_INVALID_ARG, "logmel_fwd: bad argument (need at least 400 samples incl. padding)");
    CER_LAUNCH(logmel_kernel<int16_t>, dim3(frames, clips), dim3(LM_THREADS), 0, (hipStream_t)stream, pcm, num_samples, frames,
               mel_matrix, log_offset, logmel);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_logmel_f64_fwd(const double *samples, int clips, int num_samples, const double *mel_matrix,
                                  float log_offset, float *logmel, void *stream) {
    const int frames = cer_logmel_num_frames(num_samples, 0);
    if (!samples || !mel_matrix || !logmel || clips <= 0 || clips > 65535 || num_samples <= 0 || frames <= 0)
        return cer_set_error(CER_ERR_INVALID_ARG, "logmel_f64_fwd: bad argument (need at least 400 samples, <= 65535 clips)");
    CER_LAUNCH(logmel_kernel<double>, dim3(frames, clips), dim3(LM_THREADS), 0, (hipStream_t)stream, samples, num_samples, frames,
               mel_matrix, log_offset, logmel);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_resample_pcm(const int16_t *pcm, int clips, int num_samples, int channels, int pad_samples,
                                const double *taps, int L, int M, int T, int n_out, double *out, void *stream) {
    if (!pcm || !taps || !out || clips <= 0 || clips > 65535 || num_samples <= 0 || channels <= 0 || pad_samples < 0 ||
        L <= 0 || M <= 0 || T < 2 || (T & 1) || n_out <= 0)
        return cer_set_error(CER_ERR_INVALID_ARG, "resample_pcm: bad argument (taps [L][T] with T even, <= 65535 clips)");
    CER_LAUNCH(resample_pcm_kernel, dim3(cer_blocks((size_t)n_out, RS_BLOCK), clips), dim3(RS_BLOCK), 0, (hipStream_t)stream,
               pcm, num_samples, channels, pad_samples, taps, L, M, T, n_out, out);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_frame_examples(const float *logmel, const int *starts, float *examples, int clips, int frames_per_clip,
                                  int n_examples, int win, void *stream) {
    if (!logmel || !starts || !examples || clips <= 0 || frames_per_clip <= 0 || n_examples <= 0 || win <= 0)
        return cer_set_error(CER_ERR_INVALID_ARG, "frame_examples: bad argument");
    const size_t total = (size_t)clips * n_examples * win * (LM_MEL / 4);
    CER_LAUNCH(frame_examples_kernel, dim3(cer_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, (const float4 *)logmel,
               starts, (float4 *)examples, clips, frames_per_clip, n_examples, win);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_bert_embed_ln(const long long *ids, const float *word, const float *pos, const float *type,
                                 const float *gamma, const float *beta, float *y, int B, int S, int Hd, int vocab,
                                 int max_pos, float eps, void *stream) {
    if (!ids || !word || !pos || !type || !gamma || !beta || !y || B <= 0 || S <= 0 || Hd <= 0 || vocab <= 0)
        return cer_set_error(CER_ERR_INVALID_ARG, "bert_embed_ln: bad argument");
    if (S > max_pos) return cer_set_error(CER_ERR_INVALID_ARG, "bert_embed_ln: sequence longer than the position table");
    const int tokens = B * S;
    CER_LAUNCH(bert_embed_ln_kernel, dim3((tokens + 3) / 4), dim3(256), 0, (hipStream_t)stream, ids, word, pos, type, gamma,
               beta, y, tokens, S, Hd, vocab, eps);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_add_inplace(float *y, const float *x, size_t n, void *stream) {
    if (!y || !x || n == 0 || (n & 3)) return cer_set_error(CER_ERR_INVALID_ARG, "add_inplace: n must be a positive multiple of 4");
    CER_LAUNCH(add_inplace_kernel, dim3(cer_blocks(n / 4, 256)), dim3(256), 0, (hipStream_t)stream, (float4 *)y,
               (const float4 *)x, n / 4);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
