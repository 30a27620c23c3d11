// logmel_stream.hip -- the VGGish log-mel front end run on PCM chunks: int16 samples of S streams go into per-stream sample
// rings, every STFT row is computed once, when its last sample has arrived, into a per-stream log-mel ring, and examples are
// gathered from that ring (reference abaw5_pre_processing/base/vggish/vggish_input.py:84-98 and mel_features.py:21-49, run
// incrementally).
//
// State: a sample ring [S][Rs] int16 and a log-mel ring [S][Rm][64] fp32, Rs and Rm powers of two.  The device keeps no
// counters: the host knows how many samples, rows and examples each stream has and says in small int32 tables what a launch
// does.  Positions and row numbers travel unwrapped, modulo 2^30; every ring length divides 2^30, so a mask with R - 1 finds
// the slot.  One push is three launches on one HIP stream, in this order:
//
//   append    ring[s][(pos + i) & (Rs - 1)] = packed[offset + i], i < count, for every segment (s, pos, count, offset); a
//             segment with offset < 0 repeats the sample before its position instead (the edge padding at a stream's end)
//   rows      one block per new row (s, pos, row): the 400 samples at pos .. pos + 399 -> logmel_row (logmel_row.h, the body
//             of the offline kernel) -> melring[s][row & (Rm - 1)][0 .. 63]
//   examples  out[e][f][:] = melring[s][(start + f) & (Rm - 1)][:], f < win, for every example (s, start), in float4
//
// INVARIANT.  A row is a function of its 400 samples only and is computed by the one body the offline kernel runs, so the
// examples of a stream are the same bits as VGGish.wav_int16_to_examples of the whole signal under any chunking, any S and any
// number of ring wraps.
//
// The tables are data the entries cannot inspect, so they are never trusted with an address: a stream index is clamped into
// [0, S), a count into [0, max_count], every position is masked with its ring length and every read of the packed input is
// bounded by its length (a sample past the end reads as 0).  A wrong table gives wrong numbers, never an access outside a
// ring or outside the packed input.  No grid sync, no flags, no atomics, no scratch.
//
// RESAMPLED INPUT (PCM at any rate, any number of channels).  Two more rings stand in front: a mixed-input ring [S][Rin]
// float64 (the channel mean at the input rate) and, in place of the int16 sample ring, a 16 kHz ring [S][Rs] float64 (the
// resampler's output).  A push is then four launches:
//
//   mix-append  in[s][(pos + i) & (Rin - 1)] = rs_mix(packed frame offset + i), i < count; offset < 0 repeats the sample
//               before the position (the edge padding, now at the input rate)
//   resample    segment (s, n0, count, r0, pos of q0, lo, hi): output n0 + i sits at input q0 + (r0 + i M) / L; one thread per
//               output, 256 consecutive outputs of one segment per block, summed by resample_block (resample_row.h, the
//               body of the offline kernel) and written to ring[s][(n0 + i) & (Rs - 1)].  n0 M does not fit 32 bits over a
//               long stream, so the host hands over r0 = (n0 M) mod L and the ring position of q0 = (n0 M) div L and the
//               kernel advances from there in 64 bits.  Input q0 + k is a ring read only for lo <= k < hi, the stream's
//               valid inputs relative to q0; outside it is ZERO BY THE RANGE CHECK, never a ring read: after a wrap the
//               slots before the stream's first sample and after its last hold old samples.
//   rows        the rows kernel above, instantiated for the float64 ring (lm_sample(double))
//   examples    as above
//
// INVARIANT.  An output is a function of its T inputs only and is one chain of T multiply-adds in the order j = 0 .. T - 1 in
// the one body the offline kernel runs; the mixed sample is computed by the one rs_mix.  So the 16 kHz ring holds the bits
// ops.resample_pcm gives the padded whole signal, and the examples are those of wav_int16_to_examples(resample=...).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"
#include "logmel_row.h"
#include "resample_row.h"

namespace cer {

constexpr int LS_POS_BITS = 30;   // positions and row numbers are kept modulo 2^30

__device__ __forceinline__ int ls_stream(int s, int S) { return min(max(s, 0), S - 1); }
// Slot of position pos + d in a ring of R slots; unsigned, so that no table content can overflow the sum.
__device__ __forceinline__ size_t ls_slot(int pos, int d, int R) { return ((unsigned)pos + (unsigned)d) & (unsigned)(R - 1); }

// segments: [4][A] int32 = stream, position of the first sample, count, offset into `packed` (< 0: repeat).  Grid
// (ceil(max_count / 256), A).  A repeat segment reads the slot before its first and writes at most Rs - 1 slots after it, so
// it never overwrites what it reads.
__global__ void logmel_stream_append_kernel(const int16_t *__restrict__ packed, int packed_len,
                                            const int32_t *__restrict__ segments, int A, int max_count,
                                            int16_t *__restrict__ ring, int S, int Rs) {
    const int a = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = ls_stream(segments[a], S), pos = segments[A + a], off = segments[3 * A + a];
    const int count = min(max(segments[2 * A + a], 0), max_count);
    if (i >= count) return;
    int16_t *dst = ring + (size_t)s * Rs;
    int16_t v;
    if (off < 0) {
        v = dst[ls_slot(pos, -1, Rs)];
    } else {
        const long long src = (long long)off + i;
        v = src < packed_len ? packed[src] : (int16_t)0;
    }
    dst[ls_slot(pos, i, Rs)] = v;
}

// Sample n of the row that starts at unwrapped position pos of one stream's ring (int16 PCM, or float64 resampler output).
template <typename T>
struct ls_ring_sample {
    const T *ring;   // the stream's Rs slots
    int pos, Rs;
    __device__ __forceinline__ double operator()(int n) const { return lm_sample(ring[ls_slot(pos, n, Rs)]); }
};

// rows: [3][N] int32 = stream, position of the row's first sample, row number.  One block per row.
template <typename T>
__global__ __launch_bounds__(LM_THREADS) void logmel_stream_rows_kernel(const T *__restrict__ ring, int S, int Rs,
                                                                        const int32_t *__restrict__ rows, int N,
                                                                        const double *__restrict__ mel, float log_offset,
                                                                        float *__restrict__ melring, int Rm) {
    const int m = blockIdx.x;
    const int s = ls_stream(rows[m], S), pos = rows[N + m], row = rows[2 * N + m];
    const ls_ring_sample<T> sample = {ring + (size_t)s * Rs, pos, Rs};
    logmel_row(sample, mel, log_offset, melring + ((size_t)s * Rm + ls_slot(row, 0, Rm)) * LM_MEL);
}

// segments: [4][A] int32 = stream, position of the first new input sample, count, offset into `packed` in frames (< 0:
// repeat).  packed: packed_frames frames of C interleaved int16 channels.  Grid (ceil(max_count / 256), A).  As in the append
// kernel above, a repeat segment never overwrites the slot it reads (count <= max_count < Rin).
__global__ void resample_stream_append_kernel(const int16_t *__restrict__ packed, int packed_frames, int C,
                                              const int32_t *__restrict__ segments, int A, int max_count,
                                              double *__restrict__ ring, int S, int Rin) {
    const int a = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    const int s = ls_stream(segments[a], S), pos = segments[A + a], off = segments[3 * A + a];
    const int count = min(max(segments[2 * A + a], 0), max_count);
    if (i >= count) return;
    double *dst = ring + (size_t)s * Rin;
    double v;
    if (off < 0) {
        v = dst[ls_slot(pos, -1, Rin)];
    } else {
        const long long src = (long long)off + i;
        v = src < packed_frames ? rs_mix(packed + (size_t)src * C, C) : 0.0;
    }
    dst[ls_slot(pos, i, Rin)] = v;
}

// Input q0 + k of one stream: a read of its mixed-input ring for lo <= k < hi, zero outside.
struct rs_ring_input {
    const double *ring;   // the stream's Rin slots
    int pos, Rin;         // unwrapped position of q0
    long long lo, hi;
    __device__ __forceinline__ double operator()(long long k) const {
        // (unsigned)k is k modulo 2^32, and Rin divides 2^32: the mask finds the slot of pos + k for a negative k too
        return k >= lo && k < hi ? ring[((unsigned)pos + (unsigned)k) & (unsigned)(Rin - 1)] : 0.0;
    }
};

// segments: [7][A] int32 = stream, position n0 of the first output, count, r0, position of q0, lo, hi.  Grid
// (ceil(max_count / 256), A); a block past its segment's count leaves as a whole, before any barrier.  The valid range is cut
// to the Rin samples before hi, so no two inputs of a launch can share a slot whatever the table says.
__global__ __launch_bounds__(RS_BLOCK) void resample_stream_kernel(const double *__restrict__ in_ring, int S, int Rin,
                                                                   const int32_t *__restrict__ segments, int A, int max_count,
                                                                   const double *__restrict__ taps, int L, int M, int T,
                                                                   double *__restrict__ out_ring, int Rs) {
    const int a = blockIdx.y;
    const int s = ls_stream(segments[a], S), n0 = segments[A + a];
    const int count = min(max(segments[2 * A + a], 0), max_count);
    const long long i_first = (long long)blockIdx.x * RS_BLOCK;
    if (i_first >= count) return;
    const long long i_last = (i_first + RS_BLOCK < count ? i_first + RS_BLOCK : (long long)count) - 1;
    int r0 = segments[3 * A + a] % L;   // the tap row is (r0 + i M) mod L: in [0, L) for any table
    r0 = r0 < 0 ? r0 + L : r0;
    const long long hi = segments[6 * A + a], lo_t = segments[5 * A + a];
    const rs_ring_input input = {in_ring + (size_t)s * Rin, segments[4 * A + a], Rin, lo_t > hi - Rin ? lo_t : hi - Rin, hi};
    const double acc = resample_block(input, taps, L, M, T, r0, i_first, i_last);
    const long long i = i_first + threadIdx.x;
    if (i <= i_last) out_ring[(size_t)s * Rs + ls_slot(n0, (int)i, Rs)] = acc;
}

// examples: [2][E] int32 = stream, start row.  One thread per float4 of the output [E][win][64].
__global__ void logmel_stream_examples_kernel(const float4 *__restrict__ melring, int S, int Rm,
                                              const int32_t *__restrict__ examples, int E, int win,
                                              float4 *__restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)E * win * (LM_MEL / 4);
    if (idx >= total) return;
    const int c4 = (int)(idx % (LM_MEL / 4));
    const size_t t = idx / (LM_MEL / 4);
    const int f = (int)(t % win), e = (int)(t / win);
    const int s = ls_stream(examples[e], S), start = examples[E + e];
    out[idx] = melring[((size_t)s * Rm + ls_slot(start, f, Rm)) * (LM_MEL / 4) + c4];
}

// A power of two that divides 2^30 (so a position modulo 2^30 masks to the slot of the unwrapped position).
static bool ls_ring_len(int v) { return v > 0 && (v & (v - 1)) == 0 && v <= (1 << LS_POS_BITS); }
static bool ls_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

#define ST ((hipStream_t)stream)
#define LS_REFUSE(...) return cer_set_error(CER_ERR_INVALID_ARG, __VA_ARGS__)

}  // namespace cer

using namespace cer;

extern "C" int cer_logmel_stream_append(const int16_t *packed, int packed_len, const int32_t *segments, int num_segments,
                                        int max_count, int16_t *ring, int S, int Rs, void *stream) {
    if (!packed || !segments || !ring) LS_REFUSE("logmel_stream_append: null pointer");
    if (packed_len < 1 || num_segments < 1 || max_count < 1 || S < 1)
        LS_REFUSE("logmel_stream_append: packed length, segments, samples of a segment and streams must be >= 1");
    if (!ls_ring_len(Rs) || Rs < LM_WIN)
        LS_REFUSE("logmel_stream_append: ring length Rs = %d is not a power of two from 512 to 2^30", Rs);
    if (max_count >= Rs)
        LS_REFUSE("logmel_stream_append: %d new samples of a stream and the one before them exceed Rs = %d", max_count, Rs);
    if (num_segments > 65535) LS_REFUSE("logmel_stream_append: %d segments exceed the grid", num_segments);
    CER_LAUNCH(logmel_stream_append_kernel, dim3(cer_blocks((size_t)max_count, 256), num_segments), dim3(256), 0, ST, packed,
               packed_len, segments, num_segments, max_count, ring, S, Rs);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_logmel_stream_rows(const int16_t *ring, int S, int Rs, const int32_t *rows, int num_rows,
                                      const double *mel_matrix, float log_offset, float *logmel_ring, int Rm, void *stream) {
    if (!ring || !rows || !mel_matrix || !logmel_ring) LS_REFUSE("logmel_stream_rows: null pointer");
    if (S < 1 || num_rows < 1) LS_REFUSE("logmel_stream_rows: streams and rows must be >= 1");
    if (!ls_ring_len(Rs) || Rs < LM_WIN)
        LS_REFUSE("logmel_stream_rows: ring length Rs = %d is not a power of two from 512 to 2^30", Rs);
    if (!ls_ring_len(Rm)) LS_REFUSE("logmel_stream_rows: ring length Rm = %d is not a power of two up to 2^30", Rm);
    CER_LAUNCH(logmel_stream_rows_kernel<int16_t>, dim3(num_rows), dim3(LM_THREADS), 0, ST, ring, S, Rs, rows, num_rows, mel_matrix,
               log_offset, logmel_ring, Rm);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_logmel_stream_rows_f64(const double *ring, int S, int Rs, const int32_t *rows, int num_rows,
                                          const double *mel_matrix, float log_offset, float *logmel_ring, int Rm,
                                          void *stream) {
    if (!ring || !rows || !mel_matrix || !logmel_ring) LS_REFUSE("logmel_stream_rows_f64: null pointer");
    if (S < 1 || num_rows < 1) LS_REFUSE("logmel_stream_rows_f64: streams and rows must be >= 1");
    if (!ls_ring_len(Rs) || Rs < LM_WIN)
        LS_REFUSE("logmel_stream_rows_f64: ring length Rs = %d is not a power of two from 512 to 2^30", Rs);
    if (!ls_ring_len(Rm)) LS_REFUSE("logmel_stream_rows_f64: ring length Rm = %d is not a power of two up to 2^30", Rm);
    CER_LAUNCH(logmel_stream_rows_kernel<double>, dim3(num_rows), dim3(LM_THREADS), 0, ST, ring, S, Rs, rows, num_rows,
               mel_matrix, log_offset, logmel_ring, Rm);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_resample_stream_append(const int16_t *packed, int packed_frames, int channels, const int32_t *segments,
                                          int num_segments, int max_count, int history, double *in_ring, int S, int Rin,
                                          void *stream) {
    if (!packed || !segments || !in_ring) LS_REFUSE("resample_stream_append: null pointer");
    if (packed_frames < 1 || channels < 1 || num_segments < 1 || max_count < 1 || S < 1 || history < 0)
        LS_REFUSE("resample_stream_append: packed frames, channels, segments, frames of a segment and streams must be >= 1, "
                  "history >= 0");
    if (!ls_ring_len(Rin)) LS_REFUSE("resample_stream_append: ring length Rin = %d is not a power of two up to 2^30", Rin);
    if ((long long)history + max_count > Rin || max_count >= Rin)
        LS_REFUSE("resample_stream_append: %d old inputs and %d new ones of a stream exceed Rin = %d", history, max_count, Rin);
    if (num_segments > 65535) LS_REFUSE("resample_stream_append: %d segments exceed the grid", num_segments);
    CER_LAUNCH(resample_stream_append_kernel, dim3(cer_blocks((size_t)max_count, 256), num_segments), dim3(256), 0, ST, packed,
               packed_frames, channels, segments, num_segments, max_count, in_ring, S, Rin);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_resample_stream_outputs(const double *in_ring, int S, int Rin, const int32_t *segments, int num_segments,
                                           int max_count, const double *taps, int L, int M, int T, double *out_ring, int Rs,
                                           void *stream) {
    if (!in_ring || !segments || !taps || !out_ring) LS_REFUSE("resample_stream_outputs: null pointer");
    if (S < 1 || num_segments < 1 || max_count < 1)
        LS_REFUSE("resample_stream_outputs: streams, segments and outputs of a segment must be >= 1");
    if (L <= 0 || M <= 0) LS_REFUSE("resample_stream_outputs: L = %d and M = %d must be positive", L, M);
    if (T < 2 || (T & 1)) LS_REFUSE("resample_stream_outputs: T = %d taps per phase must be even and >= 2", T);
    if (!ls_ring_len(Rin) || Rin < T)
        LS_REFUSE("resample_stream_outputs: ring length Rin = %d is not a power of two from T = %d to 2^30", Rin, T);
    if (!ls_ring_len(Rs)) LS_REFUSE("resample_stream_outputs: ring length Rs = %d is not a power of two up to 2^30", Rs);
    if (max_count > Rs) LS_REFUSE("resample_stream_outputs: %d outputs of a stream exceed Rs = %d", max_count, Rs);
    // The kernel's 64-bit r0 + i M (r0 < L < 2^31, i < max_count <= 2^30) stays below 2^62 and its 32-bit quantities (an LDS
    // window's fill, a masked slot) do not grow with M / L; what grows is the run of inputs one block walks through.
    if ((long long)RS_BLOCK * M / L + T > (1 << 24))
        LS_REFUSE("resample_stream_outputs: a block of %d outputs would read %lld inputs (M / L = %d / %d, T = %d), more than "
                  "2^24", RS_BLOCK, (long long)RS_BLOCK * M / L + T, M, L, T);
    if (num_segments > 65535) LS_REFUSE("resample_stream_outputs: %d segments exceed the grid", num_segments);
    CER_LAUNCH(resample_stream_kernel, dim3(cer_blocks((size_t)max_count, RS_BLOCK), num_segments), dim3(RS_BLOCK), 0, ST,
               in_ring, S, Rin, segments, num_segments, max_count, taps, L, M, T, out_ring, Rs);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_logmel_stream_examples(const float *logmel_ring, int S, int Rm, const int32_t *examples, int num_examples,
                                          int win, float *out, void *stream) {
    if (!logmel_ring || !examples || !out) LS_REFUSE("logmel_stream_examples: null pointer");
    if (S < 1 || num_examples < 1 || win < 1) LS_REFUSE("logmel_stream_examples: streams, examples and win must be >= 1");
    if (!ls_ring_len(Rm)) LS_REFUSE("logmel_stream_examples: ring length Rm = %d is not a power of two up to 2^30", Rm);
    if (Rm < win) LS_REFUSE("logmel_stream_examples: an example of %d rows exceeds Rm = %d", win, Rm);
    if (!ls_al16(logmel_ring) || !ls_al16(out)) LS_REFUSE("logmel_stream_examples: the ring and the output must be 16-byte aligned");
    const size_t total = (size_t)num_examples * win * (LM_MEL / 4);
    if (total > (size_t)0x7fffffff * 256) LS_REFUSE("logmel_stream_examples: too many elements");
    CER_LAUNCH(logmel_stream_examples_kernel, dim3(cer_blocks(total, 256)), dim3(256), 0, ST, (const float4 *)logmel_ring, S, Rm,
               examples, num_examples, win, (float4 *)out);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
