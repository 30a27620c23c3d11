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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"
#include "logmel_row.h"

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

// Sample n of the row that starts at unwrapped position pos of one stream's ring.
struct ls_ring_sample {
    const int16_t *ring;   // the stream's Rs slots
    int pos, Rs;
    __device__ __forceinline__ double operator()(int n) const { return lm_sample(ring[ls_slot(pos, n, Rs)]); }
};

// rows: [3][N] int32 = stream, position of the row's first sample, row number.  One block per row.
__global__ __launch_bounds__(LM_THREADS) void logmel_stream_rows_kernel(const int16_t *__restrict__ ring, int S, int Rs,
                                                                        const int32_t *__restrict__ rows, int N,
                                                                        const double *__restrict__ mel, float log_offset,
                                                                        float *__restrict__ melring, int Rm) {
    const int m = blockIdx.x;
    const int s = ls_stream(rows[m], S), pos = rows[N + m], row = rows[2 * N + m];
    const ls_ring_sample sample = {ring + (size_t)s * Rs, pos, Rs};
    logmel_row(sample, mel, log_offset, melring + ((size_t)s * Rm + ls_slot(row, 0, Rm)) * LM_MEL);
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
    CER_LAUNCH(logmel_stream_rows_kernel, dim3(num_rows), dim3(LM_THREADS), 0, ST, ring, S, Rs, rows, num_rows, mel_matrix,
               log_offset, logmel_ring, Rm);
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
