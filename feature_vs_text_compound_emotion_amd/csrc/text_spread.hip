// text_spread.hip -- token rows of one or more sentences -> the rows of spans of frames (reference
// abaw5_pre_processing/base/speech.py:690-738, align_word_embedding_new: the frames of a span are divided into n = min(tokens,
// frames) contiguous blocks, the first frames % n of them one frame longer, and every frame of block j shows token j).
//
// A launch takes G segments (out_first, n_frames, n_tokens, index_first) and an index table: frame i of a segment is output
// row out_first + i and copies token row tok_index[index_first + j(i)], or is zeros when the segment has no token.  It is a
// pure row copy: one wave moves one output row in float4 (3 KiB at hidden = 768, three float4 per lane), the segment, the
// block j and the source row are the same for every lane of a wave, there is no LDS, no atomic and no wait between
// workgroups, and an output row has exactly one writer when the host keeps the segments' ranges disjoint.
//
// Grid.  blockIdx.x is the segment; the TSP_WAVES waves of the gridDim.y blocks of a segment stride over its frames and
// leave when they are past n_frames.  The alternative, a binary search over a prefix sum of the frame counts (what
// cer_window_stitch_multi does over its frame offsets), needs a sorted table that the entry would have to trust and a total
// row count that it cannot read from device memory; here no launch dimension and no address depends on the tables' content.
// gridDim.y comes from out_rows (no segment has more frames than that inside the output), capped, so short segments cost
// a few blocks that return after one 16-byte load.
//
// The two tables are data the host code cannot see at launch.  They never become an address unchecked: an output row outside
// [0, out_rows) is skipped, the index position is clamped into [0, n_index) and the token row into [0, tok_rows).  A wrong
// table gives wrong rows, never an access outside the three buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"

namespace cer {

constexpr int TSP_THREADS = 256, TSP_WAVES = TSP_THREADS / 64, TSP_MAX_Y = 64;

__global__ __launch_bounds__(TSP_THREADS) void text_spread_rows_kernel(const float4 *__restrict__ tok, long long tok_rows, int cols4,
                                                                       const int4 *__restrict__ segments,
                                                                       const int *__restrict__ tok_index, int n_index,
                                                                       float4 *__restrict__ out, long long out_rows) {
    const int4 seg = segments[blockIdx.x];   // out_first, n_frames, n_tokens, index_first
    const int n_frames = seg.y, n = min(seg.z, n_frames);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long q = 1, r = 0;
    if (n > 0) {
        q = n_frames / n;
        r = n_frames - q * n;
    }
    const long long split = r * (q + 1);   // frames of the r longer blocks; <= n_frames
    // the frames of this segment whose output row lies in [0, out_rows): [lo, hi)
    const long long lo = max(-(long long)seg.x, 0LL), hi = min((long long)n_frames, out_rows - (long long)seg.x);
    for (long long i = lo + (long long)blockIdx.y * TSP_WAVES + wave; i < hi; i += (long long)gridDim.y * TSP_WAVES) {
        float4 *dst = out + (size_t)((long long)seg.x + i) * cols4;
        if (n <= 0) {
            for (int c = lane; c < cols4; c += 64) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const long long j = i < split ? i / (q + 1) : r + (i - split) / q;
        const long long at = min(max((long long)seg.w + j, 0LL), (long long)n_index - 1);
        const long long t = min(max((long long)tok_index[at], 0LL), tok_rows - 1);
        const float4 *src = tok + (size_t)t * cols4;
        for (int c = lane; c < cols4; c += 64) dst[c] = src[c];
    }
}

}  // namespace cer

using namespace cer;

extern "C" int cer_text_spread_rows(const float *tok, int64_t tok_rows, int hidden, const int32_t *segments, int n_segments,
                                    const int32_t *tok_index, int n_index, float *out, int64_t out_rows, void *stream) {
    if (!tok || !segments || !tok_index || !out) return cer_set_error(CER_ERR_INVALID_ARG, "text_spread_rows: null pointer");
    if (tok_rows < 1 || hidden < 1 || n_segments < 1 || n_index < 1 || out_rows < 1)
        return cer_set_error(CER_ERR_INVALID_ARG, "text_spread_rows: token rows, hidden, segments, index entries and output rows "
                                                  "must be >= 1");
    if (hidden % 4) return cer_set_error(CER_ERR_INVALID_ARG, "text_spread_rows: hidden = %d is not a multiple of 4", hidden);
    if (((uintptr_t)tok | (uintptr_t)out | (uintptr_t)segments) & 15)
        return cer_set_error(CER_ERR_INVALID_ARG, "text_spread_rows: tok, out and segments must be 16-byte aligned");
    if (out_rows > 0x7fffffffLL) return cer_set_error(CER_ERR_INVALID_ARG, "text_spread_rows: too many output rows");
    const long long tiles = (out_rows + TSP_WAVES - 1) / TSP_WAVES;
    const dim3 grid((unsigned)n_segments, (unsigned)(tiles < TSP_MAX_Y ? tiles : TSP_MAX_Y)), block(TSP_THREADS);
    CER_LAUNCH(text_spread_rows_kernel, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(tok),
               (long long)tok_rows, hidden / 4, reinterpret_cast<const int4 *>(segments), tok_index, n_index,
               reinterpret_cast<float4 *>(out), (long long)out_rows);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
