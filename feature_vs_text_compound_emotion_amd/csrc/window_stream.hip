// window_stream.hip -- the evaluator's window rule on a live stream: the frames that became final are stitched from a ring of
// the stream's last window outputs (reference trainer.py:832-912, inference_forward_windows + windowing, run incrementally).
//
// State: wring [S][K][W][C] fp32.  Regular window i of a stream (frames [i H, i H + W)) sits in slot i % (K - 1); slot K - 1
// holds the stream's tail window [n - W, n), or its single short window [0, n) when the stream ended with n < W frames.  The
// host owns the counters: per stream the number of regular windows done and the tail's start (-1: none).
//
// A launch takes P rows (stream, frame) and writes out [P][C]: per (row, class) it walks the regular windows still in the ring
// in ascending start, then the tail (whose start is above every regular start), exactly as window_stitch_kernel does,
//   s = 0.f;  s += win[...] per covering window;  out = s / (float)cnt
// so an element is the same bits as the offline stitch of the same window outputs.  One thread per element: no LDS, no
// atomic, no wait between workgroups; a row's K - 1 candidate windows cost K - 1 compares and at most ceil(W / H) loads.
//
// The tables are data the host code cannot see at launch.  They never become an address unchecked: the stream is clamped into
// [0, S), a slot is a remainder modulo K - 1 (or the constant K - 1), a window row outside [0, W) is skipped and a negative
// window count is read as 0.  Wrong tables give wrong numbers, never an access outside the ring.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"

namespace cer {

__global__ __launch_bounds__(256) void window_stitch_stream_kernel(const float *__restrict__ wring, int S, int K, int W, int C, int H,
                                                                   const int *__restrict__ row_stream,
                                                                   const int *__restrict__ row_frame, int P,
                                                                   const int *__restrict__ win_done,
                                                                   const int *__restrict__ tail_start, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)P * C) return;
    const int m = (int)(i / C), c = (int)(i - (size_t)m * C);
    const int st = min(max(row_stream[m], 0), S - 1);
    const long long f = row_frame[m];
    const int done = max(win_done[st], 0), tail = tail_start[st];
    const size_t base = (size_t)st * K;
    float s = 0.f;
    int cnt = 0;
    for (int w = max(done - (K - 1), 0); w < done; ++w) {   // the regular windows the ring still holds, ascending start
        const long long r = f - (long long)w * H;
        if (r >= 0 && r < W) {
            s += wring[((base + (size_t)(w % (K - 1))) * W + (size_t)r) * C + c];
            ++cnt;
        }
    }
    const long long r = f - (long long)tail;
    if (tail >= 0 && r >= 0 && r < W) {
        s += wring[((base + (size_t)(K - 1)) * W + (size_t)r) * C + c];
        ++cnt;
    }
    out[i] = cnt > 0 ? s / (float)cnt : 0.f;
}

}  // namespace cer

using namespace cer;

extern "C" int cer_window_stitch_stream(const float *wring, int S, int K, int W, int C, int H, const int32_t *row_stream,
                                        const int32_t *row_frame, int P, const int32_t *win_done, const int32_t *tail_start,
                                        float *out, void *stream) {
    if (!wring || !row_stream || !row_frame || !win_done || !tail_start || !out)
        return cer_set_error(CER_ERR_INVALID_ARG, "window_stitch_stream: null pointer");
    if (S < 1 || K < 2 || W < 1 || C < 1 || H < 1 || P < 1)
        return cer_set_error(CER_ERR_INVALID_ARG, "window_stitch_stream: streams, W, C, H and rows must be >= 1 and K >= 2 "
                                                  "(a regular slot and the tail's)");
    if (H > W) return cer_set_error(CER_ERR_INVALID_ARG, "window_stitch_stream: hop %d exceeds the window %d", H, W);
    if (((uintptr_t)wring | (uintptr_t)out | (uintptr_t)row_stream | (uintptr_t)row_frame | (uintptr_t)win_done |
         (uintptr_t)tail_start) & 3)
        return cer_set_error(CER_ERR_INVALID_ARG, "window_stitch_stream: buffers must be 4-byte aligned");
    const size_t n = (size_t)P * C;
    if (n > (size_t)0x7fffffff * 256) return cer_set_error(CER_ERR_INVALID_ARG, "window_stitch_stream: too many elements");
    CER_LAUNCH(window_stitch_stream_kernel, dim3(cer_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, wring, S, K, W, C, H,
               row_stream, row_frame, P, win_done, tail_start, out);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
