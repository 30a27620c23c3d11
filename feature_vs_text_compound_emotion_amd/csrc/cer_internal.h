// cer_internal.h -- shared helpers for the libcer_hip translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cer_hip.h"

// Records a thread-local message and returns `code` (always negative).
int cer_set_error(int code, const char *fmt, ...);

#define CER_HIP_CHECK(expr)                                                                   \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return cer_set_error(CER_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr,    \
                                 hipGetErrorString(_e));                                      \
    } while (0)

static inline unsigned cer_blocks(size_t n, unsigned per_block) {
    return (unsigned)((n + per_block - 1) / per_block);
}

// Launch with the thread's sticky HIP error cleared first, so that the hipGetLastError()
// check after the launch reports THIS launch and not an unrelated earlier failure (e.g. a
// device probe made before the process had initialised its GPU).
#define CER_LAUNCH(...)                 \
    do {                                \
        (void)hipGetLastError();        \
        hipLaunchKernelGGL(__VA_ARGS__); \
    } while (0)

// The float4 apply passes of cer_bn_rows_bwd_apply (unit_passes.hip): dx as a split tensor (dx_hi != NULL), or fp32 with an
// optional addend; dense rows, C % 4 == 0, arguments checked by the caller.
int bn_rows_bwd_apply4(const float *dy, const float *x, const float *save_mean, const float *save_invstd, const float *w,
                       const float *sums, float inv_count, const float *add, float *dx, uint16_t *dx_hi, uint16_t *dx_lo, int R,
                       int C, hipStream_t stream);
