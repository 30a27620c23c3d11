// conv_b3.h -- types shared by the bf16x3 (split hi/lo operand) conv kernels; the nine-tap step of the window-resident
// kernels (conv_b3_patch.hip).
#pragma once
#include "conv_common.h"

namespace cer {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));  // 16-byte staging unit (first-class vector:
                                                                 // HIP's uint4 struct arrays ended up in scratch)
typedef __attribute__((address_space(3))) void *lds_ptr_t;

__device__ __forceinline__ bf16x8 as_bf16x8(const u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

__device__ __forceinline__ int swz16(int q) { return (0x78 >> (2 * q)) & 3; }  // F = {0, 2, 3, 1}

// ---- the window-resident kernels (conv_b3_patch.hip): a block's 256 pixels x BN couts, both planes of the input window of a
// 32-channel chunk resident in LDS across the nine taps.  The kernels differ in how the pixels map to the image, how the window
// is fetched and where a pixel fragment sits in LDS; the step below is what they share (and, as text in both, the weight ring:
// conv_b3_patch_kernel says why). ----

// One step = one filter tap of one 32-channel chunk.  lda(a, pl) / ldb(b, pl): plane pl (0 = hi, 1 = lo) of the weight fragment
// of cout tile a / of the pixel fragment of pixel tile b (fragments travel as u32x4 and are re-typed at the MFMA: a lambda
// returning a __bf16 vector made hipcc's host pass drop the kernel stub); issue_w(cc, tap, ring slot), issue_x(window piece,
// cc): the caller's DMA.  Per accumulator the MFMA order is lo*hi, hi*lo, hi*hi.
//   ping-pong (!SINGLE): the two waves that share a SIMD (w and w + 4: the cout halves wc = 0 / 1) run half a step apart: a READ
//   phase (every fragment of the step, then the step's DMA: WQ pieces of the slice of step + 2 and, during taps 0 .. XPW-1, the
//   two planes of one window piece of the next chunk) and an MFMA phase (nothing else) with a block barrier after each.
//   SINGLE: at the top the slice of this step has landed (issued two steps ago: vmcnt(WQ); the one window buffer is re-filled
//   by the caller between chunks), reads run two pixel tiles ahead, the slice of step + 2 goes after the first MFMA group.
template <int TAP, int TC, int TP, int WQ, int XPW, bool SINGLE, class LDA, class LDB, class IW, class IX>
__device__ __forceinline__ void b3_step(f32x4 (&acc)[TC][TP], int cc, LDA &&lda, LDB &&ldb, IW &&issue_w, IX &&issue_x) {
    constexpr int ntap = (TAP + 2) % 9, nring = (TAP + 2) % 3;     // the slice two steps ahead
    const int ncc = cc + (TAP + 2 >= 9 ? 1 : 0);
    if constexpr (!SINGLE) {
        // ---- READ phase ----
        u32x4 ah[TC], al[TC], bh[TP], bl[TP];
#pragma unroll
        for (int a = 0; a < TC; ++a) { ah[a] = lda(a, 0); al[a] = lda(a, 1); }
#pragma unroll
        for (int b = 0; b < TP; ++b) { bh[b] = ldb(b, 0); bl[b] = ldb(b, 1); }
        issue_w(ncc, ntap, nring);
        if constexpr (TAP < XPW) issue_x(TAP, cc + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- MFMA phase: consecutive MFMAs go to different accumulators ----
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int g = 0; g < TP; ++g)
                acc[a][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(al[a]), as_bf16x8(bh[g]), acc[a][g], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int g = 0; g < TP; ++g)
                acc[a][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ah[a]), as_bf16x8(bl[g]), acc[a][g], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
            for (int g = 0; g < TP; ++g)
                acc[a][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ah[a]), as_bf16x8(bh[g]), acc[a][g], 0, 0, 0);
        // everything this wave issued before this step's READ phase has landed (slice of step + 1, older window pieces)
        constexpr int cnt = WQ + (TAP < XPW ? 2 : 0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(cnt) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    } else {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(WQ) : "memory");
        __builtin_amdgcn_s_barrier();
        u32x4 ah[TC], al[TC], bh[TP], bl[TP];
#pragma unroll
        for (int a = 0; a < TC; ++a) { ah[a] = lda(a, 0); al[a] = lda(a, 1); }
        bh[0] = ldb(0, 0); bl[0] = ldb(0, 1);
        bh[1] = ldb(1, 0); bl[1] = ldb(1, 1);
        static_for<TP>([&](auto G) {
            constexpr int g = decltype(G)::v;
            if constexpr (g + 2 < TP) { bh[g + 2] = ldb(g + 2, 0); bl[g + 2] = ldb(g + 2, 1); }
            if constexpr (g == 0) issue_w(ncc, ntap, nring);
#pragma unroll
            for (int a = 0; a < TC; ++a) {
                acc[a][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(al[a]), as_bf16x8(bh[g]), acc[a][g], 0, 0, 0);
                acc[a][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ah[a]), as_bf16x8(bl[g]), acc[a][g], 0, 0, 0);
                acc[a][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(ah[a]), as_bf16x8(bh[g]), acc[a][g], 0, 0, 0);
            }
        });
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * TC + 4, 0);
        static_for<TP>([&](auto G) {
            constexpr int g = decltype(G)::v;
            __builtin_amdgcn_sched_group_barrier(0x008, 3 * TC, 0);
            if constexpr (g + 2 < TP) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            if constexpr (g == 0) __builtin_amdgcn_sched_group_barrier(0x010, WQ, 0);
        });
    }
}

int conv_b3_patch_launch(int tile, const ConvArgs &a, hipStream_t st);  // conv_b3_patch.hip
bool conv_b3_patch_ok(const ConvArgs &a);
bool conv_b3_win_ok(const ConvArgs &a);
int conv_b3_s2d_launch(int tile, const ConvArgs &a, hipStream_t st);    // conv_b3_s2d.hip
bool conv_b3_s2d_ok(const ConvArgs &a);

}  // namespace cer
