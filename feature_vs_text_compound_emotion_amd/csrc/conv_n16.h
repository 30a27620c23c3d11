// conv_n16.h -- types and the MFMA wrapper shared by the narrow (single 16-bit plane) conv kernels; the weight ring and the
// nine-tap step of the window-resident kernels (conv_n16_patch.hip).
#pragma once
#include "conv_common.h"

namespace cer {

typedef __bf16 n_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 n_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int n_u32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 n_f32x4;
typedef __attribute__((address_space(3))) void *n_lds_ptr_t;

template <bool F16>
__device__ __forceinline__ n_f32x4 mfma_n16(const n_u32x4 a, const n_u32x4 b, const n_f32x4 c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(n_f16x8, a), __builtin_bit_cast(n_f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(n_bf16x8, a), __builtin_bit_cast(n_bf16x8, b), c, 0, 0, 0);
}

// 16x16-patch kernels: slot = chunk ^ PATCH_F[window column], 3 bits per column (tools/check_swizzle.py: patch_table_constant())
constexpr unsigned long long PATCH_F_TABLE = 0xd92dad912240ull;
__device__ __forceinline__ int patch_f(int wx) { return (int)((PATCH_F_TABLE >> (3 * wx)) & 7ull); }
// block -> (patch, cout tile) -> (image, patch row, patch column) through reciprocals of the launch constants (conv_common.h)
struct PatchGeo { FastDiv tiles_n, pxn, pyn; };

// ---- the window-resident kernels (conv_n16_patch.hip): a block's 256 pixels x BN couts, the input window of a 64-channel chunk
// resident in LDS across the nine taps.  The kernels differ in how the pixels map to the image, how the window is fetched and
// where a pixel fragment sits in LDS; the weight ring and the step below are what they share. ----

// A wave's share of the weight ring: one BN x 64 slice per step (one filter tap of one chunk) through three slots, issued two
// steps ahead, in WQ = BN / (8 NW) one-KiB pieces of 8 cout rows; row = cout, slot = chunk ^ ((row >> 1) & 7).  PP: a group's
// own cout half (BN / 16 pieces) dealt to its four waves -- the other group never reads them; else all pieces over all waves.
// Offsets are 32-bit: the launchers bound a weight panel by 2^31 bytes.
template <int BN, int NW, int TC, bool PP, int WQ>
__device__ __forceinline__ void n16_ring_assign(const ConvArgs &p, int wave, int lane, int c0, int (&piece)[WQ], unsigned (&off)[WQ]) {
    static_assert(BN % (8 * NW) == 0 && WQ == BN / (8 * NW), "weight-slice pieces are dealt round-robin to the waves");
    const int prow = lane >> 3, slot = lane & 7;
#pragma unroll
    for (int i = 0; i < WQ; ++i) {
        piece[i] = PP ? (wave >> 2) * (BN / 16) + (wave & 3) + 4 * i : wave + NW * i;
        const int row = piece[i] * 8 + prow;                                             // LDS row of the slice
        const int grow = row / (TC * 16) * (TC * 16) + epi_cout_of_row(row % (TC * 16));  // the cout it holds (conv_common.h)
        off[i] = c0 + grow < p.Cout ? (unsigned)(grow * p.Kpad * 2) + (unsigned)((slot ^ ((row >> 1) & 7)) << 4) : 0x80000000u;
    }
}
// weight slice (cc, tap) of the block's panel into ring slot `ring` (zero pieces into the sink past the end of the K loop: the
// per-step DMA count of a wave stays constant, which the counted vmcnt relies on)
template <int WSLICE, int WQ>
__device__ __forceinline__ void n16_ring_issue(const ConvArgs &p, const char *panel, unsigned char *slots, unsigned char *sink,
                                               const int (&piece)[WQ], const unsigned (&off)[WQ], int cc, int tap, int ring) {
    constexpr unsigned OOB = 0x80000000u;
    const bool real = cc < p.cin_steps;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(panel) + ((size_t)tap * p.Cin + (size_t)cc * 64) * 2, 0, (int)OOB, 0x00020000);
#pragma unroll
    for (int i = 0; i < WQ; ++i) {
        unsigned char *dst = real ? slots + ring * WSLICE + piece[i] * 1024 : sink;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (n_lds_ptr_t)dst, 16, (int)(real ? off[i] : OOB), 0, 0, 0);
    }
}

// One step = one filter tap of one 64-channel chunk.  DMA issued per wave and step: WQ weight pieces (slice of step s + 2)
// and, with two window buffers (XWIN2), one window piece of the next chunk during taps 0 .. XPW-1.
template <int TAP, int WQ, int XPW, bool XWIN2> constexpr int n16_step_pieces() { return WQ + ((XWIN2 && TAP < XPW) ? 1 : 0); }

// Top of a single-phase step (the ping-pong step has its barriers inside).  Every piece issued before step s-1 must have
// landed (slice s was issued in step s-2, the window of this chunk during the previous chunk / the prologue):
// vmcnt(pieces of the previous step); VM0 = what the prologue may leave in flight at the very first step (slice 1 where it
// was issued last).  lgkmcnt(0): this wave's fragment reads of the previous step have returned before anyone's DMA may
// overwrite the slot / window they came from.  The caller's fragment addresses of the step follow the barrier.
template <int TAP, int WQ, int XPW, bool XWIN2, bool PP, int VM0> __device__ __forceinline__ void n16_step_top(int cc) {
    if constexpr (!PP) {
        constexpr int pcnt = n16_step_pieces<(TAP + 8) % 9, WQ, XPW, XWIN2>();
        if (cc == 0 && TAP == 0) {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(VM0) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(pcnt) : "memory");
        }
        __builtin_amdgcn_s_barrier();
    }
}

// The step.  lda(a, kk) / ldb(b, kk): the weight fragment of cout tile a / the pixel fragment of pixel tile b, 32-deep half kk;
// issue_w(cc, tap, ring slot), issue_x(window piece, cc): the caller's DMA.  Per accumulator the MFMA order is kk = 0, 1.
//   PP (ping-pong): the two waves that share a SIMD (w and w + 4: the cout halves wc = 0 / 1) run half a step apart: a READ
//   phase (every fragment of the step, then the step's DMA) and an MFMA phase (nothing else) with a block barrier after each.
//   else: fragment reads run two MFMA groups (kk, b) ahead and the DMA pieces go between MFMA groups, as in conv_n16_kernel.
template <int TAP, int TC, int TP, int WQ, int XPW, bool XWIN2, bool PP, bool F16, class LDA, class LDB, class IW, class IX>
__device__ __forceinline__ void n16_step(n_f32x4 (&acc)[TC][TP], int cc, LDA &&lda, LDB &&ldb, IW &&issue_w, IX &&issue_x) {
    constexpr int NGRP = 2 * TP;                                   // MFMA groups (kk, b) per step, TC MFMAs each
    constexpr int ntap = (TAP + 2) % 9, nring = (TAP + 2) % 3;     // the slice two steps ahead
    constexpr bool XNOW = XWIN2 && TAP < XPW;                      // this step moves a window piece
    const int ncc = cc + (TAP + 2 >= 9 ? 1 : 0);
    n_u32x4 af[2][TC], bf[NGRP];
    if constexpr (PP) {
        // ---- READ phase ----
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int a = 0; a < TC; ++a) af[kk][a] = lda(a, kk);
#pragma unroll
        for (int g = 0; g < NGRP; ++g) bf[g] = ldb(g % TP, g / TP);
        issue_w(ncc, ntap, nring);
        if constexpr (XNOW) issue_x(TAP, cc + 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---- MFMA phase ----
#pragma unroll
        for (int g = 0; g < NGRP; ++g)
#pragma unroll
            for (int a = 0; a < TC; ++a) acc[a][g % TP] = mfma_n16<F16>(af[g / TP][a], bf[g], acc[a][g % TP]);
        // everything this wave issued before this step's READ phase has landed (slice of step + 1, older window pieces)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n16_step_pieces<TAP, WQ, XPW, XWIN2>()) : "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
        for (int a = 0; a < TC; ++a) af[0][a] = lda(a, 0);
        bf[0] = ldb(0, 0);
        bf[1] = ldb(1 % TP, 1 / TP);
        static_for<NGRP>([&](auto G) {
            constexpr int g = decltype(G)::v, kk = g / TP, b = g % TP;
            if constexpr (g + 2 < NGRP) bf[g + 2] = ldb((g + 2) % TP, (g + 2) / TP);
            if constexpr (g == 0) {
#pragma unroll
                for (int a = 0; a < TC; ++a) af[1][a] = lda(a, 1);
            }
            if constexpr (g == 0) issue_w(ncc, ntap, nring);
            if constexpr (g == 2 % NGRP && XNOW) issue_x(TAP, cc + 1);
#pragma unroll
            for (int a = 0; a < TC; ++a) acc[a][b] = mfma_n16<F16>(af[kk][a], bf[g], acc[a][b]);
        });
        // issue order: TC MFMAs of group g, then the reads for group g+2 and the group's DMA pieces (see conv_n16.hip)
        __builtin_amdgcn_sched_group_barrier(0x100, TC + 2, 0);
        static_for<NGRP>([&](auto G) {
            constexpr int g = decltype(G)::v;
            __builtin_amdgcn_sched_group_barrier(0x008, TC, 0);
            constexpr int nread = (g + 2 < NGRP ? 1 : 0) + (g == 0 ? TC : 0);
            if constexpr (nread > 0) __builtin_amdgcn_sched_group_barrier(0x100, nread, 0);
            constexpr int npiece = (g == 0 ? WQ : 0) + ((g == 2 % NGRP && XNOW) ? 1 : 0);
            if constexpr (npiece > 0) __builtin_amdgcn_sched_group_barrier(0x010, npiece, 0);
        });
    }
}

int conv_n16_patch_launch(int tile, const ConvArgs &a, hipStream_t st);  // conv_n16_patch.hip
int conv_n16_p64_launch(const ConvArgs &a, hipStream_t st);              // conv_n16_p64.hip: the persistent Cin == 64 patch kernel (tile 79)
bool conv_n16_p64_ok(const ConvArgs &a);
bool conv_n16_patch_ok(const ConvArgs &a, int tile);         // can the patch kernel `tile` take this conv?
bool conv_n16_win_ok(const ConvArgs &a);                     // can the 1-D window kernels (tiles 73 / 74)?
int conv_n16_s2d_launch(int tile, const ConvArgs &a, hipStream_t st);    // conv_n16_s2d.hip
bool conv_n16_s2d_ok(const ConvArgs &a);

}  // namespace cer
