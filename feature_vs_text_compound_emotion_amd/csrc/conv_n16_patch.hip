// conv_n16_patch.hip -- 3x3 / stride 1 / pad 1 convolution on narrow operands with the INPUT WINDOW RESIDENT IN LDS.
//
// Why.  PMC of the flat implicit-GEMM kernel (conv_n16.hip; profiles/round2_pmc_conv_n16.txt): the matrix pipes are busy a
// third of the time and 41 % of the wave cycles are parked at the vmcnt/barrier.  A flat M tile re-fetches its activation
// rows once per filter tap -- nine L2 -> LDS transfers of every input line, a fifth of which miss the XCD's 4 MiB L2
// because the kh-shifted re-reads come three steps (several MiB of other traffic) later; a 1-KiB DMA piece spans 8
// lines, so most pieces wait for a miss.  The kernel below fetches each input line ONCE per block:
//
//   * a block owns a 16 x 16 patch of output pixels of one image and BN output channels;
//   * per 64-channel chunk the 18 x 18 input window of the patch (halo included; out-of-image pixels come back as zeros
//     from the range-checked DMA) is brought into LDS by 41 one-KiB LDS-DMA pieces; all nine taps then read their pixel
//     fragments from it: the fragment of output row r under tap (kh, kw) is the 16 consecutive window pixels
//     (r + kh) * 18 + kw + (lane & 15).  Those rows start at any alignment, so the bank-conflict swizzle is a function of
//     the window COLUMN found by exhaustive search (tools/check_swizzle.py: conflict free for kw = 0, 1, 2);
//   * only the weights stream per step: one BN x 64 slice per (chunk, tap) through a 3-slot ring, two steps ahead with
//     a counted vmcnt; every block of a launch reads the same slices, so they are L2 hits with short latency, while the
//     long-latency window of the NEXT chunk is fetched a whole chunk (nine steps) ahead into the second window buffer;
//   * the nine taps are unrolled (tap, ring slot and the next slice's tap are compile-time), fragment reads run two
//     MFMA groups ahead and the DMA pieces are placed between MFMA groups, as in conv_n16_kernel.
//
// L2 -> LDS bytes per 256 pixels x 64 channels x 9 taps: 41 KiB of window + 9 weight slices, against 9 x 32 KiB of
// activations + the same 9 slices for the flat 256-row tile.
//
// Two kernels, ONE step: conv_n16_patch_kernel (16 x 16 patches) and conv_n16_win_kernel (256 consecutive pixels, any image
// size) differ in how a block's 256 pixels map to the image, how the window is fetched (issue_x) and where a pixel fragment
// sits in LDS (ldb).  The weight ring (n16_ring_assign / n16_ring_issue) and the unrolled step with its barriers, counted
// vmcnt and DMA placement (n16_step_top / n16_step) are conv_n16.h's, called by both: what the two compute per accumulator is
// the same instruction sequence, and their outputs are bit-equal (tests/test_conv_n16_gpu.py).
#include "conv_n16.h"

namespace cer {


template <int BN, int WP, int WC, int XBUFS, bool F16, bool PP>
__global__ __launch_bounds__(WP * WC * 64, 2) void conv_n16_patch_kernel(ConvArgs p, PatchGeo geo) {
    constexpr int NW = WP * WC, NT = NW * 64;
    constexpr int PH = 16, PWD = 16, WW = 18, WROWS = 18 * 18;    // patch and window geometry
    constexpr int XPIECES = (WROWS + 7) / 8;                       // 41 one-KiB pieces (328 rows, the last 4 unused)
    constexpr int XPW = (XPIECES + NW - 1) / NW;                   // window pieces per wave and chunk
    constexpr int XBYTES = XPIECES * 1024;
    constexpr int TP = PH / WP, TC = BN / (16 * WC);                // 16x16 MFMA tiles per wave: output rows x cout tiles
    constexpr int WSLICE = BN * 128, RING = 3, WQ = BN / (8 * NW);     // weight slice bytes, ring slots, pieces per wave and step
    static_assert(PH % WP == 0 && XBUFS >= 1 && XBUFS <= 2 && (XBUFS == 1 || XPW <= 9) && TC % 2 == 0, "geometry");
    static_assert(!PP || (WP == 4 && WC == 2 && XBUFS == 2 && (BN / 16) % 4 == 0), "ping-pong: waves w and w + 4 share a SIMD and split the couts");
    constexpr int WOFF = XBUFS * XBYTES, SINK = WOFF + RING * WSLICE;  // LDS map: windows | weight ring | 1 KiB sink
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) uint16_t smem_n16p[];
    unsigned char *smem = reinterpret_cast<unsigned char *>(smem_n16p);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave % WP, wc = wave / WP;
    const int kg = lane >> 4, l15 = lane & 15;

    const int bid = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
    const int patch = (int)fdiv((unsigned)bid, geo.tiles_n), tile_n = bid - patch * p.tiles_n;
    const int prw = (int)fdiv((unsigned)patch, geo.pxn), px = patch - prw * (int)geo.pxn.d;
    const int n = (int)fdiv((unsigned)prw, geo.pyn), py = prw - n * (int)geo.pyn.d;
    const int c0 = tile_n * BN;
    const int cin_steps = p.cin_steps;

    // ---- DMA assignment ----  (stamps of the 64 -> 64 @224x224 launch, tools/exp_stamp.py: the block used to spend 2.9 us of its
    // 13.7 on ~570 instructions of 64-bit address arithmetic and emulated divisions before its first load; everything below is
    // 32-bit -- conv_n16_patch_ok bounds an image and a weight panel by 2^31 bytes -- and the weight slices, whose addresses
    // need nothing of the patch, are issued before the window's addresses are computed)
    const int prow = lane >> 3, slot = lane & 7;
    unsigned w_off[WQ];
    int w_piece[WQ];
    n16_ring_assign<BN, NW, TC, PP>(p, wave, lane, c0, w_piece, w_off);
    const char *wpanel = reinterpret_cast<const char *>(p.w_hi) + (size_t)c0 * p.Kpad * 2;
    auto issue_w = [&](int cc, int tap, int ring) { n16_ring_issue<WSLICE>(p, wpanel, smem + WOFF, smem + SINK, w_piece, w_off, cc, tap, ring); };
    issue_w(0, 0, 0);
    issue_w(0, 1, 1);

    // window: wave w moves pieces w, w + NW, ...; in a piece lane l owns window row 8 * piece + l / 8 = (wy, wx), LDS slot
    // l % 8, and fetches source chunk slot ^ PATCH_F[wx]; offsets are relative to the image's first pixel
    unsigned x_off[XPW];
    bool x_real[XPW];
    {
        const int iy0 = py * PH - 1, ix0 = px * PWD - 1, pitch = p.x_ld * 2;
#pragma unroll
        for (int i = 0; i < XPW; ++i) {
            const int q = wave + NW * i;
            const int row = q * 8 + prow;
            const int wy = row / WW, wx = row - wy * WW;
            const int iy = iy0 + wy, ix = ix0 + wx;
            const bool inb = q < XPIECES && row < WROWS && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            const unsigned off = (unsigned)((iy * p.W + ix) * pitch) + (unsigned)((slot ^ patch_f(wx)) << 4);
            x_real[i] = q < XPIECES;
            x_off[i] = inb ? off : OOB;
        }
    }
    const char *ximg = reinterpret_cast<const char *>(p.x_hi) + (size_t)n * p.H * p.W * p.x_ld * 2;
    // window piece i of chunk cc into window buffer cc % XBUFS (or a zero piece into the sink: keeps the per-step DMA
    // count of a wave constant, which the counted vmcnt relies on)
    auto issue_x = [&](int i, int cc) {
        const bool real = x_real[i] && cc < cin_steps;
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(ximg) + (size_t)cc * 128, 0, (int)OOB, 0x00020000);
        unsigned char *dst = real ? smem + (XBUFS == 2 ? (cc & 1) * XBYTES : 0) + (wave + NW * i) * 1024 : smem + SINK;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (n_lds_ptr_t)dst, 16, (int)(real ? x_off[i] : OOB), 0, 0, 0);
    };
#pragma unroll
    for (int i = 0; i < XPW; ++i) issue_x(i, 0);

    n_f32x4 acc[TC][TP];
#pragma unroll
    for (int a = 0; a < TC; ++a)
#pragma unroll
        for (int b = 0; b < TP; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;

    // ---- fragment address bases ----
    // weights: row = cout, slot = chunk ^ ((row >> 1) & 7); pixels: window row (r + kh) * 18 + kw + l15 with output row
    // r = b * WP + wp, slot = chunk ^ PATCH_F[kw + l15]  (second 32-deep half: ^ 64 bytes)
    const int arow = WOFF + (wc * TC * 16 + l15) * 128 + ((kg ^ ((l15 >> 1) & 7)) << 4);
    int bcol[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) bcol[kw] = (wp * WW + kw + l15) * 128 + ((kg ^ patch_f(kw + l15)) << 4);

    // ---- prologue: the weight slices of steps 0 and 1 and the whole window of chunk 0 are in flight (issued above) ----
    pp_enter<PP, 0>(wc);

    for (int cc = 0; cc < cin_steps; ++cc) {
        const int xcur = XBUFS == 2 ? (cc & 1) * XBYTES : 0;
        static_for<9>([&](auto T) {
            constexpr int tap = decltype(T)::v, kh = tap / 3, kw = tap % 3;
            n16_step_top<tap, WQ, XPW, XBUFS == 2, PP, 0>(cc);
            const unsigned char *Wr = smem + (tap % 3) * WSLICE;
            const unsigned char *Xb = smem + xcur + kh * (WW * 128);
            auto lda = [&](int a, int kk) { return *reinterpret_cast<const n_u32x4 *>(Wr + ((arow + a * 16 * 128) ^ (kk << 6))); };
            auto ldb = [&](int b, int kk) { return *reinterpret_cast<const n_u32x4 *>(Xb + ((bcol[kw] + b * WP * WW * 128) ^ (kk << 6))); };
            n16_step<tap, TC, TP, WQ, XPW, XBUFS == 2, PP, F16>(acc, cc, lda, ldb, issue_w, issue_x);
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the sink pieces of the last steps (zero fills: they return at once)

    // ---- direct epilogue (the encoder's specialised modes): accumulators -> global memory, no LDS round trip (conv_common.h) ----
    const int emode = epi_mode(p);
    if (emode != EPI_GENERIC && (p.Cout & 7) == 0) {
        constexpr int NARROW = F16 ? CER_STORE_F16 : CER_STORE_BF16;
        float s1[TC / 2][8], s2[TC / 2][8];
        EpiPix epx[TP];
        {
            const int gx = px * PWD + l15;
            const int rx = gx == 0 ? 0 : (gx == p.W - 1 ? 2 : 1);
#pragma unroll
            for (int b = 0; b < TP; ++b) {
                const int gy = py * PH + b * WP + wp;
                const int ry = gy == 0 ? 0 : (gy == p.H - 1 ? 2 : 1);
                const int m = (n * p.H + gy) * p.W + gx;
                epx[b] = EpiPix{true, (size_t)(p.y_s2d ? s2d_row(m, gy, gx, p.W) : m), 3 * ry + rx};
            }
        }
        epi_dispatch(emode, [&](auto MODE_) {
            constexpr int MODE = decltype(MODE_)::v;
            if constexpr (MODE != EPI_GENERIC) epi_direct_stores<MODE, NARROW, TC, TP>(p, acc, c0 + wc * TC * 16, kg, epx, s1, s2);
        });
        pp_leave<PP>(wc);
        if (p.stats) epi_direct_stats<TC, WP, BN>(p, s1, s2, reinterpret_cast<float *>(smem_n16p), wp, wc, kg, l15, tid, c0, (size_t)patch);
        return;
    }
    pp_leave<PP>(wc);

    // ---- staged epilogue (every other launch; conv_common.h), one patch row per iteration ----
    static_assert(PWD == 16 && 256 * BN * 4 <= SINK, "patch rows of 16 pixels; one pass");
    float *Ct = reinterpret_cast<float *>(smem_n16p);
    EpiStaged<BN, NT> es;
    epi_staged_init(p, tid, c0, es);
    __syncthreads();  // the fragment reads of the last step are done
    epi_stage<BN, 0, TP>(Ct, acc, [&](int b) { return (b * WP + wp) * 16 + l15; },
                         [&](int a) { return (wc * TC * 16 + epi_cout_of_row(a * 16 + kg * 4)) >> 2; });
    __syncthreads();
    epi_staged_patch_rows<BN, NT, PH>(p, es, Ct, n, py * PH, px * PWD);
    epi_staged_stats(p, es, Ct, tid, c0, (size_t)patch);
}

// ------------------------------------------------------------------------------------------------------------------
// conv_n16_win_kernel: the window-resident structure for ANY image size (3x3 / stride 1 / pad 1) -- the 56x56 / 28x28 / 14x14 /
// 7x7 layers of the 224x224 pyramid and everything at the reference's 40x40 crop, which the 16x16-patch kernel cannot take.
// A block owns 256 CONSECUTIVE flattened output pixels m0 .. m0+255 (they may span image rows and images) and BN couts; the
// input of pixel m under tap (kh, kw) is pixel m + (kh-1) W + (kw-1) of the same flat array, so the window is the contiguous
// range [m0 - W - 1, m0 + 256 + W]: 258 + 2W rows of 128 bytes, fetched once per 64-channel chunk into one of two buffers; a
// tap is a row shift kh W + kw of the fragment address.  Taps outside the image (zero padding; in the flat array they are the
// neighbouring image row / frame) are masked per lane: the lane reads the window's last row, which the DMA zero-fills.
// Fragment rows start at any alignment: slot = chunk ^ (row & 6) is conflict free for all of them (tools/check_swizzle.py).
// PP (ping-pong): the two waves that share a SIMD (w and w + 4: the cout halves wc = 0 / 1) run half a step apart: a step is a
// READ phase (all 16 fragment reads + the step's DMA issue) and an MFMA phase (32 MFMAs, nothing else) with a block barrier
// after each, and group 1 starts one phase late, so one wave of a SIMD streams MFMAs while the other fetches.  Each group DMAs
// the weight rows of its own cout half (the other group never reads them): both keep the ring's two-step latency budget.
// XBUFS = 1: ONE window buffer (Cin == 64: a single chunk, nothing to prefetch) -- with 4 waves and 64 couts a block needs
// NP + 25 KiB, so two blocks share a CU and overlap each other's window fetch and epilogue (the 64 -> 64 layers at 40 x 40).
template <int BN, int WP, int WC, bool F16, bool PP, int XBUFS>
__global__ __launch_bounds__(WP * WC * 64, 2) void conv_n16_win_kernel(ConvArgs p, int NP, WinGeo geo) {
    constexpr int NW = WP * WC, NT = NW * 64, BM = 256;
    constexpr int NPMAX = 54;                                       // 8-row window pieces per buffer the LDS can hold twice (W <= 86)
    constexpr int XPW = (NPMAX + NW - 1) / NW;
    constexpr int TP = BM / (16 * WP), TC = BN / (16 * WC);
    constexpr int WSLICE = BN * 128, RING = 3, WQ = BN / (8 * NW);     // weight slice bytes, ring slots, pieces per wave and step
    static_assert((XBUFS == 1 || XPW <= 9) && TP >= 2 && (XBUFS == 2 || !PP) && TC % 2 == 0, "geometry");
    static_assert(!PP || (WP == 4 && WC == 2 && (BN / 16) % 4 == 0), "ping-pong: waves w and w + 4 share a SIMD and split the couts");
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) uint16_t smem_n16p[];
    unsigned char *smem = reinterpret_cast<unsigned char *>(smem_n16p);
    const int XBYTES = NP * 1024, WOFF = XBUFS * XBYTES, SINK = WOFF + RING * WSLICE;
    const int ZROW = NP * 8 - 1;                                    // past the rows the taps address: always zero-filled

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave % WP, wc = wave / WP;
    const int kg = lane >> 4, l15 = lane & 15;

    const int bid = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
    const int tile_m = (int)fdiv((unsigned)bid, geo.tiles_n), tile_n = bid - tile_m * p.tiles_n;
    const int m0 = tile_m * BM, c0 = tile_n * BN;
    const int cin_steps = p.cin_steps;
    const int rows_needed = BM + 2 * p.W + 2;
    const int wstart = m0 - p.W - 1;                                // first window pixel (negative in the first tile)

    // (32-bit address arithmetic: conv_n16_win_ok bounds a window by 2^31 bytes and M = N H W is an int)
    const int prow = lane >> 3, slot = lane & 7;
    unsigned x_off[XPW];
    bool x_real[XPW];
#pragma unroll
    for (int i = 0; i < XPW; ++i) {
        const int q = wave + NW * i;
        const int row = q * 8 + prow;
        const int pix = wstart + row;
        const bool inb = q < NP && row < rows_needed && pix >= 0 && pix < p.M;
        x_real[i] = q < NP;
        x_off[i] = inb ? (unsigned)(row * p.x_ld * 2) + (unsigned)((slot ^ (row & 6)) << 4) : OOB;
    }
    unsigned w_off[WQ];
    int w_piece[WQ];
    n16_ring_assign<BN, NW, TC, PP>(p, wave, lane, c0, w_piece, w_off);
    // base of the window's first pixel; lanes whose pixel lies outside the tensor carry the out-of-range offset instead
    const char *xwin = reinterpret_cast<const char *>(p.x_hi) + (long long)wstart * p.x_ld * 2;
    const char *wpanel = reinterpret_cast<const char *>(p.w_hi) + (size_t)c0 * p.Kpad * 2;

    auto issue_x = [&](int i, int cc) {
        const bool real = x_real[i] && cc < cin_steps;
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(xwin) + (size_t)cc * 128, 0, (int)OOB, 0x00020000);
        unsigned char *dst = real ? smem + (XBUFS == 2 ? (cc & 1) * XBYTES : 0) + (wave + NW * i) * 1024 : smem + SINK;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (n_lds_ptr_t)dst, 16, (int)(real ? x_off[i] : OOB), 0, 0, 0);
    };
    auto issue_w = [&](int cc, int tap, int ring) { n16_ring_issue<WSLICE>(p, wpanel, smem + WOFF, smem + SINK, w_piece, w_off, cc, tap, ring); };

    n_f32x4 acc[TC][TP];
#pragma unroll
    for (int a = 0; a < TC; ++a)
#pragma unroll
        for (int b = 0; b < TP; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.f;

    // per pixel tile b: the lane's window row under tap (0, 0) and the 9-bit mask of the taps that stay inside its image
    int prow0[TP];
    unsigned taps[TP];
#pragma unroll
    for (int b = 0; b < TP; ++b) {
        const int pl = (b * WP + wp) * 16 + l15;
        prow0[b] = pl;
        const int m = m0 + pl;
        unsigned bits = 0;
        if (m < p.M) {
            const int r = m - (int)fdiv((unsigned)m, geo.hw) * (int)geo.hw.d;
            const int y = (int)fdiv((unsigned)r, geo.w), x = r - y * p.W;
            const unsigned rowm = (y > 0 ? 1u : 0u) | 2u | (y < p.H - 1 ? 4u : 0u), colm = (x > 0 ? 1u : 0u) | 2u | (x < p.W - 1 ? 4u : 0u);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
                if ((rowm >> kh) & 1u) bits |= colm << (3 * kh);
        }
        taps[b] = bits;
    }
    const int arow = (wc * TC * 16 + l15) * 128 + ((kg ^ ((l15 >> 1) & 7)) << 4);

#pragma unroll
    for (int i = 0; i < XPW; ++i) issue_x(i, 0);
    issue_w(0, 0, 0);
    issue_w(0, 1, 1);
    pp_enter<PP, WQ>(wc);

    for (int cc = 0; cc < cin_steps; ++cc) {
        const int xcur = XBUFS == 2 ? (cc & 1) * XBYTES : 0;
        static_for<9>([&](auto T) {
            constexpr int tap = decltype(T)::v, kh = tap / 3, kw = tap % 3;
            n16_step_top<tap, WQ, XPW, XBUFS == 2, PP, WQ>(cc);
            const unsigned char *Wr = smem + WOFF + (tap % 3) * WSLICE;
            const unsigned char *Xb = smem + xcur;
            const int toff = kh * p.W + kw;
            int baddr[TP];
#pragma unroll
            for (int b = 0; b < TP; ++b) {
                const int row = ((taps[b] >> tap) & 1u) ? prow0[b] + toff : ZROW;
                baddr[b] = row * 128 + ((kg ^ (row & 6)) << 4);
            }
            auto lda = [&](int a, int kk) { return *reinterpret_cast<const n_u32x4 *>(Wr + ((arow + a * 16 * 128) ^ (kk << 6))); };
            auto ldb = [&](int b, int kk) { return *reinterpret_cast<const n_u32x4 *>(Xb + (baddr[b] ^ (kk << 6))); };
            n16_step<tap, TC, TP, WQ, XPW, XBUFS == 2, PP, F16>(acc, cc, lda, ldb, issue_w, issue_x);
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- direct epilogue (the encoder's specialised modes): accumulators -> global memory, no LDS round trip (conv_common.h) ----
    const int emode = epi_mode(p);
    if (emode != EPI_GENERIC && (p.Cout & 7) == 0) {
        constexpr int NARROW = F16 ? CER_STORE_F16 : CER_STORE_BF16;
        float s1[TC / 2][8], s2[TC / 2][8];
        // the lane's pixel of every pixel tile: its output row and border case (from the tap mask: a missing (0, 1) / (2, 1) /
        // (1, 0) / (1, 2) tap is the first / last image row / column)
        EpiPix epx[TP];
#pragma unroll
        for (int b = 0; b < TP; ++b) {
            const int m = m0 + prow0[b];
            const unsigned bits = taps[b];
            const int ry = !((bits >> 1) & 1u) ? 0 : (!((bits >> 7) & 1u) ? 2 : 1), rx = !((bits >> 3) & 1u) ? 0 : (!((bits >> 5) & 1u) ? 2 : 1);
            epx[b] = EpiPix{m < p.M, (size_t)m, 3 * ry + rx};
            if (p.y_s2d && epx[b].live) {
                const int r = m % (p.Ho * p.Wo);
                const int ho = r / p.Wo;
                epx[b].row = (size_t)s2d_row(m, ho, r - ho * p.Wo, p.Wo);
            }
        }
        epi_dispatch(emode, [&](auto MODE_) {
            constexpr int MODE = decltype(MODE_)::v;
            if constexpr (MODE != EPI_GENERIC) epi_direct_stores<MODE, NARROW, TC, TP>(p, acc, c0 + wc * TC * 16, kg, epx, s1, s2);
        });
        pp_leave<PP>(wc);
        if (p.stats) epi_direct_stats<TC, WP, BN>(p, s1, s2, reinterpret_cast<float *>(smem_n16p), wp, wc, kg, l15, tid, c0, (size_t)tile_m);
        return;
    }
    pp_leave<PP>(wc);

    // ---- staged epilogue (every other launch; conv_common.h) over consecutive output pixels ----
    float *Ct = reinterpret_cast<float *>(smem_n16p);   // the launcher sizes the LDS for 256 * BN floats at least
    EpiStaged<BN, NT> es;
    epi_staged_init(p, tid, c0, es);
    __syncthreads();
    epi_stage<BN, 0, TP>(Ct, acc, [&](int b) { return (b * WP + wp) * 16 + l15; },
                         [&](int a) { return (wc * TC * 16 + epi_cout_of_row(a * 16 + kg * 4)) >> 2; });
    __syncthreads();
    epi_staged_rows<BN, NT, BM, false, true, true>(p, es, Ct, m0, 0);
    epi_staged_stats(p, es, Ct, tid, c0, (size_t)tile_m);
}

// 8-row window pieces per buffer for this conv, or 0 when two buffers do not fit beside the 128-cout weight ring
static int n16_win_pieces(const ConvArgs &a) {
    const int np = (256 + 2 * a.W + 2 + 1 + 7) / 8;   // + 1: the last row stays zero (masked taps read it)
    return np <= 54 ? np : 0;
}

template <int BN, int WP, int WC, bool PP, int XBUFS = 2>
static int launch_win(const ConvArgs &a, hipStream_t st) {
    const int np = n16_win_pieces(a);
    size_t lds = (size_t)XBUFS * np * 1024 + 3 * (size_t)BN * 128 + 1024;
    if (lds < (size_t)256 * BN * 4) lds = (size_t)256 * BN * 4;   // the epilogue's accumulator tile
    const dim3 grid(a.tiles_m * a.tiles_n, 1, 1), block(WP * WC * 64);
    const WinGeo geo{make_fastdiv((unsigned)a.tiles_n), make_fastdiv((unsigned)(a.H * a.W)), make_fastdiv((unsigned)a.W)};
    return a.narrow == CER_STORE_F16 ? launch_lds(conv_n16_win_kernel<BN, WP, WC, true, PP, XBUFS>, grid, block, lds, st, a, np, geo)
                                     : launch_lds(conv_n16_win_kernel<BN, WP, WC, false, PP, XBUFS>, grid, block, lds, st, a, np, geo);
}

bool conv_n16_win_ok(const ConvArgs &a) {
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.dil_h != 1 || a.dil_w != 1 || a.pad_t != 1 || a.pad_l != 1 || a.Ho != a.H ||
        a.Wo != a.W || a.H < 2 || a.W < 2 || (a.Cin & 63) || a.split_k != 1 || n16_win_pieces(a) == 0)
        return false;
    return (long long)(512 + 2 * a.W) * a.x_ld * 2 < (1ll << 31) && (long long)128 * a.Kpad * 2 < (1ll << 31);
}

template <int BN, int WP, int WC, int XBUFS, bool PP>
static int launch_patch(const ConvArgs &a, hipStream_t st) {
    constexpr int XPIECES = 41;
    const size_t lds = (size_t)XBUFS * XPIECES * 1024 + 3 * (size_t)BN * 128 + 1024;
    const dim3 grid(a.tiles_m * a.tiles_n, 1, 1), block(WP * WC * 64);
    const PatchGeo geo{make_fastdiv((unsigned)a.tiles_n), make_fastdiv((unsigned)(a.W / 16)), make_fastdiv((unsigned)(a.H / 16))};
    return a.narrow == CER_STORE_F16 ? launch_lds(conv_n16_patch_kernel<BN, WP, WC, XBUFS, true, PP>, grid, block, lds, st, a, geo)
                                     : launch_lds(conv_n16_patch_kernel<BN, WP, WC, XBUFS, false, PP>, grid, block, lds, st, a, geo);
}

// tile ids: 71 = 16x16 patch x 64 couts, 4 waves, ONE window buffer (Cin == 64 only; 74 KiB of LDS -> two blocks per CU, so
// one block's window fetch overlaps the other's nine steps); 72 = 16x16 patch x 128 couts, 8 waves, two window buffers
bool conv_n16_patch_ok(const ConvArgs &a, int tile) {
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.dil_h != 1 || a.dil_w != 1 || a.pad_t != 1 || a.pad_l != 1 || a.Ho != a.H ||
        a.Wo != a.W || (a.H & 15) || (a.W & 15) || (a.Cin & 63) || a.split_k != 1)
        return false;
    if ((long long)a.H * a.W * a.x_ld * 2 >= (1ll << 31) || (long long)128 * a.Kpad * 2 >= (1ll << 31)) return false;
    if (tile == 71) return a.Cin == 64;
    return tile == 72 || tile == 78;
}

int conv_n16_patch_launch(int tile, const ConvArgs &a, hipStream_t st) {
    if (tile == 77) {
        if (!conv_n16_win_ok(a) || a.Cin != 64)
            return cer_set_error(CER_ERR_UNSUPPORTED, "conv2d (narrow, single-window kernel): needs a 3x3 / stride 1 / pad 1 conv with "
                                                       "W <= 86 and Cin == 64, no split-K");
        return launch_win<64, 4, 1, false, 1>(a, st);
    }
    if (tile == 73 || tile == 76) {
        if (!conv_n16_win_ok(a))
            return cer_set_error(CER_ERR_UNSUPPORTED, "conv2d (narrow, window kernel): needs a 3x3 / stride 1 / pad 1 conv with W <= 86, "
                                                       "Cin % 64 == 0, no split-K");
        return tile == 73 ? launch_win<64, 4, 2, false>(a, st) : launch_win<128, 4, 2, true>(a, st);   // 76: ping-pong phases
    }
    if (!conv_n16_patch_ok(a, tile))
        return cer_set_error(CER_ERR_UNSUPPORTED, "conv2d (narrow, patch kernel): needs a 3x3 / stride 1 / pad 1 conv on images whose "
                                                   "height and width are multiples of 16, Cin % 64 == 0 (tile 71: Cin == 64), no split-K");
    switch (tile) {
        case 71: return launch_patch<64, 4, 1, 1, false>(a, st);
        case 72: return launch_patch<128, 4, 2, 2, false>(a, st);
        case 78: return launch_patch<128, 4, 2, 2, true>(a, st);     // ping-pong variant of 72
        default: return cer_set_error(CER_ERR_INVALID_ARG, "conv2d (narrow, patch kernel): unknown tile id");
    }
}

}  // namespace cer
