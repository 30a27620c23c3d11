// tcn_stream.hip -- frame-at-a-time causal TCN: the conv of a TemporalBlock over c new frames of S streams, its taps gathered
// from a ring of past frames (reference models/temporal_convolutional_model.py:21-56, run incrementally).
//
// State of one ring: [S][R][C] fp32, channels-last, R a power of two; the host owns the write positions.  In lockstep (all
// streams advance together) that is one `head`: row (s, i), i < c, is the frame written at slot (head + i) & (R - 1); tap j of
// a k-tap, dilation-d conv reads slot (head + i - (k - 1 - j) d) & (R - 1).  A reset stream's ring is all zeros, which is the
// causal left zero-pad.
//
// The work is M = S * c rows (1 .. a few hundred) against k * Cin * Cout weights: bound by the weight read.  One block owns
// CO_T = 4 output channels x ROW_T = 8 rows; its 256 threads split K = k * Cin between them in float4 chunks (thread t takes
// chunks t, t + 256, ...), weights and ring rows go straight from global memory to registers, and the 256 partial sums of an
// output are folded by a wave butterfly and a fixed tree over the four waves.  So the grid is (Cout / 4) x (M / 8) blocks:
// one stream still spreads a 512-channel layer over 128 blocks.
//
// INVARIANT.  The chunk a thread owns, the order it adds them in, the butterfly and the wave tree depend on (k, Cin) only:
// an output value is the same bits whatever S, c, head, the wrap count or the neighbouring rows of its block.  There is no
// split over blocks along K, no atomics and no path picked by the row count.  Rows beyond M are clamped to row M - 1 for the
// loads (in bounds, never stored).
//
// Two ways to find the M rows, one arithmetic.  Lockstep (cer_tcn_stream_conv): M = S * c, row m is frame m % c of stream
// m / c at position head + m % c.  Row table (cer_tcn_stream_conv_rows): row m is the frame of stream row_stream[m] at
// position row_pos[m] (unwrapped, modulo 2^30), read from device memory; every ring of a launch masks the same position with
// its own R - 1, so one table serves all levels of a net and streams advance independently.  The table is data the host
// code cannot see at launch: the stream index is clamped into [0, S) and every slot is masked, so any content stays inside the
// rings.  The two differ in a `Where` functor (row m -> stream and positions) and in nothing else: one kernel template and one
// host path, ts_launch<Where>, with every shared check, the ts_args and the VEC / RES_VEC dispatch.  An entry point keeps what
// is its own (lockstep: the S * c product and the heads' ranges; row table: the table pointers) and hands ts_launch its name.
// The append kernels stay two (the lockstep one indexes rows in size_t, a functor over int rows would narrow it) behind one
// set of host checks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"

namespace cer {

constexpr int TS_THREADS = 256, TS_WAVES = TS_THREADS / 64, TS_CO = 4, TS_ROWS = 8;

// Where the rows of a block sit in a ring.
struct ts_rows {
    size_t base[TS_ROWS];   // s * R: first slot of the row's stream
    int pos[TS_ROWS];       // head + i (not wrapped)
};

// acc[a][r] += sum over this thread's chunks of w[co0 + a][chunk] * ring-row r [chunk].
// w: [Cout4][k][C4 * 4] zero-padded, 16-byte aligned.  VEC: C % 4 == 0 and the ring is 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void ts_dot(float (&acc)[TS_CO][TS_ROWS], const float *__restrict__ ring, const float *__restrict__ w,
                                       int C, int C4, int k, int dil, int R, const ts_rows &rw, int co0) {
    const int Q = k * C4;
    const size_t wrow = (size_t)Q * 4;
    for (int q = threadIdx.x; q < Q; q += TS_THREADS) {
        const int j = q / C4, ci = (q - j * C4) * 4, back = (k - 1 - j) * dil;
        float4 wv[TS_CO];
#pragma unroll
        for (int a = 0; a < TS_CO; ++a) wv[a] = *reinterpret_cast<const float4 *>(w + (size_t)(co0 + a) * wrow + (size_t)q * 4);
        float4 xv[TS_ROWS];
#pragma unroll
        for (int r = 0; r < TS_ROWS; ++r) {
            const float *p = ring + (rw.base[r] + (size_t)((rw.pos[r] - back) & (R - 1))) * C + ci;
            if (VEC) {
                xv[r] = *reinterpret_cast<const float4 *>(p);
            } else {   // the padded weight columns are zero, the matching inputs must be finite: 0, not the next row
                xv[r].x = p[0];
                xv[r].y = ci + 1 < C ? p[1] : 0.f;
                xv[r].z = ci + 2 < C ? p[2] : 0.f;
                xv[r].w = ci + 3 < C ? p[3] : 0.f;
            }
        }
#pragma unroll
        for (int a = 0; a < TS_CO; ++a)
#pragma unroll
            for (int r = 0; r < TS_ROWS; ++r) {
                float s = acc[a][r];
                s = fmaf(wv[a].x, xv[r].x, s);
                s = fmaf(wv[a].y, xv[r].y, s);
                s = fmaf(wv[a].z, xv[r].z, s);
                s = fmaf(wv[a].w, xv[r].w, s);
                acc[a][r] = s;
            }
    }
}

// Fold the block's 256 partials of each of the 32 outputs: butterfly over the 64 lanes, then (w0 + w1) + (w2 + w3).
// Threads 0 .. 31 return their output (a = t % TS_CO, r = t / TS_CO); `lds` holds TS_WAVES * 32 floats.
__device__ __forceinline__ float ts_fold(float (&acc)[TS_CO][TS_ROWS], float *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < TS_CO; ++a)
#pragma unroll
        for (int r = 0; r < TS_ROWS; ++r) {
            float v = acc[a][r];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) lds[wave * (TS_CO * TS_ROWS) + r * TS_CO + a] = v;
        }
    __syncthreads();
    float out = 0.f;
    if (threadIdx.x < TS_CO * TS_ROWS) {
        const float *p = lds + threadIdx.x;
        out = (p[0] + p[TS_CO * TS_ROWS]) + (p[2 * TS_CO * TS_ROWS] + p[3 * TS_CO * TS_ROWS]);
    }
    __syncthreads();
    return out;
}

struct ts_args {
    const float *ring, *w, *bias;          // conv input ring [S][R][Cin], packed filter, bias [Cout]
    const float *res_ring, *res_w, *res_bias;   // phase B: residual ring [S][res_R][res_C]; res_w NULL = identity
    float *out_ring, *out_dense;           // [S][out_R][Cout] and / or [M][Cout]
    int M, Cin, Cout, k, dil, R;
    int res_C, res_R, out_R;
    float slope;
};

// Where row m sits: its stream and its (unwrapped) position in the tap ring, the residual ring and the written ring.
struct ts_where {
    int s, pos, res_pos, out_pos;
};

// All streams advance together: row m is frame m % c of stream m / c, the rings' heads come from the host.
struct ts_lockstep {
    int c, head, res_head, out_head;
    __device__ __forceinline__ ts_where operator()(int m) const {
        const int s = m / c, i = m - s * c;
        return {s, head + i, res_head + i, out_head + i};
    }
};

// Each row names its stream and position; one position serves every ring.  The stream is clamped: a wrong table gives wrong
// numbers, never an address outside a ring.
struct ts_table {
    const int *row_stream, *row_pos;
    int S;
    __device__ __forceinline__ ts_where operator()(int m) const {
        const int s = min(max(row_stream[m], 0), S - 1), pos = row_pos[m];
        return {s, pos, pos, pos};
    }
};

__device__ __forceinline__ float ts_leaky(float v, float slope) { return v >= 0.f ? v : v * slope; }

template <bool VEC, bool RES_VEC, class Where>
__device__ __forceinline__ void ts_block(const ts_args &p, const Where &where, float *lds) {
    const int M = p.M, co0 = blockIdx.x * TS_CO, m0 = blockIdx.y * TS_ROWS;
    ts_rows rw, rr;
#pragma unroll
    for (int r = 0; r < TS_ROWS; ++r) {
        const ts_where at = where(min(m0 + r, M - 1));
        rw.base[r] = (size_t)at.s * p.R;
        rw.pos[r] = at.pos;
        rr.base[r] = (size_t)at.s * p.res_R;
        rr.pos[r] = at.res_pos;
    }
    float acc[TS_CO][TS_ROWS];
#pragma unroll
    for (int a = 0; a < TS_CO; ++a)
#pragma unroll
        for (int r = 0; r < TS_ROWS; ++r) acc[a][r] = 0.f;
    ts_dot<VEC>(acc, p.ring, p.w, p.Cin, (p.Cin + 3) >> 2, p.k, p.dil, p.R, rw, co0);
    const float conv = ts_fold(acc, lds);
    float proj = 0.f;
    if (p.res_w) {   // the 1x1 downsample of the block input at the new slots: a one-tap conv over the residual ring
#pragma unroll
        for (int a = 0; a < TS_CO; ++a)
#pragma unroll
            for (int r = 0; r < TS_ROWS; ++r) acc[a][r] = 0.f;
        ts_dot<RES_VEC>(acc, p.res_ring, p.res_w, p.res_C, (p.res_C + 3) >> 2, 1, 0, p.res_R, rr, co0);
        proj = ts_fold(acc, lds);
    }
    if (threadIdx.x >= TS_CO * TS_ROWS) return;
    const int a = threadIdx.x % TS_CO, r = threadIdx.x / TS_CO, co = co0 + a, m = m0 + r;
    if (co >= p.Cout || m >= M) return;
    const ts_where at = where(m);
    float v = ts_leaky(conv + p.bias[co], p.slope);
    if (p.res_ring) {
        float res;
        if (p.res_w)
            res = proj + p.res_bias[co];
        else
            res = p.res_ring[((size_t)at.s * p.res_R + (size_t)(at.res_pos & (p.res_R - 1))) * p.Cout + co];
        v = ts_leaky(v + res, p.slope);
    }
    if (p.out_ring) p.out_ring[((size_t)at.s * p.out_R + (size_t)(at.out_pos & (p.out_R - 1))) * p.Cout + co] = v;
    if (p.out_dense) p.out_dense[(size_t)m * p.Cout + co] = v;
}

template <bool VEC, bool RES_VEC, class Where>
__global__ __launch_bounds__(TS_THREADS) void tcn_stream_conv_kernel(ts_args p, Where where) {
    __shared__ float lds[TS_WAVES * TS_CO * TS_ROWS];
    ts_block<VEC, RES_VEC>(p, where, lds);
}

__global__ void tcn_stream_append_kernel(const float *__restrict__ rows, float *__restrict__ ring, int c, int C, int R, int head,
                                         size_t n) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const size_t m = idx / C;
    const int ch = (int)(idx - m * C);
    const size_t s = m / c;
    const int i = (int)(m - s * c);
    ring[(s * R + (size_t)((head + i) & (R - 1))) * C + ch] = rows[idx];
}

__global__ void tcn_stream_append_rows_kernel(const float *__restrict__ rows, float *__restrict__ ring,
                                              const int *__restrict__ row_stream, const int *__restrict__ row_pos, int S, int C,
                                              int R, size_t n) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const size_t m = idx / C;
    const int ch = (int)(idx - m * C);
    const size_t s = (size_t)min(max(row_stream[m], 0), S - 1);
    ring[(s * R + (size_t)(row_pos[m] & (R - 1))) * C + ch] = rows[idx];
}

// A power of two; 2^30 is the largest an int holds, and row positions are kept modulo 2^30.
static bool ts_ring_len(int v) { return v > 0 && (v & (v - 1)) == 0; }
static bool ts_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

#define ST ((hipStream_t)stream)
#define TS_REFUSE(...) return cer_set_error(CER_ERR_INVALID_ARG, __VA_ARGS__)

// The one validated launch under both conv entries.  `d`: the dimensions in the row-table descriptor's terms (lockstep: M =
// S * c, max_count = c); `p`: the eight pointers, the rest is filled in here; `entry` names the caller in every refusal.
template <class Where>
static int ts_launch(const char *entry, const cer_tcn_stream_rows_desc &d, ts_args p, const Where &where, void *stream) {
    const long long hist = (long long)(d.k - 1) * d.dil, ytiles = ((long long)d.M + TS_ROWS - 1) / TS_ROWS;
    if (!p.ring || !p.w || !p.bias || (!p.out_ring && !p.out_dense)) TS_REFUSE("%s: null pointer", entry);
    if ((p.res_w && (!p.res_ring || !p.res_bias)) || (!p.res_w && p.res_bias))
        TS_REFUSE("%s: res_w and res_bias come together, with res_ring", entry);
    if (d.S < 1 || d.M < 1 || d.max_count < 1 || d.Cin < 1 || d.Cout < 1 || d.k < 1 || d.dil < 1)
        TS_REFUSE("%s: streams, rows, new frames of a stream, Cin, Cout, k and dil must be >= 1", entry);
    if (!ts_ring_len(d.R) || (p.out_ring && !ts_ring_len(d.out_R)) || (p.res_ring && !ts_ring_len(d.res_R)))
        TS_REFUSE("%s: ring length R = %d (out %d, res %d) is not a power of two up to 2^30", entry, d.R, d.out_R, d.res_R);
    if (hist + d.max_count > d.R || (p.out_ring && d.max_count > d.out_R) || (p.res_ring && d.max_count > d.res_R))
        TS_REFUSE("%s: %d new frames of a stream plus (k - 1) * dil = %lld of history exceed R = %d (out %d, res %d)", entry,
                  d.max_count, hist, d.R, d.out_R, d.res_R);
    if (p.res_ring && (p.res_w ? d.res_C < 1 : d.res_C != d.Cout))
        TS_REFUSE("%s: residual ring of %d channels for Cout = %d without a projection", entry, d.res_C, d.Cout);
    if (!ts_al16(p.w) || (p.res_w && !ts_al16(p.res_w))) TS_REFUSE("%s: packed weights must be 16-byte aligned", entry);
    if (ytiles > 65535) TS_REFUSE("%s: %d rows exceed the grid", entry, d.M);
    p.M = d.M; p.Cin = d.Cin; p.Cout = d.Cout; p.k = d.k; p.dil = d.dil; p.R = d.R;
    p.res_C = p.res_ring ? d.res_C : 1; p.res_R = p.res_ring ? d.res_R : 1; p.out_R = p.out_ring ? d.out_R : 1;
    p.slope = d.slope;
    const bool vec = d.Cin % 4 == 0 && ts_al16(p.ring), rvec = p.res_w && d.res_C % 4 == 0 && ts_al16(p.res_ring);
    const dim3 grid((d.Cout + TS_CO - 1) / TS_CO, (unsigned)ytiles), block(TS_THREADS);
    if (vec && rvec) CER_LAUNCH((tcn_stream_conv_kernel<true, true, Where>), grid, block, 0, ST, p, where);
    else if (vec) CER_LAUNCH((tcn_stream_conv_kernel<true, false, Where>), grid, block, 0, ST, p, where);
    else if (rvec) CER_LAUNCH((tcn_stream_conv_kernel<false, true, Where>), grid, block, 0, ST, p, where);
    else CER_LAUNCH((tcn_stream_conv_kernel<false, false, Where>), grid, block, 0, ST, p, where);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

// What both append entries refuse: `count` new frames of a stream into a ring of R slots, n elements in all.
static int ts_append_check(const char *entry, bool null, int S, int M, int count, int C, int R, size_t n) {
    if (null) TS_REFUSE("%s: null pointer", entry);
    if (S < 1 || M < 1 || count < 1 || C < 1) TS_REFUSE("%s: streams, rows, new frames of a stream and C must be >= 1", entry);
    if (!ts_ring_len(R)) TS_REFUSE("%s: ring length R = %d is not a power of two up to 2^30", entry, R);
    if (count > R) TS_REFUSE("%s: %d new frames of a stream exceed R = %d", entry, count, R);
    if (n > (size_t)0x7fffffff * 256) TS_REFUSE("%s: too many elements", entry);
    return CER_OK;
}

}  // namespace cer

using namespace cer;

extern "C" int cer_tcn_stream_conv(const cer_tcn_stream_desc *d, const float *ring, const float *w, const float *bias,
                                   const float *res_ring, const float *res_w, const float *res_bias, float *out_ring,
                                   float *out_dense, void *stream) {
    if (!d) TS_REFUSE("tcn_stream_conv: null pointer");
    const long long M = (long long)d->S * d->c;   // bounded before it is narrowed; S < 1 or c < 1 is refused in ts_launch
    if (M > 65535LL * TS_ROWS) TS_REFUSE("tcn_stream_conv: S * c = %lld rows exceed the grid", M);
    if (d->head < 0 || d->head >= d->R || (out_ring && (d->out_head < 0 || d->out_head >= d->out_R)) ||
        (res_ring && (d->res_head < 0 || d->res_head >= d->res_R)))
        TS_REFUSE("tcn_stream_conv: head outside [0, R)");
    const cer_tcn_stream_rows_desc dims = {d->S, (int)M, d->c, d->Cin, d->Cout, d->k, d->dil, d->R, d->res_C, d->res_R,
                                           d->out_R, d->slope};
    const ts_lockstep where = {d->c, d->head, res_ring ? d->res_head : 0, out_ring ? d->out_head : 0};
    return ts_launch("tcn_stream_conv", dims, {ring, w, bias, res_ring, res_w, res_bias, out_ring, out_dense}, where, stream);
}

extern "C" int cer_tcn_stream_conv_rows(const cer_tcn_stream_rows_desc *d, const int32_t *row_stream, const int32_t *row_pos,
                                        const float *ring, const float *w, const float *bias, const float *res_ring,
                                        const float *res_w, const float *res_bias, float *out_ring, float *out_dense,
                                        void *stream) {
    if (!d || !row_stream || !row_pos) TS_REFUSE("tcn_stream_conv_rows: null pointer");
    const ts_table where = {row_stream, row_pos, d->S};
    return ts_launch("tcn_stream_conv_rows", *d, {ring, w, bias, res_ring, res_w, res_bias, out_ring, out_dense}, where, stream);
}

extern "C" int cer_tcn_stream_append(const float *rows, float *ring, int S, int c, int C, int R, int head, void *stream) {
    const size_t n = (size_t)S * c * C;
    if (int rc = ts_append_check("tcn_stream_append", !rows || !ring, S, c, c, C, R, n)) return rc;
    if (head < 0 || head >= R) TS_REFUSE("tcn_stream_append: head %d outside [0, %d)", head, R);
    CER_LAUNCH(tcn_stream_append_kernel, dim3(cer_blocks(n, 256)), dim3(256), 0, ST, rows, ring, c, C, R, head, n);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_tcn_stream_append_rows(const float *rows, float *ring, const int32_t *row_stream, const int32_t *row_pos,
                                          int S, int M, int max_count, int C, int R, void *stream) {
    const size_t n = (size_t)M * C;
    if (int rc = ts_append_check("tcn_stream_append_rows", !rows || !ring || !row_stream || !row_pos, S, M, max_count, C, R, n))
        return rc;
    CER_LAUNCH(tcn_stream_append_rows_kernel, dim3(cer_blocks(n, 256)), dim3(256), 0, ST, rows, ring, row_stream, row_pos, S, C, R,
               n);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
