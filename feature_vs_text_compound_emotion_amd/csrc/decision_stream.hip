// decision_stream.hip -- running video-level decisions of S live streams: logit rows in, the reference's three decisions out
// (metrics.py:118-139: majority vote over the frame predictions, argmax of the mean logits, argmax of the mean softmax
// probabilities; optionally without the last column, C-EXPR-DB's 'Other').
//
// Two modes.  Whole-stream (W = 0): all frames since the stream's reset, held as four accumulators per (stream, class) in HBM:
// votes and first (int64: the count of frames predicted as c and the index since reset of the first one; never seen:
// INT64_MAX), slog and sprob (float64 sums of the logits and of the probabilities).  Window (W >= 1): the last min(n, W)
// frames, held as the logits themselves in a ring zring [S][R][C] fp32, R a power of two >= W + max_count; a decision is
// recomputed from the window's rows, nothing is accumulated across pushes.
//
// ONE ARITHMETIC, used by both modes and by both entries (ds_run):
//   frame prediction   argmax_first over the first nc columns (the first NaN, otherwise the first maximum: numpy.argmax)
//   probability        expf(z[c]) / (expf(z[0]) + ... + expf(z[nc - 1])), fp32, no max subtraction, the sum in column order
//   column sums        acc += (double)value, ONE CHAIN per (stream, class) IN TIME ORDER
//   mean               sum / n in double; the decisions compare the doubles, the output is that double rounded once to fp32
//   vote               the largest count, ties to the class first seen earliest (collections.Counter.most_common)
// argmax_first and the probability expression are restated from csrc/eval_metrics.hip, which keeps its own copy (and its
// bits: its column sums are a 256-way tree over the whole video, which no stream can continue).
//
// INVARIANT.  The chain of a (stream, class) walks that stream's rows in time order and nothing else: whole-stream, a push
// continues it from the accumulators; window, it starts at zero at the window's oldest row.  Its bits do not depend on how
// the rows were cut into pushes, on max_count, on the ring position, on S or on the other streams of a launch.
//
// Launch shape: one block of one wave per segment (one stream's new rows of this push), or per stream for a read.  Rows
// go through LDS in tiles of 64 taken in order: lane i computes the prediction and the softmax denominator of row i, then
// lane c runs the chains of class c over the tile's rows.  No global atomics, no grid sync, no flags, no scratch.
//
// The device keeps no counters: a push uploads a table segments [6][A] int32 = stream, count, offset into the packed rows,
// ring position of the first new row (modulo 2^30), and the stream's frames since reset BEFORE this push as a 64-bit value
// (low word, high word).  A read takes the same six fields per stream: count = rows in the window (ignored whole-stream),
// position = where the NEXT row would go, frames = frames since reset.  The table is never trusted with an address: the
// stream is clamped into [0, S), counts are cut to max_count (to W for a read), positions are masked by R - 1, and every
// access to the packed rows and the track is bounded by M.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cer_internal.h"

namespace cer {

constexpr int DS_LANES = 64, DS_MAXC = 16;
constexpr long long DS_NEVER = 0x7fffffffffffffffLL;

// numpy.argmax: the first NaN if there is one, otherwise the first maximum (as in eval_metrics.hip).
template <class T>
__device__ __forceinline__ int ds_argmax_first(const T *z, int n) {
    int b = 0;
    T m = z[0];
    if (m != m) return 0;
    for (int c = 1; c < n; ++c) {
        const T x = z[c];
        if (x != x) return c;
        if (x > m) { m = x; b = c; }
    }
    return b;
}

struct ds_lds {
    float z[DS_LANES][DS_MAXC + 1];                       // the tile's rows (padded: lanes over rows write, lanes over classes read)
    float den[DS_LANES];
    int pred[DS_LANES];
    long long v[DS_LANES][DS_MAXC], f[DS_LANES][DS_MAXC];   // the accumulators as they stand after each row of the tile
    double ml[DS_LANES][DS_MAXC], mp[DS_LANES][DS_MAXC];    // sum / n
};

// What lane c carries along its chain.
struct ds_acc {
    long long v, f;
    double a, b;
};

struct ds_dims {
    int C, nc, classify;
};

// Rows of a push: packed row off + j, a row outside [0, M) reads as 0.
struct ds_packed {
    const float *rows;
    long long off;
    int M, C;
    __device__ __forceinline__ float operator()(int j, int c) const {
        const long long m = off + j;
        return m >= 0 && m < M ? rows[(size_t)m * C + c] : 0.f;
    }
};

// Rows of a window: slot (pos0 + j) & (R - 1) of one stream's ring.
struct ds_ring {
    const float *ring;
    unsigned pos0;
    int R, C;
    __device__ __forceinline__ float operator()(int j, int c) const {
        return ring[(size_t)((pos0 + (unsigned)j) & (unsigned)(R - 1)) * C + c];
    }
};

// The three decisions and the two means of tile row i from what the chains left in LDS.  dec / means may be null.
__device__ __forceinline__ void ds_decide(const ds_lds &L, int i, const ds_dims &d, int *dec, float *means) {
    if (d.classify && dec) {
        int pv = 0;
        for (int c = 1; c < d.nc; ++c)
            if (L.v[i][c] > L.v[i][pv] || (L.v[i][c] == L.v[i][pv] && L.f[i][c] < L.f[i][pv])) pv = c;
        dec[0] = pv;
        dec[1] = ds_argmax_first(L.ml[i], d.nc);
        dec[2] = ds_argmax_first(L.mp[i], d.nc);
    }
    if (means)
        for (int c = 0; c < d.C; ++c) {
            means[c] = (float)L.ml[i][c];
            means[d.C + c] = d.classify ? (float)L.mp[i][c] : 0.f;
        }
}

// Lane c leaves its accumulators after row i of the tile, n frames in all.
__device__ __forceinline__ void ds_leave(ds_lds &L, int i, int c, const ds_acc &acc, long long n) {
    L.v[i][c] = acc.v;
    L.f[i][c] = acc.f;
    L.ml[i][c] = acc.a / (double)n;
    L.mp[i][c] = acc.b / (double)n;
}

// The chains over `count` rows of `src` in time order, row j being frame n0 + j (since reset, or of the window).  With
// `every_row`, row j's decisions go to track[3 j ..] and its means to tmeans[2 C j ..] when the packed row toff + j lies in
// [0, M) (either may be null).  Every lane of the block calls this.
template <class Src>
__device__ __forceinline__ void ds_run(const Src &src, int count, unsigned long long n0, const ds_dims &d, ds_acc &acc, ds_lds &L,
                                       bool every_row, long long toff, int M, int *track, float *tmeans) {
    const int lane = threadIdx.x;
    for (int t0 = 0; t0 < count; t0 += DS_LANES) {
        const int nt = min(DS_LANES, count - t0);
        if (lane < nt) {
            for (int k = 0; k < d.C; ++k) L.z[lane][k] = src(t0 + lane, k);
            if (d.classify) {
                float den = 0.f;
                for (int k = 0; k < d.nc; ++k) den += expf(L.z[lane][k]);
                L.den[lane] = den;
                L.pred[lane] = ds_argmax_first(L.z[lane], d.nc);
            }
        }
        __syncthreads();
        if (lane < d.C) {
            const bool cls = d.classify && lane < d.nc;
            for (int i = 0; i < nt; ++i) {
                const float z = L.z[i][lane];
                acc.a += (double)z;
                if (cls) {
                    acc.b += (double)(expf(z) / L.den[i]);
                    if (L.pred[i] == lane) {
                        acc.v += 1;
                        if (acc.f == DS_NEVER) acc.f = (long long)(n0 + (unsigned long long)(t0 + i));
                    }
                }
                if (every_row) ds_leave(L, i, lane, acc, (long long)(n0 + (unsigned long long)(t0 + i) + 1ull));
            }
        }
        __syncthreads();
        if (every_row && lane < nt) {
            const long long m = toff + t0 + lane;
            if (m >= 0 && m < M) ds_decide(L, lane, d, track ? track + (size_t)m * 3 : nullptr, tmeans ? tmeans + (size_t)m * 2 * d.C : nullptr);
        }
    }
}

// The decisions of the accumulators as they stand after n frames: lane 0 writes them.  Every lane of the block calls this.
__device__ __forceinline__ void ds_final(const ds_acc &acc, long long n, const ds_dims &d, ds_lds &L, int *dec, float *means) {
    __syncthreads();                                   // the last tile's readers are done with L
    if (threadIdx.x < d.C) ds_leave(L, 0, threadIdx.x, acc, n);
    __syncthreads();
    if (threadIdx.x == 0) ds_decide(L, 0, d, dec, means);
}

struct ds_args {
    const float *rows;
    const int *seg;
    long long *votes, *first;
    double *slog, *sprob;
    float *zring;
    int *track;
    float *tmeans;
    int A, S, M, max_count, W, R;
    ds_dims d;
};

struct ds_segment {
    int s, count, pos;
    long long off;
    unsigned long long n;
};

__device__ __forceinline__ ds_segment ds_read_segment(const int *seg, int A, int a, int S, int max_count) {
    ds_segment g;
    g.s = min(max(seg[a], 0), S - 1);
    g.count = min(max(seg[A + a], 0), max_count);
    g.off = seg[2 * A + a];
    g.pos = seg[3 * A + a];
    g.n = (unsigned long long)(unsigned)seg[4 * A + a] | ((unsigned long long)(unsigned)seg[5 * A + a] << 32);
    return g;
}

__device__ __forceinline__ ds_acc ds_load(const ds_args &p, int s, int c) {
    ds_acc acc = {0, DS_NEVER, 0.0, 0.0};
    if (c < p.d.C) {
        const size_t at = (size_t)s * p.d.C + c;
        acc.a = p.slog[at];
        if (p.d.classify) { acc.v = p.votes[at]; acc.f = p.first[at]; acc.b = p.sprob[at]; }
    }
    return acc;
}

// The rows of the window that ends with the frame at ring position `last` (n frames since reset, that one included).
__device__ __forceinline__ int ds_window_rows(unsigned long long n, int W) {
    return (long long)n < 1 ? 1 : (n > (unsigned long long)W ? W : (int)n);
}

__global__ __launch_bounds__(DS_LANES) void decision_stream_push_kernel(ds_args p) {
    __shared__ ds_lds L;
    const ds_segment g = ds_read_segment(p.seg, p.A, blockIdx.x, p.S, p.max_count);
    const int lane = threadIdx.x, C = p.d.C;
    const ds_packed packed = {p.rows, g.off, p.M, C};
    if (p.W == 0) {   // whole-stream: continue the chains
        ds_acc acc = ds_load(p, g.s, lane);
        ds_run(packed, g.count, g.n, p.d, acc, L, p.track || p.tmeans, g.off, p.M, p.track, p.tmeans);
        if (lane < C && g.count > 0) {
            const size_t at = (size_t)g.s * C + lane;
            p.slog[at] = acc.a;
            if (p.d.classify) { p.votes[at] = acc.v; p.first[at] = acc.f; p.sprob[at] = acc.b; }
        }
        return;
    }
    // window: the new rows go into the ring; with a track, each new row's window is walked from its oldest row
    float *ring = p.zring + (size_t)g.s * p.R * C;
    for (int idx = lane; idx < g.count * C; idx += DS_LANES) {
        const int i = idx / C, c = idx - i * C;
        ring[(size_t)(((unsigned)g.pos + (unsigned)i) & (unsigned)(p.R - 1)) * C + c] = packed(i, c);
    }
    if (!p.track && !p.tmeans) return;
    __syncthreads();                                   // the block's own ring writes, before it reads them back
    for (int i = 0; i < g.count; ++i) {
        const long long m = g.off + i;
        const int nw = ds_window_rows(g.n + (unsigned long long)i + 1ull, p.W);
        const ds_ring win = {ring, (unsigned)g.pos + (unsigned)i + 1u - (unsigned)nw, p.R, C};
        ds_acc acc = {0, DS_NEVER, 0.0, 0.0};
        ds_run(win, nw, 0ull, p.d, acc, L, false, 0, 0, nullptr, nullptr);
        const bool in = m >= 0 && m < p.M;
        ds_final(acc, nw, p.d, L, in && p.track ? p.track + (size_t)m * 3 : nullptr,
                 in && p.tmeans ? p.tmeans + (size_t)m * 2 * C : nullptr);
        __syncthreads();                               // lane 0 is done with L before the next window's tiles
    }
}

// One block per stream: segment s of the table describes stream s (its own stream field is not read).
__global__ __launch_bounds__(DS_LANES) void decision_stream_read_kernel(ds_args p, int *dec, float *means) {
    __shared__ ds_lds L;
    const int s = blockIdx.x, lane = threadIdx.x, C = p.d.C;
    const ds_segment g = ds_read_segment(p.seg, p.A, s, p.S, max(p.W, 1));
    int *dout = dec ? dec + (size_t)s * 3 : nullptr;
    float *mout = means + (size_t)s * 2 * C;
    if (g.n == 0ull || (p.W > 0 && g.count == 0)) {   // no frame yet: no decision, and 0 / 0 for the means
        if (lane == 0 && dout) dout[0] = dout[1] = dout[2] = -1;
        if (lane < 2 * C) mout[lane] = __builtin_nanf("");
        return;
    }
    if (p.W == 0) {
        const ds_acc acc = ds_load(p, s, lane);
        ds_final(acc, (long long)g.n, p.d, L, dout, mout);
        return;
    }
    const ds_ring win = {p.zring + (size_t)s * p.R * C, (unsigned)g.pos - (unsigned)g.count, p.R, C};
    ds_acc acc = {0, DS_NEVER, 0.0, 0.0};
    ds_run(win, g.count, 0ull, p.d, acc, L, false, 0, 0, nullptr, nullptr);
    ds_final(acc, g.count, p.d, L, dout, mout);
}

#define DS_REFUSE(...) return cer_set_error(CER_ERR_INVALID_ARG, __VA_ARGS__)

// What both entries refuse, by the descriptor alone.
static int ds_check(const char *entry, const cer_decision_stream_desc *d) {
    if (!d) DS_REFUSE("%s: null pointer", entry);
    if (d->C < 2 || d->C > DS_MAXC) DS_REFUSE("%s: C = %d outside 2 .. %d", entry, d->C, DS_MAXC);
    if (d->S < 1 || d->M < 1 || d->max_count < 1) DS_REFUSE("%s: streams, rows and max_count must be >= 1", entry);
    if (d->W < 0) DS_REFUSE("%s: window W = %d is negative", entry, d->W);
    if (d->W > 0) {
        if (d->R < 1 || (d->R & (d->R - 1)) != 0) DS_REFUSE("%s: ring length R = %d is not a power of two up to 2^30", entry, d->R);
        if ((long long)d->W + d->max_count > d->R)
            DS_REFUSE("%s: a window of %d frames plus %d new ones exceed R = %d", entry, d->W, d->max_count, d->R);
    }
    if (d->drop_last && d->C < 3) DS_REFUSE("%s: drop_last leaves fewer than two of C = %d classes", entry, d->C);
    if (d->drop_last && !d->classify) DS_REFUSE("%s: drop_last without classification", entry);
    return CER_OK;
}

static bool ds_state_null(const cer_decision_stream_desc *d, const void *votes, const void *first, const void *slog,
                          const void *sprob, const void *zring) {
    if (d->W > 0) return !zring;
    return !slog || (d->classify && (!votes || !first || !sprob));
}

static ds_dims ds_dims_of(const cer_decision_stream_desc *d) {
    return {d->C, d->drop_last ? d->C - 1 : d->C, d->classify ? 1 : 0};
}

}  // namespace cer

using namespace cer;

extern "C" int cer_decision_stream_push(const cer_decision_stream_desc *d, const float *rows, const int32_t *segments,
                                        int num_segments, long long *votes, long long *first, double *slog, double *sprob,
                                        float *zring, int32_t *track, float *track_means, void *stream) {
    if (int rc = ds_check("decision_stream_push", d)) return rc;
    if (!rows || !segments || ds_state_null(d, votes, first, slog, sprob, zring)) DS_REFUSE("decision_stream_push: null pointer");
    if (num_segments < 1) DS_REFUSE("decision_stream_push: %d segments", num_segments);
    if (track && !d->classify) DS_REFUSE("decision_stream_push: a decision track without classification");
    ds_args p = {rows, segments, votes, first, slog, sprob, zring, track, track_means, num_segments, d->S, d->M, d->max_count,
                 d->W, d->W > 0 ? d->R : 1, ds_dims_of(d)};
    CER_LAUNCH(decision_stream_push_kernel, dim3(num_segments), dim3(DS_LANES), 0, (hipStream_t)stream, p);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_decision_stream_read(const cer_decision_stream_desc *d, const int32_t *table, const long long *votes,
                                        const long long *first, const double *slog, const double *sprob, const float *zring,
                                        int32_t *decisions, float *means, void *stream) {
    if (int rc = ds_check("decision_stream_read", d)) return rc;
    if (!table || !means || (d->classify && !decisions) || ds_state_null(d, votes, first, slog, sprob, zring))
        DS_REFUSE("decision_stream_read: null pointer");
    ds_args p = {nullptr, table, const_cast<long long *>(votes), const_cast<long long *>(first), const_cast<double *>(slog),
                 const_cast<double *>(sprob), const_cast<float *>(zring), nullptr, nullptr, d->S, d->S, d->M, d->max_count, d->W,
                 d->W > 0 ? d->R : 1, ds_dims_of(d)};
    CER_LAUNCH(decision_stream_read_kernel, dim3(d->S), dim3(DS_LANES), 0, (hipStream_t)stream, p, d->classify ? decisions : nullptr,
               means);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}
