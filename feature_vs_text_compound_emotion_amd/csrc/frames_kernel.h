// frames_kernel.h -- the one frame-transform kernel behind cer_frames_transform (frames.hip) and cer_frames_stream_append
// (frames_stream.hip), and the pixel expression cer_frames_stream_gather shares with it.
//
// One path, two ways to name a frame: the kernel is a template over a small `Place` functor that says, for frame index f of the
// launch, which packed input frame it reads, which (x1, y1, flip) crop entry it takes and where an output pixel goes.  The
// band staging into LDS, the dword fast path and the generic path exist once; both passes are integer sums of non-negative
// products below 2^31, so a pixel's byte does not depend on the launch it was computed in.
#pragma once
#include <stdint.h>

#include "cer_internal.h"

namespace cer {

constexpr int FR_PREC = 32 - 8 - 2;  // Pillow's PRECISION_BITS
constexpr int FR_BAND = 8;           // output rows per block
constexpr int FR_FAST_TAPS = 13;     // horizontal taps of the dword fast path (256 -> 48: ksize 13)

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ToTorchFormatTensor + Normalize of one resized byte: the float is a pure function of the byte
__device__ __forceinline__ float frame_px(int v, float mean, float stdv) { return ((float)v / 255.0f - mean) / stdv; }

struct FramesArgs {
    const uint8_t *frames;
    const int32_t *hb, *hk, *vb, *vk;  // bounds [size][2] = (first, count), coefficients [size][ks]
    int H, W, hks, vks, size, crop, max_rows;
};

// Pixel:  size_t frame_bytes(int H, int W)                     bytes of one packed H x W frame
//         Row    row(const uint8_t *img, int W, int y)         row y of the frame at img, 0 <= y < H
//         void   get(const Row &r, int x, int (&px)[3])        R, G, B of its pixel x, 0 <= x < W: loads at x itself and
//                                                              at addresses derived from it, so a clamped x reads in bounds
struct px_rgb24 {
    static constexpr bool packed_rgb = true;  // [H][W][3] as the LDS tile wants it: staged with 16-byte copies
    struct Row {
        const uint8_t *p;
    };
    __device__ __forceinline__ size_t frame_bytes(int H, int W) const { return (size_t)H * W * 3; }
    __device__ __forceinline__ Row row(const uint8_t *img, int W, int y) const { return Row{img + (size_t)y * W * 3}; }
    __device__ __forceinline__ void get(const Row &r, int x, int (&px)[3]) const {
        const uint8_t *s = r.p + (size_t)x * 3;
        px[0] = s[0]; px[1] = s[1]; px[2] = s[2];
    }
};

// 8-bit 4:2:0, H * 3 / 2 rows of W bytes: the Y plane [H][W], then the chroma of sample (x >> 1, y >> 1) at
// uoff / voff + (y >> 1) * crow + (x >> 1) * cpx.  NV12: (H W, H W + 1, W, 2); I420: (H W, H W + H W / 4, W / 2, 1).
struct px_yuv420 {
    static constexpr bool packed_rgb = false;
    int uoff, voff, crow, cpx;
    int cy, crv, cgu, cgv, cbu, yoff;
    struct Row {
        const uint8_t *y, *u, *v;
    };
    __device__ __forceinline__ size_t frame_bytes(int H, int W) const { return (size_t)H * W / 2 * 3; }
    __device__ __forceinline__ Row row(const uint8_t *img, int W, int y) const {
        const uint8_t *c = img + (size_t)(y >> 1) * crow;
        return Row{img + (size_t)y * W, c + uoff, c + voff};
    }
    __device__ __forceinline__ void get(const Row &r, int x, int (&px)[3]) const {
        const int ci = (x >> 1) * cpx;
        const int c = cy * ((int)r.y[x] - yoff) + (1 << (CER_YUV_PREC - 1)), u = (int)r.u[ci] - 128, v = (int)r.v[ci] - 128;
        px[0] = clip8((c + crv * v) >> CER_YUV_PREC);
        px[1] = clip8((c + cgu * u + cgv * v) >> CER_YUV_PREC);
        px[2] = clip8((c + cbu * u) >> CER_YUV_PREC);
    }
};

// What the 4:2:0 entries refuse about the picture and the conversion, and the functor of what they accept.
inline int yuv420_pixel(const char *name, const cer_yuv420 *d, int H, int W, px_yuv420 *px) {
    if (!d) return cer_set_error(CER_ERR_INVALID_ARG, "%s: null pointer", name);
    if (H < 2 || W < 2 || (H & 1) || (W & 1))
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: a 4:2:0 picture needs even H and W, got %d x %d", name, H, W);
    if ((size_t)H * W > (size_t)1 << 29)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: a 4:2:0 picture of %d x %d exceeds 2^29 pixels", name, H, W);
    if (d->layout != CER_YUV_NV12 && d->layout != CER_YUV_I420)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: layout = %d is neither CER_YUV_NV12 nor CER_YUV_I420", name, d->layout);
    const int32_t k[5] = {d->cy, d->crv, d->cgu, d->cgv, d->cbu};
    for (int i = 0; i < 5; ++i)
        if (k[i] < -(1 << 20) || k[i] > (1 << 20))
            return cer_set_error(CER_ERR_INVALID_ARG, "%s: a conversion coefficient of %d lies beyond +-2^20 (int32 sums)", name, k[i]);
    if (d->yoff < 0 || d->yoff > 255) return cer_set_error(CER_ERR_INVALID_ARG, "%s: yoff = %d is outside 0 .. 255", name, d->yoff);
    const int nv12 = d->layout == CER_YUV_NV12, hw = H * W;
    *px = px_yuv420{hw, nv12 ? hw + 1 : hw + hw / 4, nv12 ? W : W / 2, nv12 ? 2 : 1, d->cy, d->crv, d->cgu, d->cgv, d->cbu, d->yoff};
    return CER_OK;
}

// A surface (cer_surface, cer_hip.h): the three bytes of pixel (x, y) lie at
//   a[y * pitch0 + x * s0 + o0],  b[(y >> ysh) * pitch1 + (x >> xsh) * s1 + o1],  c[(y >> ysh) * pitch1 + (x >> xsh) * s1 + o2]
// from the plane offsets off0, off1, off2 of a frame of `stride` bytes.  One functor for the three cases -- packed 3 / 4 bytes
// in any channel order (no shifts, the three planes are one), 4:2:0 with independent planes (NV12, NV21, I420, YV12), packed
// 4:2:2 -- because the index arithmetic is the same expression for all of them; the only branch, `convert`, is uniform over
// the launch.  Indices are 64-bit: x * 4 of a 2^29-pixel row does not fit an int.
struct px_surface {
    static constexpr bool packed_rgb = false;
    int64_t stride, pitch0, pitch1, off0, off1, off2;
    int s0, s1, o0, o1, o2, xsh, ysh, convert;
    int cy, crv, cgu, cgv, cbu, yoff;
    struct Row {
        const uint8_t *a, *b, *c;
    };
    __device__ __forceinline__ size_t frame_bytes(int, int) const { return (size_t)stride; }
    __device__ __forceinline__ Row row(const uint8_t *img, int, int y) const {
        const uint8_t *c = img + (size_t)(y >> ysh) * (size_t)pitch1;
        return Row{img + (size_t)off0 + (size_t)y * (size_t)pitch0, c + (size_t)off1, c + (size_t)off2};
    }
    __device__ __forceinline__ void get(const Row &r, int x, int (&px)[3]) const {
        const size_t ci = (size_t)(x >> xsh) * s1;
        const int a = r.a[(size_t)x * s0 + o0], b = r.b[ci + o1], c3 = r.c[ci + o2];
        if (convert) {  // the expression of px_yuv420::get
            const int c = cy * (a - yoff) + (1 << (CER_YUV_PREC - 1)), u = b - 128, v = c3 - 128;
            px[0] = clip8((c + crv * v) >> CER_YUV_PREC);
            px[1] = clip8((c + cgu * u + cgv * v) >> CER_YUV_PREC);
            px[2] = clip8((c + cbu * u) >> CER_YUV_PREC);
        } else {
            px[0] = a; px[1] = b; px[2] = c3;
        }
    }
};

// What the _surface entries refuse about the descriptor, the picture and the extent of `frames`, and the functor of what they
// accept.  Everything is compared or divided, never multiplied up, so no value can wrap: after this check
// (n_frames - 1) * stride + the end of every plane <= frames_bytes, which is the bound of every address px_surface forms from
// a frame below n_frames and a pixel inside the picture.
inline int surface_pixel(const char *name, const cer_surface *d, size_t frames_bytes, int n_frames, int H, int W, px_surface *px) {
#define SP_REFUSE(...) return cer_set_error(CER_ERR_INVALID_ARG, __VA_ARGS__)
    if (!d) SP_REFUSE("%s: null pointer (surface)", name);
    if (d->format != CER_SURFACE_PACKED && d->format != CER_SURFACE_YUV420 && d->format != CER_SURFACE_YUV422)
        SP_REFUSE("%s: format = %d is not a CER_SURFACE_ format", name, d->format);
    const int32_t k[5] = {d->cy, d->crv, d->cgu, d->cgv, d->cbu};
    for (int i = 0; i < 5; ++i)
        if (k[i] < -(1 << 20) || k[i] > (1 << 20))
            SP_REFUSE("%s: a conversion coefficient of %d lies beyond +-2^20 (int32 sums)", name, k[i]);
    if (d->yoff < 0 || d->yoff > 255) SP_REFUSE("%s: yoff = %d is outside 0 .. 255", name, d->yoff);
    const bool p = d->format == CER_SURFACE_PACKED, c420 = d->format == CER_SURFACE_YUV420;
    if (n_frames < 1 || H < 1 || W < 1) SP_REFUSE("%s: frames and the picture's H and W must be >= 1", name);
    if (c420 ? ((H | W) & 1) != 0 : (!p && (W & 1)))
        SP_REFUSE("%s: a %s picture needs even %s, got %d x %d", name, c420 ? "4:2:0" : "4:2:2", c420 ? "H and W" : "W", H, W);
    if ((size_t)H * W > (size_t)1 << 29) SP_REFUSE("%s: a picture of %d x %d exceeds 2^29 pixels", name, H, W);
    // the byte pattern of the format
    const int32_t *s = d->step, *o = d->pos;
    bool ok;
    if (p) ok = (s[0] == 3 || s[0] == 4) && s[1] == s[0] && o[0] >= 0 && o[0] < s[0] && o[1] >= 0 && o[1] < s[0] && o[2] >= 0 && o[2] < s[0];
    else if (c420) ok = s[0] == 1 && (s[1] == 1 || s[1] == 2) && o[0] == 0 && o[1] == 0 && o[2] == 0;
    else ok = s[0] == 2 && s[1] == 4 && (o[0] == 0 || o[0] == 1) && o[1] >= 0 && o[1] < 4 && o[2] >= 0 && o[2] < 4;
    if (!ok)
        SP_REFUSE("%s: step = (%d, %d), pos = (%d, %d, %d) is not a byte pattern of format %d", name, s[0], s[1], o[0], o[1], o[2],
                  d->format);
    const int64_t lim = (int64_t)1 << 40;
    const int64_t v[6] = {d->frame_stride, d->pitch[0], d->pitch[1], d->offset[0], d->offset[1], d->offset[2]};
    for (int i = 0; i < 6; ++i) {
        if (v[i] < 0) SP_REFUSE("%s: a negative offset, pitch or frame_stride (%lld)", name, (long long)v[i]);
        if (v[i] >= lim) SP_REFUSE("%s: an offset, pitch or frame_stride of %lld is 2^40 or more", name, (long long)v[i]);
    }
    if (!c420 && (d->pitch[1] != d->pitch[0] || d->offset[1] != d->offset[0] || d->offset[2] != d->offset[0]))
        SP_REFUSE("%s: a packed format has one plane: its pitches and its offsets must be equal", name);
    // rows, nominal bytes of a row (what the pitch must cover) and bytes a row is read over, per plane
    const int64_t rows[3] = {H, c420 ? H / 2 : H, c420 ? H / 2 : H};
    const int64_t pitch[3] = {d->pitch[0], d->pitch[1], d->pitch[1]};
    const int64_t need[3] = {(int64_t)W * s[0], c420 ? (int64_t)(W / 2) * s[1] : (int64_t)W * s[0], c420 ? (int64_t)(W / 2) * s[1] : (int64_t)W * s[0]};
    const int64_t used[3] = {need[0], c420 ? (int64_t)(W / 2 - 1) * s[1] + 1 : need[0], c420 ? (int64_t)(W / 2 - 1) * s[1] + 1 : need[0]};
    int64_t extent = 0;
    for (int i = 0; i < 3; ++i) {
        if (pitch[i] < need[i])
            SP_REFUSE("%s: a pitch of %lld is below the %lld bytes of a row", name, (long long)pitch[i], (long long)need[i]);
        // offset + (rows - 1) * pitch + used <= frame_stride, without forming the product
        const int64_t room = d->frame_stride - d->offset[i] - used[i];
        if (d->offset[i] > d->frame_stride || used[i] > d->frame_stride - d->offset[i] || (rows[i] > 1 && pitch[i] > room / (rows[i] - 1)))
            SP_REFUSE("%s: the plane at offset %lld (%lld rows, pitch %lld) ends past frame_stride = %lld", name,
                      (long long)d->offset[i], (long long)rows[i], (long long)pitch[i], (long long)d->frame_stride);
        const int64_t end = d->offset[i] + (rows[i] - 1) * pitch[i] + used[i];  // <= frame_stride < 2^40
        extent = end > extent ? end : extent;
    }
    if ((uint64_t)extent > (uint64_t)frames_bytes ||
        (n_frames > 1 && (uint64_t)d->frame_stride > ((uint64_t)frames_bytes - (uint64_t)extent) / (uint64_t)(n_frames - 1)))
        SP_REFUSE("%s: %d frames of stride %lld and extent %lld exceed frames_bytes = %zu", name, n_frames, (long long)d->frame_stride,
                  (long long)extent, frames_bytes);
#undef SP_REFUSE
    *px = px_surface{d->frame_stride, d->pitch[0], d->pitch[1], d->offset[0], d->offset[1], d->offset[2],
                     s[0], s[1], o[0], o[1], o[2], p ? 0 : 1, c420 ? 1 : 0, p ? 0 : 1,
                     d->cy, d->crv, d->cgu, d->cgv, d->cbu, d->yoff};
    return CER_OK;
}

// LDS of one block: the staged input rows, the horizontally resampled rows, the two coefficient tiles
inline size_t frames_lds_bytes(int max_band_rows, int W, int crop) {
    return (((size_t)max_band_rows * W * 3 + 15) & ~(size_t)15) + (((size_t)max_band_rows * crop * 3 + 15) & ~(size_t)15) +
           (size_t)(crop + FR_BAND) * 16 * sizeof(int32_t);
}

// Place:  int  source(int f)                                   the packed input frame that launch frame f reads
//         void entry(int f, int &x1, int &y1, int &flip)       its crop entry
//         void store(int f, int c, int yy, int xc, int v)      where byte v of channel c, cropped row yy, column xc goes
template <class Place, class Pixel>
__global__ __launch_bounds__(256) void frames_transform_kernel(FramesArgs p, Place place, Pixel pix) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fr_smem[];
    const int f = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    int x1, y1, flip;
    place.entry(f, x1, y1, flip);
    const int yy0 = band * FR_BAND, yy1 = min(p.crop, yy0 + FR_BAND);
    const int r0 = p.vb[2 * (y1 + yy0)];
    const int r1 = p.vb[2 * (y1 + yy1 - 1)] + p.vb[2 * (y1 + yy1 - 1) + 1];  // one past the last input row
    const int rows = r1 - r0, rowb = p.W * 3;
    uint8_t *src = fr_smem;                                        // [rows][W*3]
    uint8_t *tmp = fr_smem + (((size_t)p.max_rows * rowb + 15) & ~(size_t)15);  // [rows][crop][3]
    // coefficient rows of this block's columns / output rows, zero-padded to 16 taps (13 dependent global loads per
    // output were the bulk of the kernel's memory instructions)
    int32_t *hkl = reinterpret_cast<int32_t *>(tmp + (((size_t)p.max_rows * p.crop * 3 + 15) & ~(size_t)15));  // [crop][16]
    int32_t *vkl = hkl + p.crop * 16;                                                                          // [FR_BAND][16]
    const bool ktab = p.hks <= 16 && p.vks <= 16;
    if (ktab) {
        for (int i = tid; i < p.crop * 16; i += 256) {
            const int xc = i >> 4, j = i & 15;
            const int col = x1 + (flip ? p.crop - 1 - xc : xc);
            hkl[i] = j < p.hks ? p.hk[(size_t)col * p.hks + j] : 0;
        }
        for (int i = tid; i < (yy1 - yy0) * 16; i += 256) {
            const int ry = i >> 4, j = i & 15;
            vkl[i] = j < p.vks ? p.vk[(size_t)(y1 + yy0 + ry) * p.vks + j] : 0;
        }
    }
    if constexpr (Pixel::packed_rgb) {
        const uint8_t *g = p.frames + ((size_t)place.source(f) * p.H + r0) * rowb;
        const size_t nbytes = (size_t)rows * rowb;
        if (((reinterpret_cast<uintptr_t>(g) | nbytes) & 15) == 0) {
            // four loads in flight per thread before the first LDS store (a load-store-per-iteration loop serialises the
            // HBM latency: one band is only ~10 loads per thread).  Every load is issued, at an index clamped into the
            // band, and only the stores are predicated: values that are loaded under a condition end up in scratch memory.
            const uint4 *g4 = reinterpret_cast<const uint4 *>(g);
            uint4 *s4 = reinterpret_cast<uint4 *>(src);
            const size_t n16 = nbytes / 16;
            for (size_t i = tid; i < n16; i += 4 * 256) {
                uint4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = g4[min(i + u * 256, n16 - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i + u * 256 < n16) s4[i + u * 256] = v[u];
            }
        } else {
            for (size_t i = tid; i < nbytes; i += 256) src[i] = g[i];
        }
    } else {
        // the same tile, converted on the way in: one thread per pixel of the band's rows, four in flight.  Every load is
        // issued, at a pixel clamped into the band (and its row into the frame), and only the LDS stores are predicated.
        const uint8_t *img = p.frames + (size_t)place.source(f) * pix.frame_bytes(p.H, p.W);
        const int npx = rows * p.W;
        for (int i = tid; i < npx; i += 4 * 256) {
            int v[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(i + u * 256, npx - 1);
                const int r = q / p.W, x = q - r * p.W;
                pix.get(pix.row(img, p.W, min(r0 + r, p.H - 1)), x, v[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + u * 256 < npx) {
                    uint8_t *d = src + (size_t)(i + u * 256) * 3;
                    d[0] = (uint8_t)v[u][0]; d[1] = (uint8_t)v[u][1]; d[2] = (uint8_t)v[u][2];
                }
        }
    }
    __syncthreads();
    // horizontal pass, column already flipped
    const int per_row = p.crop * 3;
    if (((rowb & 3) == 0) && p.hks <= FR_FAST_TAPS && ktab) {
        // fast path: one thread per (row, cropped column) does all three channels.  Its taps are the 3*cnt <= 39
        // CONSECUTIVE bytes from xmin*3 of the row: 11 aligned dword LDS reads, v_alignbyte to drop the per-lane
        // misalignment, after which every (tap, channel) byte sits at a compile-time position.
        for (int i = tid; i < rows * p.crop; i += 256) {
            const int r = i / p.crop, xc = i - r * p.crop;
            const int col = x1 + (flip ? p.crop - 1 - xc : xc);
            const int xmin = p.hb[2 * col];
            const int4 *k4 = reinterpret_cast<const int4 *>(hkl + xc * 16);
            const int4 ka = k4[0], kb = k4[1], kc = k4[2], kd = k4[3];
            const int k[16] = {ka.x, ka.y, ka.z, ka.w, kb.x, kb.y, kb.z, kb.w, kc.x, kc.y, kc.z, kc.w, kd.x, kd.y, kd.z, kd.w};
            const int b0 = r * rowb + xmin * 3, mis = b0 & 3;
            const uint32_t *w32 = reinterpret_cast<const uint32_t *>(src + (b0 - mis));
            constexpr int NW32 = (FR_FAST_TAPS * 3 + 3 + 3) / 4;  // dwords that cover 39 bytes at any misalignment
            uint32_t raw[NW32 + 1];
            const int last = (rows * rowb - (b0 - mis) + 3) / 4;  // dwords available before the end of the staged rows
#pragma unroll
            for (int q = 0; q <= NW32; ++q) raw[q] = q < last ? w32[q] : 0u;
            uint32_t al[NW32];
#pragma unroll
            for (int q = 0; q < NW32; ++q) al[q] = __builtin_amdgcn_alignbyte(raw[q + 1], raw[q], (uint32_t)mis);
            int a0 = 1 << (FR_PREC - 1), a1 = a0, a2 = a0;
#pragma unroll
            for (int j = 0; j < FR_FAST_TAPS; ++j) {
                const int kj = k[j];  // zero beyond the tap count
                a0 += (int)((al[(3 * j + 0) >> 2] >> (8 * ((3 * j + 0) & 3))) & 255u) * kj;
                a1 += (int)((al[(3 * j + 1) >> 2] >> (8 * ((3 * j + 1) & 3))) & 255u) * kj;
                a2 += (int)((al[(3 * j + 2) >> 2] >> (8 * ((3 * j + 2) & 3))) & 255u) * kj;
            }
            uint8_t *t = tmp + (size_t)i * 3;
            t[0] = (uint8_t)clip8(a0 >> FR_PREC);
            t[1] = (uint8_t)clip8(a1 >> FR_PREC);
            t[2] = (uint8_t)clip8(a2 >> FR_PREC);
        }
    } else {
        for (int i = tid; i < rows * per_row; i += 256) {  // generic: (row, cropped column, channel), byte reads
            const int r = i / per_row, q = i - r * per_row;
            const int xc = q / 3, c = q - xc * 3;
            const int col = x1 + (flip ? p.crop - 1 - xc : xc);
            const int xmin = p.hb[2 * col], cnt = p.hb[2 * col + 1];
            const int32_t *k = p.hk + (size_t)col * p.hks;
            const uint8_t *s = src + (size_t)r * rowb + xmin * 3 + c;
            int acc = 1 << (FR_PREC - 1);
            for (int j = 0; j < cnt; ++j) acc += (int)s[3 * j] * k[j];
            tmp[i] = (uint8_t)clip8(acc >> FR_PREC);
        }
    }
    __syncthreads();
    // vertical pass; the place turns the byte into its output (ToTensor + Normalize offline, the ring slot when streamed)
    for (int i = tid; i < (yy1 - yy0) * per_row; i += 256) {
        const int ry = i / per_row, q = i - ry * per_row;
        const int c = q / p.crop, xc = q - c * p.crop;  // channel-major so that the fp32 stores coalesce
        const int yy = yy0 + ry, vy = y1 + yy;
        const int ymin = p.vb[2 * vy], cnt = p.vb[2 * vy + 1];
        const int32_t *k = ktab ? vkl + ry * 16 : p.vk + (size_t)vy * p.vks;
        const uint8_t *s = tmp + ((size_t)(ymin - r0) * p.crop + xc) * 3 + c;
        int acc = 1 << (FR_PREC - 1);
        for (int j = 0; j < cnt; ++j) acc += (int)s[(size_t)j * per_row] * k[j];
        place.store(f, c, yy, xc, clip8(acc >> FR_PREC));
    }
}

}  // namespace cer
