// frames_affine.hip -- the video-frame input transform (frames.hip) on FULL camera frames with one affine map per frame:
// PIL's Image.transform((A, A), AFFINE, a, BILINEAR) -> Image.resize(BILINEAR) -> crop -> flip, per frame, in one launch.
// A = align_size; a = six float64 coefficients that take an output pixel centre to a frame coordinate (Pillow's
// convention), so the face a similarity transform fitted to five landmarks puts on the ArcFace template comes out of
// the camera frame aligned, without a warp on the host.
//
// The warp, per output pixel (x, y) and channel, every step in float64 and none of them fused:
//   xin = x + 0.5, yin = y + 0.5;  X = (a0 xin + a1 yin) + a2;  Y = (a3 xin + a4 yin) + a5
//   outside unless X >= 0 && X < W && Y >= 0 && Y < H: the pixel is (0, 0, 0)
//   X -= 0.5, Y -= 0.5;  ix = floor(X), iy = floor(Y);  dx = X - ix, dy = Y - iy
//   x0 = clamp(ix, 0, W - 1), x1 = clamp(ix + 1, 0, W - 1), row0 = clamp(iy, 0, H - 1)
//   v1 = p[row0][x0] + (p[row0][x1] - p[row0][x0]) dx
//   v2 = 0 <= iy + 1 < H ? p[iy + 1][x0] + (p[iy + 1][x1] - p[iy + 1][x0]) dx : v1
//   byte = (uint8) trunc(v1 + (v2 - v1) dy)
// which is Pillow's affine_transform + bilinear_filter32RGB (Geometry.c, third-party, restated).  hipcc contracts a * b + c
// by default; a fused step rounds once where Pillow rounds twice and changes a byte on a small share of pixels, so
// contraction is off for this translation unit.
//
// The two resize passes are the integer sums of frames_kernel.h over the coefficient rows of side A -> size: that geometry
// is fixed per call, so the rows are launch arguments (one table, both passes: the aligned face is square), not a store.
//
// A warped pixel costs four pixel fetches and some thirty float64 operations and is a tap of up to ksize outputs in each
// direction, so the band's warped rows are computed ONCE into an LDS tile [band rows][columns the crop reads][3] and the
// horizontal pass reads the tile.  LDS is bounded by (size, crop, align_size) and does not grow with the camera frame.
//
// One path, two ways to name a frame (Place) and two ways to read a pixel (Pixel), as in frames_box.hip:
//   cer_frames_transform_affine       clip form        cer_frames_stream_append_affine       ring form
// and their _yuv siblings for NV12 / I420: the four pixels are converted, then interpolated, which is what converting the
// frame and then warping it gives; the _surface siblings do the same on frames read in place (px_surface).
//
// Nothing here trusts a table with an address.  An affine row is six doubles that are only ever compared and multiplied: a
// coordinate becomes an int after the positive-form inside test has passed (a NaN is outside), and every pixel is fetched at
// an index clamped into the frame.  The packed frame index is bounded by n_frames, the stream index clamped, the position
// masked, the crop entry clamped into the resized image, and rows, columns and tap counts are bounded by what the LDS tiles
// hold.  A wrong table gives wrong numbers, never an access outside the packed frames, the ring or the LDS.  No atomics, no
// grid sync, no flags, no scratch; a byte depends on (frame, affine, geometry) only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frames_kernel.h"

#pragma clang fp contract(off)

namespace cer {

constexpr int FA_POS_BITS = 30;
constexpr int FA_MAX_ALIGN = 1 << 14;  // far above what the LDS holds; keeps every product of sizes inside int

__device__ __forceinline__ int fa_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct FramesAffineArgs {
    const uint8_t *frames;   // [n_frames] packed frames of the Pixel's layout
    const double *affines;   // [rows][6]
    const int32_t *bounds;   // [size][2] = (first, count) of align -> size
    const int32_t *coef;     // [size][ks]
    int n_frames, H, W, size, crop, align, ks, max_rows;
};

// the warped tile [max_rows][align][3], the horizontally resampled rows [max_rows][crop][3], the coefficient rows of the
// block's columns and output rows, the bounds of its columns
inline size_t frames_affine_lds_bytes(int align, int max_rows, int ks, int crop) {
    return (((size_t)max_rows * align * 3 + 15) & ~(size_t)15) + (((size_t)max_rows * crop * 3 + 15) & ~(size_t)15) +
           (size_t)(crop + FR_BAND) * ks * sizeof(int32_t) + (size_t)crop * 2 * sizeof(int32_t);
}

// One warped pixel.  Every load is issued, at indices clamped into the frame; a pixel outside is computed at a safe
// coordinate and zeroed afterwards, so no value is loaded under a condition.
template <class Pixel>
__device__ __forceinline__ void fa_warp(const Pixel &pix, const uint8_t *img, int H, int W, const double (&a)[6], int x, int y,
                                        int (&out)[3]) {
    const double xin = (double)x + 0.5, yin = (double)y + 0.5;
    double X = (a[0] * xin + a[1] * yin) + a[2];
    double Y = (a[3] * xin + a[4] * yin) + a[5];
    const bool inside = X >= 0.0 && X < (double)W && Y >= 0.0 && Y < (double)H;
    X = inside ? X : 0.5;
    Y = inside ? Y : 0.5;
    X -= 0.5;
    Y -= 0.5;
    const double fx = floor(X), fy = floor(Y);
    const int ix = (int)fx, iy = (int)fy;  // -1 .. W - 1 and -1 .. H - 1
    const double dx = X - fx, dy = Y - fy;
    const int x0 = fa_clamp(ix, 0, W - 1), x1 = fa_clamp(ix + 1, 0, W - 1);
    const bool below = iy + 1 >= 0 && iy + 1 < H;
    const typename Pixel::Row ra = pix.row(img, W, fa_clamp(iy, 0, H - 1)), rb = pix.row(img, W, fa_clamp(iy + 1, 0, H - 1));
    int p00[3], p01[3], p10[3], p11[3];
    pix.get(ra, x0, p00);
    pix.get(ra, x1, p01);
    pix.get(rb, x0, p10);
    pix.get(rb, x1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v1 = (double)p00[c] + ((double)p01[c] - (double)p00[c]) * dx;
        const double w2 = (double)p10[c] + ((double)p11[c] - (double)p10[c]) * dx;
        const double v2 = below ? w2 : v1;
        const double v = v1 + (v2 - v1) * dy;  // within 0 .. 255: a convex combination of bytes
        out[c] = inside ? (int)v : 0;
    }
}

// Place:  int  source(int f)                                   the packed input frame that launch row f reads (any int)
//         void entry(int f, int &x1, int &y1, int &flip)       its crop entry (any ints)
//         void store(int f, int c, int yy, int xc, int v)      where byte v of channel c, cropped row yy, column xc goes
// Pixel:  px_rgb24, px_yuv420 or px_surface (frames_kernel.h), asked at clamped indices only
template <class Place, class Pixel>
__global__ __launch_bounds__(256) void frames_affine_kernel(FramesAffineArgs p, Place place, Pixel pix) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fa_smem[];
    const int f = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    int x1, y1, flip;
    place.entry(f, x1, y1, flip);
    x1 = fa_clamp(x1, 0, p.size - p.crop);
    y1 = fa_clamp(y1, 0, p.size - p.crop);
    double a[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) a[i] = p.affines[(size_t)f * 6 + i];
    const int yy0 = band * FR_BAND, yy1 = min(p.crop, yy0 + FR_BAND);
    // the rows of the aligned face this band reads and the columns the crop reads, bounded by what the tile holds
    const int r0 = fa_clamp(p.bounds[2 * (y1 + yy0)], 0, p.align - 1);
    const int r1 = p.bounds[2 * (y1 + yy1 - 1)] + p.bounds[2 * (y1 + yy1 - 1) + 1];
    const int rows = fa_clamp(r1 - r0, 1, p.max_rows);
    const int c0 = fa_clamp(p.bounds[2 * x1], 0, p.align - 1);
    const int c1 = p.bounds[2 * (x1 + p.crop - 1)] + p.bounds[2 * (x1 + p.crop - 1) + 1];
    const int cols = fa_clamp(c1 - c0, 1, p.align);
    uint8_t *src = fa_smem;                                                         // [rows][cols][3]
    uint8_t *tmp = fa_smem + (((size_t)p.max_rows * p.align * 3 + 15) & ~(size_t)15);  // [rows][crop][3]
    int32_t *hkl = reinterpret_cast<int32_t *>(tmp + (((size_t)p.max_rows * p.crop * 3 + 15) & ~(size_t)15));  // [crop][ks]
    int32_t *vkl = hkl + (size_t)p.crop * p.ks;                                                                // [FR_BAND][ks]
    int32_t *hbl = vkl + (size_t)FR_BAND * p.ks;                                                               // [crop][2]
    for (int i = tid; i < p.crop * p.ks; i += 256) {
        const int xc = i / p.ks, j = i - xc * p.ks;
        const int col = x1 + (flip ? p.crop - 1 - xc : xc);
        hkl[i] = p.coef[(size_t)col * p.ks + j];
    }
    for (int i = tid; i < (yy1 - yy0) * p.ks; i += 256) {
        const int ry = i / p.ks, j = i - ry * p.ks;
        vkl[i] = p.coef[(size_t)(y1 + yy0 + ry) * p.ks + j];
    }
    for (int xc = tid; xc < p.crop; xc += 256) {
        const int col = x1 + (flip ? p.crop - 1 - xc : xc);
        const int first = fa_clamp(p.bounds[2 * col] - c0, 0, cols - 1);
        hbl[2 * xc] = first;
        hbl[2 * xc + 1] = fa_clamp(min(p.bounds[2 * col + 1], p.ks), 0, cols - first);
    }
    // the warp: one thread per pixel of the tile
    const uint8_t *img = p.frames + (size_t)fa_clamp(place.source(f), 0, p.n_frames - 1) * pix.frame_bytes(p.H, p.W);
    for (int i = tid; i < rows * cols; i += 256) {
        const int r = i / cols, cx = i - r * cols;
        int v[3];
        fa_warp(pix, img, p.H, p.W, a, c0 + cx, r0 + r, v);
        uint8_t *d = src + (size_t)i * 3;
        d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
    }
    __syncthreads();
    // horizontal pass over the tile, column already flipped: one thread per (row, cropped column) does the three channels
    for (int i = tid; i < rows * p.crop; i += 256) {
        const int r = i / p.crop, xc = i - r * p.crop;
        const int cnt = hbl[2 * xc + 1];
        const int32_t *k = hkl + xc * p.ks;
        const uint8_t *s = src + ((size_t)r * cols + hbl[2 * xc]) * 3;
        int a0 = 1 << (FR_PREC - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < cnt; ++j) {
            const int kj = k[j];
            a0 += (int)s[3 * j] * kj;
            a1 += (int)s[3 * j + 1] * kj;
            a2 += (int)s[3 * j + 2] * kj;
        }
        uint8_t *t = tmp + (size_t)i * 3;
        t[0] = (uint8_t)clip8(a0 >> FR_PREC);
        t[1] = (uint8_t)clip8(a1 >> FR_PREC);
        t[2] = (uint8_t)clip8(a2 >> FR_PREC);
    }
    __syncthreads();
    // vertical pass, as in frames_transform_kernel; the place turns the byte into its output
    const int per_row = p.crop * 3;
    for (int i = tid; i < (yy1 - yy0) * per_row; i += 256) {
        const int ry = i / per_row, q = i - ry * per_row;
        const int c = q / p.crop, xc = q - c * p.crop;  // channel-major so that the fp32 stores coalesce
        const int yy = yy0 + ry, vy = y1 + yy;
        const int first = fa_clamp(p.bounds[2 * vy] - r0, 0, rows - 1);
        const int cnt = min(min(p.bounds[2 * vy + 1], p.ks), rows - first);
        const int32_t *k = vkl + ry * p.ks;
        const uint8_t *s = tmp + ((size_t)first * p.crop + xc) * 3 + c;
        int acc = 1 << (FR_PREC - 1);
        for (int j = 0; j < cnt; ++j) acc += (int)s[(size_t)j * per_row] * k[j];
        place.store(f, c, yy, xc, clip8(acc >> FR_PREC));
    }
}

// The offline way to name a frame: row f is packed frame f, its crop entry is its clip's, and a pixel goes to the fp32 NCHW
// output (and to the optional uint8 NHWC one).
struct AffineClipPlace {
    const int32_t *crop_xyf;  // [groups][3] = (x1, y1, flip)
    float *out;               // [n][3][crop][crop]
    uint8_t *out_u8;          // optional [n][crop][crop][3]
    int frames_per_group, crop;
    float mean, stdv;
    __device__ __forceinline__ int source(int f) const { return f; }
    __device__ __forceinline__ void entry(int f, int &x1, int &y1, int &flip) const {
        const int32_t *cx = crop_xyf + (size_t)(f / frames_per_group) * 3;
        x1 = cx[0]; y1 = cx[1]; flip = cx[2] != 0;
    }
    __device__ __forceinline__ void store(int f, int c, int yy, int xc, int v) const {
        out[(((size_t)f * 3 + c) * crop + yy) * crop + xc] = frame_px(v, mean, stdv);
        if (out_u8) out_u8[(((size_t)f * crop + yy) * crop + xc) * 3 + c] = (uint8_t)v;
    }
};

// The streamed way: row f of the row table reads packed frame f, takes its stream's crop entry and writes the byte into its
// stream's ring slot.
struct AffineRingPlace {
    const int32_t *crop_xyf;  // [S][3] = (x1, y1, flip)
    const int32_t *row_stream, *row_pos;
    uint8_t *ring;  // [S][Rf][crop][crop][3]
    int S, Rf, crop;
    __device__ __forceinline__ int stream(int f) const { return fa_clamp(row_stream[f], 0, S - 1); }
    __device__ __forceinline__ int source(int f) const { return f; }
    __device__ __forceinline__ void entry(int f, int &x1, int &y1, int &flip) const {
        const int32_t *cx = crop_xyf + (size_t)stream(f) * 3;
        x1 = cx[0]; y1 = cx[1]; flip = cx[2] != 0;
    }
    __device__ __forceinline__ void store(int f, int c, int yy, int xc, int v) const {
        const size_t slot = (size_t)stream(f) * Rf + (row_pos[f] & (Rf - 1));
        ring[((slot * crop + yy) * crop + xc) * 3 + c] = (uint8_t)v;
    }
};

static bool fa_ring_len(int v) { return v > 0 && (v & (v - 1)) == 0 && v <= (1 << FA_POS_BITS); }

}  // namespace cer

using namespace cer;

extern "C" size_t cer_frames_affine_lds_bytes(int align_size, int max_band_rows, int ksize, int crop) {
    if (align_size < 1 || max_band_rows < 1 || ksize < 1 || crop < 1) return 0;
    return frames_affine_lds_bytes(align_size, max_band_rows, ksize, crop);
}

// what all four entries refuse about the frames and the geometry; `name` is the entry's
static int fa_check(const char *name, int n_frames, int rows, int H, int W, const double *affines, int align_size, int max_band_rows,
                    int ksize, int size, int crop, size_t *lds) {
    if (n_frames < 1 || rows < 1 || H < 1 || W < 1 || size < 1 || crop < 1 || max_band_rows < 1 || ksize < 1)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: frames, rows, the geometry, band rows and tap count must be >= 1", name);
    if (crop > size) return cer_set_error(CER_ERR_INVALID_ARG, "%s: crop = %d exceeds size = %d", name, crop, size);
    if (align_size < 1 || align_size > FA_MAX_ALIGN)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: align_size = %d is outside 1 .. %d", name, align_size, FA_MAX_ALIGN);
    if (max_band_rows > align_size)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: %d band rows exceed align_size = %d", name, max_band_rows, align_size);
    if (rows > 65535 || n_frames > 65535)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: more than 65535 frames per call (%d rows, %d frames)", name, rows, n_frames);
    if ((size_t)ksize > 2 * (size_t)align_size + 3)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: %d taps exceed what align_size = %d can need", name, ksize, align_size);
    if ((size_t)H * W > (size_t)1 << 29)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: a frame of %d x %d exceeds 2^29 pixels", name, H, W);
    if (reinterpret_cast<uintptr_t>(affines) & 7)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: the affine table is not 8-byte aligned", name);
    *lds = frames_affine_lds_bytes(align_size, max_band_rows, ksize, crop);
    if (*lds > 160 * 1024)
        return cer_set_error(CER_ERR_UNSUPPORTED,
                             "%s: align_size = %d needs %zu bytes for the warped band, the resampled rows and %d-tap coefficient "
                             "rows, above the 160 KiB LDS", name, align_size, *lds, ksize);
    return CER_OK;
}

// the bodies of the clip and the ring entries; `name` is the entry's and `pix` says how a pixel is read
template <class Pixel>
static int fa_clip_launch(const char *name, const uint8_t *frames, int n_frames, int H, int W, const double *affines,
                          const int32_t *bounds, const int32_t *coef, int ksize, int align_size, int max_band_rows, int size, int crop,
                          const int32_t *crop_xyf, int frames_per_group, float mean, float stdv, float *out, uint8_t *out_u8,
                          void *stream, Pixel pix) {
    if (!frames || !affines || !bounds || !coef || !crop_xyf || !out)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: null pointer", name);
    if (frames_per_group < 1 || stdv == 0.f)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: frames per group must be >= 1 and std non-zero", name);
    size_t lds = 0;
    const int rc = fa_check(name, n_frames, n_frames, H, W, affines, align_size, max_band_rows, ksize, size, crop, &lds);
    if (rc != CER_OK) return rc;
    FramesAffineArgs a{frames, affines, bounds, coef, n_frames, H, W, size, crop, align_size, ksize, max_band_rows};
    const AffineClipPlace place{crop_xyf, out, out_u8, frames_per_group, crop, mean, stdv};
    auto k = frames_affine_kernel<AffineClipPlace, Pixel>;
    if (lds > 64 * 1024) CER_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CER_LAUNCH(k, dim3((crop + FR_BAND - 1) / FR_BAND, n_frames), dim3(256), lds, (hipStream_t)stream, a, place, pix);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

template <class Pixel>
static int fa_ring_launch(const char *name, const uint8_t *frames, int n_frames, int H, int W, const double *affines,
                          const int32_t *bounds, const int32_t *coef, int ksize, int align_size, int max_band_rows, int size, int crop,
                          const int32_t *crop_xyf, const int32_t *row_stream, const int32_t *row_pos, int num_rows, int max_count,
                          uint8_t *u8ring, int S, int Rf, void *stream, Pixel pix) {
    if (!frames || !affines || !bounds || !coef || !crop_xyf || !row_stream || !row_pos || !u8ring)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: null pointer", name);
    if (S < 1 || max_count < 1)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: streams and new frames of a stream must be >= 1", name);
    if (!fa_ring_len(Rf)) return cer_set_error(CER_ERR_INVALID_ARG, "%s: ring length Rf = %d is not a power of two up to 2^30", name, Rf);
    if (max_count > Rf) return cer_set_error(CER_ERR_INVALID_ARG, "%s: %d new frames of a stream exceed Rf = %d", name, max_count, Rf);
    size_t lds = 0;
    const int rc = fa_check(name, n_frames, num_rows, H, W, affines, align_size, max_band_rows, ksize, size, crop, &lds);
    if (rc != CER_OK) return rc;
    FramesAffineArgs a{frames, affines, bounds, coef, n_frames, H, W, size, crop, align_size, ksize, max_band_rows};
    const AffineRingPlace place{crop_xyf, row_stream, row_pos, u8ring, S, Rf, crop};
    auto k = frames_affine_kernel<AffineRingPlace, Pixel>;
    if (lds > 64 * 1024) CER_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CER_LAUNCH(k, dim3((crop + FR_BAND - 1) / FR_BAND, num_rows), dim3(256), lds, (hipStream_t)stream, a, place, pix);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_frames_transform_affine(const uint8_t *frames, int n_frames, int H, int W, const double *affines,
                                           const int32_t *bounds, const int32_t *coef, int ksize, int align_size, int max_band_rows,
                                           int size, int crop, const int32_t *crop_xyf, int frames_per_group, float mean, float stdv,
                                           float *out, uint8_t *out_u8, void *stream) {
    return fa_clip_launch("frames_transform_affine", frames, n_frames, H, W, affines, bounds, coef, ksize, align_size, max_band_rows,
                          size, crop, crop_xyf, frames_per_group, mean, stdv, out, out_u8, stream, px_rgb24{});
}

extern "C" int cer_frames_stream_append_affine(const uint8_t *frames, int n_frames, int H, int W, const double *affines,
                                               const int32_t *bounds, const int32_t *coef, int ksize, int align_size,
                                               int max_band_rows, int size, int crop, const int32_t *crop_xyf,
                                               const int32_t *row_stream, const int32_t *row_pos, int num_rows, int max_count,
                                               uint8_t *u8ring, int S, int Rf, void *stream) {
    return fa_ring_launch("frames_stream_append_affine", frames, n_frames, H, W, affines, bounds, coef, ksize, align_size,
                          max_band_rows, size, crop, crop_xyf, row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream,
                          px_rgb24{});
}

extern "C" int cer_frames_transform_affine_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                               const double *affines, const int32_t *bounds, const int32_t *coef, int ksize,
                                               int align_size, int max_band_rows, int size, int crop, const int32_t *crop_xyf,
                                               int frames_per_group, float mean, float stdv, float *out, uint8_t *out_u8,
                                               void *stream) {
    const char *name = "frames_transform_affine_yuv";
    px_yuv420 pix;
    const int rc = yuv420_pixel(name, yuv, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fa_clip_launch(name, frames, n_frames, H, W, affines, bounds, coef, ksize, align_size, max_band_rows, size, crop, crop_xyf,
                          frames_per_group, mean, stdv, out, out_u8, stream, pix);
}

extern "C" int cer_frames_stream_append_affine_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                                   const double *affines, const int32_t *bounds, const int32_t *coef, int ksize,
                                                   int align_size, int max_band_rows, int size, int crop, const int32_t *crop_xyf,
                                                   const int32_t *row_stream, const int32_t *row_pos, int num_rows, int max_count,
                                                   uint8_t *u8ring, int S, int Rf, void *stream) {
    const char *name = "frames_stream_append_affine_yuv";
    px_yuv420 pix;
    const int rc = yuv420_pixel(name, yuv, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fa_ring_launch(name, frames, n_frames, H, W, affines, bounds, coef, ksize, align_size, max_band_rows, size, crop, crop_xyf,
                          row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream, pix);
}

extern "C" int cer_frames_transform_affine_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface,
                                                   int n_frames, int H, int W, const double *affines, const int32_t *bounds,
                                                   const int32_t *coef, int ksize, int align_size, int max_band_rows, int size,
                                                   int crop, const int32_t *crop_xyf, int frames_per_group, float mean,
                                                   float stdv, float *out, uint8_t *out_u8, void *stream) {
    const char *name = "frames_transform_affine_surface";
    px_surface pix;
    const int rc = surface_pixel(name, surface, frames_bytes, n_frames, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fa_clip_launch(name, frames, n_frames, H, W, affines, bounds, coef, ksize, align_size, max_band_rows, size, crop, crop_xyf,
                          frames_per_group, mean, stdv, out, out_u8, stream, pix);
}

extern "C" int cer_frames_stream_append_affine_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface,
                                                       int n_frames, int H, int W, const double *affines, const int32_t *bounds,
                                                       const int32_t *coef, int ksize, int align_size, int max_band_rows,
                                                       int size, int crop, const int32_t *crop_xyf, const int32_t *row_stream,
                                                       const int32_t *row_pos, int num_rows, int max_count, uint8_t *u8ring,
                                                       int S, int Rf, void *stream) {
    const char *name = "frames_stream_append_affine_surface";
    px_surface pix;
    const int rc = surface_pixel(name, surface, frames_bytes, n_frames, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fa_ring_launch(name, frames, n_frames, H, W, affines, bounds, coef, ksize, align_size, max_band_rows, size, crop, crop_xyf,
                          row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream, pix);
}
