// frames_box.hip -- the video-frame input transform (frames.hip) on FULL camera frames with one integer face box per frame:
// PIL's Image.crop(box) -> Image.resize(BILINEAR) -> crop -> flip, per frame, in one launch.
//
// A box is (x0, y0, x1, y1), right and lower exclusive; the part of it outside the frame reads as 0 (Image.crop).  Frame f
// with box b gives the bytes frames_transform_kernel (frames_kernel.h) gives the contiguous zero-padded slice: the two
// Pillow passes are the same integer sums, over the coefficient rows of the box's own width and height.
//
// Geometry is per frame, so nothing about it is a launch argument: the boxes are a device table [rows][4], and the
// coefficients of EVERY side n = 1 .. max_side live in one table store, uploaded once per (size, max_side):
//   meta [max_side + 1][4] = (offset of bounds, offset of coefficients, tap count ksize, band span) of side n, offsets into
//   data;  data = for each n the bounds [size][2] = (first, count) and the coefficients [size][ksize], concatenated.
// The kernel picks the rows of the box's width for the horizontal pass and of its height for the vertical one.
//
// One path, two ways to name a frame (the idiom of frames_kernel.h): frames_box_kernel is a template over a Place.
//   cer_frames_transform_boxes       clip form: fp32 NCHW (and the optional uint8 NHWC), a crop entry per clip.
//   cer_frames_stream_append_boxes   ring form: the byte into u8ring at row_pos & (Rf - 1), row_stream clamped.
// And two ways to read a pixel (Pixel, frames_kernel.h): the _yuv siblings of both take NV12 / I420 frames and convert the
// pixels of the box, and nothing else, in registers; the _surface siblings read frames in place in any byte order and layout
// (px_surface), after surface_pixel has checked the descriptor against the bytes the caller vouches for.
//
// LDS does not grow with the camera frame: the horizontal pass reads the frame from global memory (a band of a 1024-pixel box
// would be 590 KB of staged rows) and writes an LDS tile [band rows][crop][3]; the coefficient rows of the block's columns and
// output rows sit beside it.  All three are bounded by (size, crop, max_side).
//
// Nothing here trusts a table with an address.  Box coordinates are clamped into +-2^20 before any arithmetic, width and
// height into [1, max_side]; every input pixel is fetched at an index clamped into the frame and zeroed when the unclamped
// one was outside; the packed frame index is bounded by n_frames, the stream index clamped, the position masked, the crop
// entry clamped into the resized image, row and tap counts bounded by what the LDS tiles hold.  A wrong table gives wrong
// numbers, never an access outside the packed frames, the ring or the LDS.  No atomics, no grid sync, no flags, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frames_kernel.h"

namespace cer {

constexpr int FB_COORD = 1 << 20;  // |box coordinate| bound: sums of a few of them and a side stay far inside int
constexpr int FB_POS_BITS = 30;

__device__ __forceinline__ int fb_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct FramesBoxArgs {
    const uint8_t *frames;  // [n_frames] packed frames of the Pixel's layout
    const int32_t *boxes;   // [rows][4] = (x0, y0, x1, y1)
    const int32_t *meta;    // [max_side + 1][4]
    const int32_t *data;
    int n_frames, H, W, size, crop, max_side, max_rows, max_ks;
};

inline size_t frames_box_lds_bytes(int max_rows, int crop, int max_ks) {
    return (((size_t)max_rows * crop * 3 + 15) & ~(size_t)15) + (size_t)(crop + FR_BAND) * max_ks * sizeof(int32_t) +
           (size_t)crop * 2 * sizeof(int32_t);
}

// Place:  int  source(int f)                                   the packed input frame that launch row f reads (any int)
//         void entry(int f, int &x1, int &y1, int &flip)       its crop entry (any ints)
//         void store(int f, int c, int yy, int xc, int v)      where byte v of channel c, cropped row yy, column xc goes
// Pixel:  px_rgb24, px_yuv420 or px_surface (frames_kernel.h), asked at the clamped (fx, fy) only
template <class Place, class Pixel>
__global__ __launch_bounds__(256) void frames_box_kernel(FramesBoxArgs p, Place place, Pixel pix) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fb_smem[];
    const int f = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
    int x1, y1, flip;
    place.entry(f, x1, y1, flip);
    x1 = fb_clamp(x1, 0, p.size - p.crop);
    y1 = fb_clamp(y1, 0, p.size - p.crop);
    const int32_t *bx = p.boxes + (size_t)f * 4;
    const int bx0 = fb_clamp(bx[0], -FB_COORD, FB_COORD), by0 = fb_clamp(bx[1], -FB_COORD, FB_COORD);
    const int bw = fb_clamp(fb_clamp(bx[2], -FB_COORD, FB_COORD) - bx0, 1, p.max_side);
    const int bh = fb_clamp(fb_clamp(bx[3], -FB_COORD, FB_COORD) - by0, 1, p.max_side);
    const int32_t *hm = p.meta + (size_t)bw * 4, *vm = p.meta + (size_t)bh * 4;
    const int32_t *hb = p.data + hm[0], *hk = p.data + hm[1], *vb = p.data + vm[0], *vk = p.data + vm[1];
    const int hks = hm[2], vks = vm[2];  // the rows' strides; at most max_ks taps of a row are used
    const int yy0 = band * FR_BAND, yy1 = min(p.crop, yy0 + FR_BAND);
    const int r0 = vb[2 * (y1 + yy0)];
    const int r1 = vb[2 * (y1 + yy1 - 1)] + vb[2 * (y1 + yy1 - 1) + 1];  // one past the last row of the box this band reads
    const int rows = fb_clamp(r1 - r0, 1, p.max_rows);
    uint8_t *tmp = fb_smem;                                                                                      // [rows][crop][3]
    int32_t *hkl = reinterpret_cast<int32_t *>(fb_smem + (((size_t)p.max_rows * p.crop * 3 + 15) & ~(size_t)15));  // [crop][max_ks]
    int32_t *vkl = hkl + (size_t)p.crop * p.max_ks;                                                              // [FR_BAND][max_ks]
    int32_t *hbl = vkl + (size_t)FR_BAND * p.max_ks;                                                             // [crop][2]
    const int hn = min(hks, p.max_ks), vn = min(vks, p.max_ks);
    for (int i = tid; i < p.crop * hn; i += 256) {
        const int xc = i / hn, j = i - xc * hn;
        const int col = x1 + (flip ? p.crop - 1 - xc : xc);
        hkl[xc * p.max_ks + j] = hk[(size_t)col * hks + j];
    }
    for (int i = tid; i < (yy1 - yy0) * vn; i += 256) {
        const int ry = i / vn, j = i - ry * vn;
        vkl[ry * p.max_ks + j] = vk[(size_t)(y1 + yy0 + ry) * vks + j];
    }
    for (int xc = tid; xc < p.crop; xc += 256) {
        const int col = x1 + (flip ? p.crop - 1 - xc : xc);
        hbl[2 * xc] = hb[2 * col];
        hbl[2 * xc + 1] = fb_clamp(hb[2 * col + 1], 0, hn);
    }
    __syncthreads();
    // horizontal pass from global memory, column already flipped: one thread per (box row, cropped column) does the three
    // channels.  Every load is issued, at an index clamped into the frame; a tap outside the frame gets coefficient 0 (the
    // pixel Image.crop pads with), so no value is loaded under a condition -- and the padding is RGB 0 whatever the Pixel
    // makes of the bytes it found at the clamped index.
    const uint8_t *img = p.frames + (size_t)fb_clamp(place.source(f), 0, p.n_frames - 1) * pix.frame_bytes(p.H, p.W);
    for (int i = tid; i < rows * p.crop; i += 256) {
        const int r = i / p.crop, xc = i - r * p.crop;
        const int fy = by0 + r0 + r;
        const bool yin = fy >= 0 && fy < p.H;
        const typename Pixel::Row row = pix.row(img, p.W, fb_clamp(fy, 0, p.H - 1));
        const int fx0 = bx0 + hbl[2 * xc], cnt = yin ? hbl[2 * xc + 1] : 0;  // a row outside the frame is all zero
        const int32_t *k = hkl + xc * p.max_ks;
        int a0 = 1 << (FR_PREC - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < cnt; ++j) {
            const int fx = fx0 + j;
            int px[3];
            pix.get(row, fb_clamp(fx, 0, p.W - 1), px);
            const int kj = (fx >= 0 && fx < p.W) ? k[j] : 0;
            a0 += px[0] * kj;
            a1 += px[1] * kj;
            a2 += px[2] * kj;
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
        const int first = fb_clamp(vb[2 * vy] - r0, 0, rows - 1);
        const int cnt = min(min(vb[2 * vy + 1], vn), rows - first);
        const int32_t *k = vkl + ry * p.max_ks;
        const uint8_t *s = tmp + ((size_t)first * p.crop + xc) * 3 + c;
        int acc = 1 << (FR_PREC - 1);
        for (int j = 0; j < cnt; ++j) acc += (int)s[(size_t)j * per_row] * k[j];
        place.store(f, c, yy, xc, clip8(acc >> FR_PREC));
    }
}

// The offline way to name a frame: row f is packed frame f, its crop entry is its clip's, and a pixel goes to the fp32 NCHW
// output (and to the optional uint8 NHWC one).
struct BoxClipPlace {
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
struct BoxRingPlace {
    const int32_t *crop_xyf;  // [S][3] = (x1, y1, flip)
    const int32_t *row_stream, *row_pos;
    uint8_t *ring;  // [S][Rf][crop][crop][3]
    int S, Rf, crop;
    __device__ __forceinline__ int stream(int f) const { return fb_clamp(row_stream[f], 0, S - 1); }
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

static bool fb_ring_len(int v) { return v > 0 && (v & (v - 1)) == 0 && v <= (1 << FB_POS_BITS); }

}  // namespace cer

using namespace cer;

// what both entries refuse about the frames and the table store; `name` is the entry's
static int fb_check(const char *name, int n_frames, int rows, int H, int W, int max_side, int max_band_rows, int max_ksize,
                    int size, int crop, size_t *lds) {
    if (n_frames < 1 || rows < 1 || H < 1 || W < 1 || size < 1 || crop < 1 || max_band_rows < 1 || max_ksize < 1)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: frames, rows, the geometry, band rows and tap count must be >= 1", name);
    if (crop > size) return cer_set_error(CER_ERR_INVALID_ARG, "%s: crop = %d exceeds size = %d", name, crop, size);
    if (max_side < 1 || max_side > FB_COORD)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: max_side = %d is outside 1 .. 2^20", name, max_side);
    if (max_band_rows > max_side)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: %d band rows exceed max_side = %d", name, max_band_rows, max_side);
    if (rows > 65535 || n_frames > 65535)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: more than 65535 frames per call (%d rows, %d frames)", name, rows, n_frames);
    if ((size_t)max_ksize > 2 * (size_t)max_side + 3)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: %d taps exceed what max_side = %d can need", name, max_ksize, max_side);
    *lds = frames_box_lds_bytes(max_band_rows, crop, max_ksize);
    if (*lds > 160 * 1024)
        return cer_set_error(CER_ERR_UNSUPPORTED, "%s: the band tile and coefficient rows need %zu bytes of the 160 KiB LDS", name, *lds);
    return CER_OK;
}

// the bodies of the clip and the ring entries; `name` is the entry's and `pix` says how a pixel is read
template <class Pixel>
static int fb_clip_launch(const char *name, const uint8_t *frames, int n_frames, int H, int W, const int32_t *boxes,
                          const int32_t *box_meta, const int32_t *box_data, int max_side, int max_band_rows, int max_ksize, int size,
                          int crop, const int32_t *crop_xyf, int frames_per_group, float mean, float stdv, float *out,
                          uint8_t *out_u8, void *stream, Pixel pix) {
    if (!frames || !boxes || !box_meta || !box_data || !crop_xyf || !out)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: null pointer", name);
    if (frames_per_group < 1 || stdv == 0.f)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: frames per group must be >= 1 and std non-zero", name);
    size_t lds = 0;
    const int rc = fb_check(name, n_frames, n_frames, H, W, max_side, max_band_rows, max_ksize, size, crop, &lds);
    if (rc != CER_OK) return rc;
    FramesBoxArgs a{frames, boxes, box_meta, box_data, n_frames, H, W, size, crop, max_side, max_band_rows, max_ksize};
    const BoxClipPlace place{crop_xyf, out, out_u8, frames_per_group, crop, mean, stdv};
    auto k = frames_box_kernel<BoxClipPlace, Pixel>;
    if (lds > 64 * 1024) CER_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CER_LAUNCH(k, dim3((crop + FR_BAND - 1) / FR_BAND, n_frames), dim3(256), lds, (hipStream_t)stream, a, place, pix);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

template <class Pixel>
static int fb_ring_launch(const char *name, const uint8_t *frames, int n_frames, int H, int W, const int32_t *boxes,
                          const int32_t *box_meta, const int32_t *box_data, int max_side, int max_band_rows, int max_ksize, int size,
                          int crop, const int32_t *crop_xyf, const int32_t *row_stream, const int32_t *row_pos, int num_rows,
                          int max_count, uint8_t *u8ring, int S, int Rf, void *stream, Pixel pix) {
    if (!frames || !boxes || !box_meta || !box_data || !crop_xyf || !row_stream || !row_pos || !u8ring)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: null pointer", name);
    if (S < 1 || max_count < 1)
        return cer_set_error(CER_ERR_INVALID_ARG, "%s: streams and new frames of a stream must be >= 1", name);
    if (!fb_ring_len(Rf)) return cer_set_error(CER_ERR_INVALID_ARG, "%s: ring length Rf = %d is not a power of two up to 2^30", name, Rf);
    if (max_count > Rf) return cer_set_error(CER_ERR_INVALID_ARG, "%s: %d new frames of a stream exceed Rf = %d", name, max_count, Rf);
    size_t lds = 0;
    const int rc = fb_check(name, n_frames, num_rows, H, W, max_side, max_band_rows, max_ksize, size, crop, &lds);
    if (rc != CER_OK) return rc;
    FramesBoxArgs a{frames, boxes, box_meta, box_data, n_frames, H, W, size, crop, max_side, max_band_rows, max_ksize};
    const BoxRingPlace place{crop_xyf, row_stream, row_pos, u8ring, S, Rf, crop};
    auto k = frames_box_kernel<BoxRingPlace, Pixel>;
    if (lds > 64 * 1024) CER_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CER_LAUNCH(k, dim3((crop + FR_BAND - 1) / FR_BAND, num_rows), dim3(256), lds, (hipStream_t)stream, a, place, pix);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_frames_transform_boxes(const uint8_t *frames, int n_frames, int H, int W, const int32_t *boxes,
                                          const int32_t *box_meta, const int32_t *box_data, int max_side, int max_band_rows,
                                          int max_ksize, int size, int crop, const int32_t *crop_xyf, int frames_per_group,
                                          float mean, float stdv, float *out, uint8_t *out_u8, void *stream) {
    return fb_clip_launch("frames_transform_boxes", frames, n_frames, H, W, boxes, box_meta, box_data, max_side, max_band_rows,
                          max_ksize, size, crop, crop_xyf, frames_per_group, mean, stdv, out, out_u8, stream, px_rgb24{});
}

extern "C" int cer_frames_stream_append_boxes(const uint8_t *frames, int n_frames, int H, int W, const int32_t *boxes,
                                              const int32_t *box_meta, const int32_t *box_data, int max_side,
                                              int max_band_rows, int max_ksize, int size, int crop, const int32_t *crop_xyf,
                                              const int32_t *row_stream, const int32_t *row_pos, int num_rows, int max_count,
                                              uint8_t *u8ring, int S, int Rf, void *stream) {
    return fb_ring_launch("frames_stream_append_boxes", frames, n_frames, H, W, boxes, box_meta, box_data, max_side, max_band_rows,
                          max_ksize, size, crop, crop_xyf, row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream,
                          px_rgb24{});
}

extern "C" int cer_frames_transform_boxes_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                              const int32_t *boxes, const int32_t *box_meta, const int32_t *box_data, int max_side,
                                              int max_band_rows, int max_ksize, int size, int crop, const int32_t *crop_xyf,
                                              int frames_per_group, float mean, float stdv, float *out, uint8_t *out_u8,
                                              void *stream) {
    const char *name = "frames_transform_boxes_yuv";
    px_yuv420 pix;
    const int rc = yuv420_pixel(name, yuv, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fb_clip_launch(name, frames, n_frames, H, W, boxes, box_meta, box_data, max_side, max_band_rows, max_ksize, size, crop,
                          crop_xyf, frames_per_group, mean, stdv, out, out_u8, stream, pix);
}

extern "C" int cer_frames_stream_append_boxes_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                                  const int32_t *boxes, const int32_t *box_meta, const int32_t *box_data,
                                                  int max_side, int max_band_rows, int max_ksize, int size, int crop,
                                                  const int32_t *crop_xyf, const int32_t *row_stream, const int32_t *row_pos,
                                                  int num_rows, int max_count, uint8_t *u8ring, int S, int Rf, void *stream) {
    const char *name = "frames_stream_append_boxes_yuv";
    px_yuv420 pix;
    const int rc = yuv420_pixel(name, yuv, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fb_ring_launch(name, frames, n_frames, H, W, boxes, box_meta, box_data, max_side, max_band_rows, max_ksize, size, crop,
                          crop_xyf, row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream, pix);
}

extern "C" int cer_frames_transform_boxes_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface,
                                                  int n_frames, int H, int W, const int32_t *boxes, const int32_t *box_meta,
                                                  const int32_t *box_data, int max_side, int max_band_rows, int max_ksize,
                                                  int size, int crop, const int32_t *crop_xyf, int frames_per_group, float mean,
                                                  float stdv, float *out, uint8_t *out_u8, void *stream) {
    const char *name = "frames_transform_boxes_surface";
    px_surface pix;
    const int rc = surface_pixel(name, surface, frames_bytes, n_frames, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fb_clip_launch(name, frames, n_frames, H, W, boxes, box_meta, box_data, max_side, max_band_rows, max_ksize, size, crop,
                          crop_xyf, frames_per_group, mean, stdv, out, out_u8, stream, pix);
}

extern "C" int cer_frames_stream_append_boxes_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface,
                                                      int n_frames, int H, int W, const int32_t *boxes, const int32_t *box_meta,
                                                      const int32_t *box_data, int max_side, int max_band_rows, int max_ksize,
                                                      int size, int crop, const int32_t *crop_xyf, const int32_t *row_stream,
                                                      const int32_t *row_pos, int num_rows, int max_count, uint8_t *u8ring,
                                                      int S, int Rf, void *stream) {
    const char *name = "frames_stream_append_boxes_surface";
    px_surface pix;
    const int rc = surface_pixel(name, surface, frames_bytes, n_frames, H, W, &pix);
    if (rc != CER_OK) return rc;
    return fb_ring_launch(name, frames, n_frames, H, W, boxes, box_meta, box_data, max_side, max_band_rows, max_ksize, size, crop,
                          crop_xyf, row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream, pix);
}
