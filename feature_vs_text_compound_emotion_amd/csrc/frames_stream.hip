// frames_stream.hip -- the video-frame input transform (frames.hip) on raw camera frames of S live streams.
//
// State: one ring u8ring [S][Rf][crop][crop][3] of uint8, the cropped (and flipped) GroupScale result of the last Rf frames of
// every stream, NHWC.  The ring holds bytes and not floats: a frame waits about a second for its audio example, the
// normalised float is a pure function of the byte (frame_px), and a byte ring is a quarter of the memory.  The device keeps no
// counters: the host names every row of a launch by (stream, position) in two int32 arrays, positions unwrapped modulo 2^30,
// and Rf is a power of two, so `pos & (Rf - 1)` is the slot.
//
//   cer_frames_stream_append   packed raw frames [n][H][W][3] -> GroupScale -> crop -> flip -> ring slot.  This is
//                              frames_transform_kernel (frames_kernel.h) with the streamed way to name a frame: the same band
//                              staging, dword fast path and generic path as cer_frames_transform, so the same bytes.
//                              cer_frames_stream_append_yuv: the same on NV12 / I420 frames, as cer_frames_transform_yuv;
//                              cer_frames_stream_append_surface: on frames read in place, as cer_frames_transform_surface.
//   cer_frames_stream_gather   ring slots -> fp32 [M][3][crop][crop] = frame_px(byte), the tensor the visual backbone takes.
//                              HBM-bound (3 crop^2 bytes in, 12 crop^2 out per frame); no LDS: a thread turns 16 pixels (three
//                              16-byte loads) into four float4 stores per channel plane, and a block's stores of one plane
//                              are one contiguous run.  A byte path takes the shapes the 16-byte one cannot.
//
// Neither kernel trusts a table with an address: stream indices are clamped into [0, S), positions masked, the packed frame
// index bounded by n, crop entries clamped into the resized image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frames_kernel.h"

namespace cer {

constexpr int FS_POS_BITS = 30;
constexpr int FS_PX = 16;  // pixels per thread of the gather's 16-byte path

__device__ __forceinline__ int fs_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The streamed way to name a frame: row f of the table reads packed frame min(f, n - 1), takes its stream's crop entry and
// writes the byte into its stream's ring slot.
struct FramesRingPlace {
    const int32_t *crop_xyf;  // [S][3] = (x1, y1, flip)
    const int32_t *row_stream, *row_pos;
    uint8_t *ring;  // [S][Rf][crop][crop][3]
    int n_frames, S, Rf, size, crop;
    __device__ __forceinline__ int stream(int f) const { return fs_clamp(row_stream[f], S - 1); }
    __device__ __forceinline__ int source(int f) const { return min(f, n_frames - 1); }
    __device__ __forceinline__ void entry(int f, int &x1, int &y1, int &flip) const {
        const int32_t *cx = crop_xyf + (size_t)stream(f) * 3;
        x1 = fs_clamp(cx[0], size - crop); y1 = fs_clamp(cx[1], size - crop); flip = cx[2] != 0;
    }
    __device__ __forceinline__ void store(int f, int c, int yy, int xc, int v) const {
        const size_t slot = (size_t)stream(f) * Rf + (row_pos[f] & (Rf - 1));
        ring[((slot * crop + yy) * crop + xc) * 3 + c] = (uint8_t)v;
    }
};

__global__ __launch_bounds__(256) void frames_stream_gather_kernel(const uint8_t *ring, const int32_t *row_stream,
                                                                   const int32_t *row_pos, float *out, int S, int Rf, int npx,
                                                                   int wide, float mean, float stdv) {
    const int m = blockIdx.y;
    const size_t slot = (size_t)fs_clamp(row_stream[m], S - 1) * Rf + (row_pos[m] & (Rf - 1));
    const uint8_t *src = ring + slot * npx * 3;
    float *dst = out + (size_t)m * npx * 3;
    if (wide) {  // npx % 16 == 0 and both bases 16-byte aligned: so is every slot and channel plane
        const int t = blockIdx.x * 256 + threadIdx.x;
        if (t >= npx / FS_PX) return;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src) + (size_t)t * 3;
        const uint4 a = s4[0], b = s4[1], c4 = s4[2];
        const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 *d4 = reinterpret_cast<float4 *>(dst + (size_t)c * npx) + (size_t)t * (FS_PX / 4);
#pragma unroll
            for (int q = 0; q < FS_PX / 4; ++q) {
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int byte = (4 * q + i) * 3 + c;  // compile-time after unrolling
                    v[i] = frame_px((int)((w[byte >> 2] >> (8 * (byte & 3))) & 255u), mean, stdv);
                }
                d4[q] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    } else {  // one output element per thread, channel-major so that the fp32 stores coalesce
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e >= npx * 3) return;
        const int c = e / npx, px = e - c * npx;
        dst[e] = frame_px((int)src[(size_t)px * 3 + c], mean, stdv);
    }
}

static bool fs_ring_len(int v) { return v > 0 && (v & (v - 1)) == 0 && v <= (1 << FS_POS_BITS); }

}  // namespace cer

using namespace cer;

#define FS_REFUSE(...) return cer_set_error(CER_ERR_INVALID_ARG, __VA_ARGS__)

// the one body of both append entries; `pix` says how a pixel is read
template <class Pixel>
static int frames_stream_append_launch(const uint8_t *frames, int n_frames, int H, int W, const int32_t *hbounds,
                                       const int32_t *hcoef, int hksize, const int32_t *vbounds, const int32_t *vcoef, int vksize,
                                       int size, int crop, const int32_t *crop_xyf, int max_band_rows, const int32_t *row_stream,
                                       const int32_t *row_pos, int num_rows, int max_count, uint8_t *u8ring, int S, int Rf,
                                       void *stream, Pixel pix) {
    if (!frames || !hbounds || !hcoef || !vbounds || !vcoef || !crop_xyf || !row_stream || !row_pos || !u8ring)
        FS_REFUSE("frames_stream_append: null pointer");
    if (n_frames < 1 || num_rows < 1 || max_count < 1 || S < 1 || H < 1 || W < 1 || size < 1 || crop < 1 || hksize < 1 ||
        vksize < 1 || max_band_rows < 1 || max_band_rows > H)
        FS_REFUSE("frames_stream_append: frames, rows, new frames of a stream, streams and the geometry must be >= 1 "
                  "(band rows at most H)");
    if (crop > size) FS_REFUSE("frames_stream_append: crop = %d exceeds size = %d", crop, size);
    if (!fs_ring_len(Rf)) FS_REFUSE("frames_stream_append: ring length Rf = %d is not a power of two up to 2^30", Rf);
    if (max_count > Rf) FS_REFUSE("frames_stream_append: %d new frames of a stream exceed Rf = %d", max_count, Rf);
    if (num_rows > 65535 || n_frames > 65535)
        FS_REFUSE("frames_stream_append: more than 65535 frames per call (%d rows, %d frames)", num_rows, n_frames);
    const size_t lds = frames_lds_bytes(max_band_rows, W, crop);
    if (lds > 160 * 1024)
        return cer_set_error(CER_ERR_UNSUPPORTED, "frames_stream_append: a band of input rows needs %zu bytes of the 160 KiB LDS", lds);
    FramesArgs a{};
    a.frames = frames; a.hb = hbounds; a.hk = hcoef; a.vb = vbounds; a.vk = vcoef;
    a.H = H; a.W = W; a.hks = hksize; a.vks = vksize; a.size = size; a.crop = crop; a.max_rows = max_band_rows;
    const FramesRingPlace place{crop_xyf, row_stream, row_pos, u8ring, n_frames, S, Rf, size, crop};
    auto k = frames_transform_kernel<FramesRingPlace, Pixel>;
    if (lds > 64 * 1024) CER_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CER_LAUNCH(k, dim3((crop + FR_BAND - 1) / FR_BAND, num_rows), dim3(256), lds, (hipStream_t)stream, a, place, pix);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_frames_stream_append(const uint8_t *frames, int n_frames, int H, int W, const int32_t *hbounds,
                                        const int32_t *hcoef, int hksize, const int32_t *vbounds, const int32_t *vcoef,
                                        int vksize, int size, int crop, const int32_t *crop_xyf, int max_band_rows,
                                        const int32_t *row_stream, const int32_t *row_pos, int num_rows, int max_count,
                                        uint8_t *u8ring, int S, int Rf, void *stream) {
    return frames_stream_append_launch(frames, n_frames, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, size, crop,
                                       crop_xyf, max_band_rows, row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream,
                                       px_rgb24{});
}

extern "C" int cer_frames_stream_append_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                            const int32_t *hbounds, const int32_t *hcoef, int hksize, const int32_t *vbounds,
                                            const int32_t *vcoef, int vksize, int size, int crop, const int32_t *crop_xyf,
                                            int max_band_rows, const int32_t *row_stream, const int32_t *row_pos, int num_rows,
                                            int max_count, uint8_t *u8ring, int S, int Rf, void *stream) {
    px_yuv420 pix;
    const int rc = yuv420_pixel("frames_stream_append_yuv", yuv, H, W, &pix);
    if (rc != CER_OK) return rc;
    return frames_stream_append_launch(frames, n_frames, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, size, crop,
                                       crop_xyf, max_band_rows, row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream,
                                       pix);
}

extern "C" int cer_frames_stream_gather(const uint8_t *u8ring, int S, int Rf, int crop, const int32_t *row_stream,
                                        const int32_t *row_pos, int num_rows, float mean, float stdv, float *out, void *stream) {
    if (!u8ring || !row_stream || !row_pos || !out) FS_REFUSE("frames_stream_gather: null pointer");
    if (S < 1 || num_rows < 1 || crop < 1 || crop > 16384 || stdv == 0.f)
        FS_REFUSE("frames_stream_gather: streams, rows and crop (up to 16384) must be >= 1 and std non-zero");
    if (!fs_ring_len(Rf)) FS_REFUSE("frames_stream_gather: ring length Rf = %d is not a power of two up to 2^30", Rf);
    if (num_rows > 65535) FS_REFUSE("frames_stream_gather: more than 65535 frames per call (%d)", num_rows);
    const int npx = crop * crop;
    const int wide = npx % FS_PX == 0 && ((reinterpret_cast<uintptr_t>(u8ring) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const size_t threads = wide ? (size_t)npx / FS_PX : (size_t)npx * 3;
    CER_LAUNCH(frames_stream_gather_kernel, dim3(cer_blocks(threads, 256), num_rows), dim3(256), 0, (hipStream_t)stream, u8ring,
               row_stream, row_pos, out, S, Rf, npx, wide, mean, stdv);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_frames_stream_append_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface,
                                                int n_frames, int H, int W, const int32_t *hbounds, const int32_t *hcoef,
                                                int hksize, const int32_t *vbounds, const int32_t *vcoef, int vksize, int size,
                                                int crop, const int32_t *crop_xyf, int max_band_rows, const int32_t *row_stream,
                                                const int32_t *row_pos, int num_rows, int max_count, uint8_t *u8ring, int S,
                                                int Rf, void *stream) {
    px_surface pix;
    const int rc = surface_pixel("frames_stream_append_surface", surface, frames_bytes, n_frames, H, W, &pix);
    if (rc != CER_OK) return rc;
    return frames_stream_append_launch(frames, n_frames, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, size, crop,
                                       crop_xyf, max_band_rows, row_stream, row_pos, num_rows, max_count, u8ring, S, Rf, stream,
                                       pix);
}
