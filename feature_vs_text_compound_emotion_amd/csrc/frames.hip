// frames.hip -- the video-frame input transform of the reference's Dataset on the GPU
// (/root/reference/base/dataset.py:487-508, base/transforms3D.py:33-143): uint8 frames
// [n,H,W,3] -> GroupScale(size) -> GroupRandomCrop / GroupCenterCrop(crop) ->
// GroupRandomHorizontalFlip -> ToTorchFormatTensor (/255, CHW) -> Normalize(mean, std), fused.
//
// GroupScale is torchvision Resize == PIL Image.resize(BILINEAR): an antialiased triangle filter in
// Pillow's 8-bit fixed-point arithmetic (coefficients scaled by 2^22, horizontal pass into a uint8
// intermediate, then the vertical pass).  The kernel reproduces that arithmetic bit for bit; the
// integer coefficient tables are computed by the host (frames.py) exactly as Pillow's
// precompute_coeffs does and handed over as device arrays.
//
// HBM-bound: 3*H*W bytes in, 12*crop*crop bytes out per frame.  One block owns a band of ROWS_PER_BLOCK
// output rows of one frame: the input rows the band needs are fetched ONCE with 16-byte coalesced
// loads into LDS, resampled horizontally (only the cropped columns, already flipped) into a uint8 LDS
// image, then vertically into the normalised fp32 output.
//
// cer_frames_transform_yuv is the same launch on NV12 / I420 frames: the band is converted to RGB bytes while it is staged
// (px_yuv420, frames_kernel.h), and everything after that is the code above on the same bytes.  cer_frames_transform_surface
// is the same launch again on frames read in place in any byte order and layout (px_surface, after surface_pixel's check).
#include <stdint.h>

#include "frames_kernel.h"

namespace cer {

// The offline way to name a frame: frame f of the launch is packed frame f, its crop entry is its clip's, and a pixel goes
// to the fp32 NCHW output (and to the optional uint8 NHWC one).
struct FramesClipPlace {
    const int32_t *crop_xyf;  // [groups][3] = (x1, y1, flip)
    float *out;               // [n][3][crop][crop]
    uint8_t *out_u8;          // optional [n][crop][crop][3]
    int frames_per_group, crop;
    float mean, stdv;
    __device__ __forceinline__ int source(int f) const { return f; }
    __device__ __forceinline__ void entry(int f, int &x1, int &y1, int &flip) const {
        const int32_t *cx = crop_xyf + (size_t)(f / frames_per_group) * 3;
        x1 = cx[0]; y1 = cx[1]; flip = cx[2];
    }
    __device__ __forceinline__ void store(int f, int c, int yy, int xc, int v) const {
        out[(((size_t)f * 3 + c) * crop + yy) * crop + xc] = frame_px(v, mean, stdv);
        if (out_u8) out_u8[(((size_t)f * crop + yy) * crop + xc) * 3 + c] = (uint8_t)v;
    }
};

}  // namespace cer

using namespace cer;

// the one body of both entries; `pix` says how a pixel is read
template <class Pixel>
static int frames_transform_launch(const uint8_t *frames, int n_frames, int H, int W, const int32_t *hbounds, const int32_t *hcoef,
                                   int hksize, const int32_t *vbounds, const int32_t *vcoef, int vksize, int size, int crop,
                                   const int32_t *crop_xyf, int frames_per_group, int max_band_rows, float mean, float stdv,
                                   float *out, uint8_t *out_u8, void *stream, Pixel pix) {
    if (!frames || !hbounds || !hcoef || !vbounds || !vcoef || !crop_xyf || !out)
        return cer_set_error(CER_ERR_INVALID_ARG, "frames_transform: NULL pointer");
    if (n_frames <= 0 || H <= 0 || W <= 0 || size <= 0 || crop <= 0 || crop > size || hksize <= 0 || vksize <= 0 ||
        frames_per_group <= 0 || max_band_rows <= 0 || max_band_rows > H || stdv == 0.f)
        return cer_set_error(CER_ERR_INVALID_ARG, "frames_transform: bad geometry");
    if (n_frames > 65535) return cer_set_error(CER_ERR_UNSUPPORTED, "frames_transform: more than 65535 frames per call");
    const size_t lds = frames_lds_bytes(max_band_rows, W, crop);
    if (lds > 160 * 1024) return cer_set_error(CER_ERR_UNSUPPORTED, "frames_transform: a band of input rows exceeds the 160 KiB LDS");
    FramesArgs a{};
    a.frames = frames; a.hb = hbounds; a.hk = hcoef; a.vb = vbounds; a.vk = vcoef;
    a.H = H; a.W = W; a.hks = hksize; a.vks = vksize; a.size = size; a.crop = crop; a.max_rows = max_band_rows;
    const FramesClipPlace place{crop_xyf, out, out_u8, frames_per_group, crop, mean, stdv};
    auto k = frames_transform_kernel<FramesClipPlace, Pixel>;
    if (lds > 64 * 1024) CER_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CER_LAUNCH(k, dim3((crop + FR_BAND - 1) / FR_BAND, n_frames), dim3(256), lds, (hipStream_t)stream, a, place, pix);
    CER_HIP_CHECK(hipGetLastError());
    return CER_OK;
}

extern "C" int cer_frames_transform(const uint8_t *frames, int n_frames, int H, int W, const int32_t *hbounds,
                                    const int32_t *hcoef, int hksize, const int32_t *vbounds, const int32_t *vcoef,
                                    int vksize, int size, int crop, const int32_t *crop_xyf, int frames_per_group,
                                    int max_band_rows, float mean, float stdv, float *out, uint8_t *out_u8,
                                    void *stream) {
    return frames_transform_launch(frames, n_frames, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, size, crop, crop_xyf,
                                   frames_per_group, max_band_rows, mean, stdv, out, out_u8, stream, px_rgb24{});
}

extern "C" int cer_frames_transform_yuv(const uint8_t *frames, const cer_yuv420 *yuv, int n_frames, int H, int W,
                                        const int32_t *hbounds, const int32_t *hcoef, int hksize, const int32_t *vbounds,
                                        const int32_t *vcoef, int vksize, int size, int crop, const int32_t *crop_xyf,
                                        int frames_per_group, int max_band_rows, float mean, float stdv, float *out,
                                        uint8_t *out_u8, void *stream) {
    px_yuv420 pix;
    const int rc = yuv420_pixel("frames_transform_yuv", yuv, H, W, &pix);
    if (rc != CER_OK) return rc;
    return frames_transform_launch(frames, n_frames, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, size, crop, crop_xyf,
                                   frames_per_group, max_band_rows, mean, stdv, out, out_u8, stream, pix);
}

extern "C" int cer_frames_band_rows(void) { return FR_BAND; }

extern "C" int cer_frames_transform_surface(const uint8_t *frames, size_t frames_bytes, const cer_surface *surface, int n_frames,
                                            int H, int W, const int32_t *hbounds, const int32_t *hcoef, int hksize,
                                            const int32_t *vbounds, const int32_t *vcoef, int vksize, int size, int crop,
                                            const int32_t *crop_xyf, int frames_per_group, int max_band_rows, float mean,
                                            float stdv, float *out, uint8_t *out_u8, void *stream) {
    px_surface pix;
    const int rc = surface_pixel("frames_transform_surface", surface, frames_bytes, n_frames, H, W, &pix);
    if (rc != CER_OK) return rc;
    return frames_transform_launch(frames, n_frames, H, W, hbounds, hcoef, hksize, vbounds, vcoef, vksize, size, crop, crop_xyf,
                                   frames_per_group, max_band_rows, mean, stdv, out, out_u8, stream, pix);
}
