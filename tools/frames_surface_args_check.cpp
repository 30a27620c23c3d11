// frames_surface_args_check.cpp -- a stand-alone host program that drives the descriptor check of the six _surface entries
// (csrc/frames*.hip, surface_pixel in csrc/frames_kernel.h) with bad descriptors, pictures and extents.  Every call below must
// be refused before any GPU call, with the entry's own name at the head of cer_last_error(); the pointers handed over are never
// dereferenced.  The extent arithmetic is driven at 2^62-scale values: it must refuse them and not wrap.  Meant to be compiled
// together with the four frame translation units and cer_common.hip under the host sanitizers and run on a machine without a
// GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/frames_surface_args_check.cpp <pkg>/csrc/frames.hip <pkg>/csrc/frames_stream.hip <pkg>/csrc/frames_box.hip \
//         <pkg>/csrc/frames_affine.hip <pkg>/csrc/cer_common.hip -o frames_surface_args_check
//
// Exit status 0 and the line "ok: N refusals" when every case was refused as expected.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "cer_hip.h"

// cer_common.hip holds the error recorder under test and, next to it, one entry that asks another translation unit for
// this; nothing here calls that entry
extern "C" int cer_conv_kpad(int, int, int) { return 0; }

namespace {

int failures = 0, cases = 0;

struct Args {
    const uint8_t *frames;
    size_t bytes;
    cer_surface d;
    bool null_desc = false;
    const double *affines;
    const int32_t *tab;
    float *out;
    uint8_t *ring;
    int n = 1, H = 8, W = 8, crop = 4, Rf = 8;
};

int call(int entry, const Args &a) {
    const cer_surface *d = a.null_desc ? nullptr : &a.d;
    const int32_t *t = a.tab;
    switch (entry) {
    case 0:
        return cer_frames_transform_surface(a.frames, a.bytes, d, a.n, a.H, a.W, t, t, 3, t, t, 3, 6, a.crop, t, 1, 2, 0.5f, 0.5f,
                                            a.out, nullptr, nullptr);
    case 1:
        return cer_frames_stream_append_surface(a.frames, a.bytes, d, a.n, a.H, a.W, t, t, 3, t, t, 3, 6, a.crop, t, 2, t, t, 1, 1,
                                                a.ring, 1, a.Rf, nullptr);
    case 2:
        return cer_frames_transform_boxes_surface(a.frames, a.bytes, d, a.n, a.H, a.W, t, t, t, 16, 8, 7, 6, a.crop, t, 1, 0.5f, 0.5f,
                                                  a.out, nullptr, nullptr);
    case 3:
        return cer_frames_stream_append_boxes_surface(a.frames, a.bytes, d, a.n, a.H, a.W, t, t, t, 16, 8, 7, 6, a.crop, t, t, t, 1, 1,
                                                      a.ring, 1, a.Rf, nullptr);
    case 4:
        return cer_frames_transform_affine_surface(a.frames, a.bytes, d, a.n, a.H, a.W, a.affines, t, t, 3, 8, 8, 6, a.crop, t, 1, 0.5f,
                                                   0.5f, a.out, nullptr, nullptr);
    default:
        return cer_frames_stream_append_affine_surface(a.frames, a.bytes, d, a.n, a.H, a.W, a.affines, t, t, 3, 8, 8, 6, a.crop, t, t, t,
                                                       1, 1, a.ring, 1, a.Rf, nullptr);
    }
}

const char *const NAMES[6] = {"frames_transform_surface:",       "frames_stream_append_surface:",
                              "frames_transform_boxes_surface:", "frames_stream_append_boxes_surface:",
                              "frames_transform_affine_surface:", "frames_stream_append_affine_surface:"};

void refused(int entry, const Args &a, const char *text, const char *what, bool own_name = true) {
    ++cases;
    const int rc = call(entry, a);
    const char *msg = cer_last_error();
    if (rc == 0 || !msg || (own_name && std::strncmp(msg, NAMES[entry], std::strlen(NAMES[entry])) != 0) || !std::strstr(msg, text)) {
        std::printf("FAIL %s %s: rc = %d, message = %s\n", NAMES[entry], what, rc, msg ? msg : "(none)");
        ++failures;
    }
}

cer_surface packed(int W, int H, int bpp) {
    cer_surface d = {CER_SURFACE_PACKED, 19077, 26149, -6419, -13320, 33050, 16, {bpp, bpp}, {2, 1, 0}, 0, {0, 0}, {0, 0, 0}};
    d.pitch[0] = d.pitch[1] = (int64_t)W * bpp;
    d.frame_stride = d.pitch[0] * H;
    return d;
}

}  // namespace

int main() {
    alignas(16) static unsigned char buf[256];
    const int64_t big = (int64_t)1 << 62;
    Args good;
    good.frames = buf;
    good.d = packed(8, 8, 3);
    good.bytes = 192;
    good.affines = reinterpret_cast<const double *>(buf);
    good.tab = reinterpret_cast<const int32_t *>(buf);
    good.out = reinterpret_cast<float *>(buf);
    good.ring = buf;
    // 4:2:0 (NV12) and 4:2:2 (YUYV) descriptors of an 8 x 8 picture, tight
    cer_surface nv12 = good.d, yuyv = good.d;
    nv12.format = CER_SURFACE_YUV420;
    nv12.step[0] = 1; nv12.step[1] = 2; nv12.pos[0] = nv12.pos[1] = nv12.pos[2] = 0;
    nv12.pitch[0] = nv12.pitch[1] = 8; nv12.offset[1] = 64; nv12.offset[2] = 65; nv12.frame_stride = 96;
    yuyv.format = CER_SURFACE_YUV422;
    yuyv.step[0] = 2; yuyv.step[1] = 4; yuyv.pos[0] = 0; yuyv.pos[1] = 1; yuyv.pos[2] = 3;
    yuyv.pitch[0] = yuyv.pitch[1] = 16; yuyv.frame_stride = 128;
    for (int e = 0; e < 6; ++e) {
        Args a = good;
        a.null_desc = true; refused(e, a, "null", "descriptor"); a = good;
        a.d.format = 3; refused(e, a, "format", "format 3"); a = good;
        a.d.format = -1; refused(e, a, "format", "format -1"); a = good;
        a.d.cgu = 1 << 21; refused(e, a, "coefficient", "coefficient above 2^20"); a = good;
        a.d.cbu = -(1 << 21); refused(e, a, "coefficient", "coefficient below -2^20"); a = good;
        a.d.yoff = 256; refused(e, a, "yoff", "yoff 256"); a = good;
        a.d.yoff = -1; refused(e, a, "yoff", "yoff -1"); a = good;
        a.d.step[0] = 5; a.d.step[1] = 5; refused(e, a, "byte pattern", "5 bytes per pixel"); a = good;
        a.d.step[1] = 4; refused(e, a, "byte pattern", "two steps of a packed format"); a = good;
        a.d.pos[0] = 3; refused(e, a, "byte pattern", "R at byte 3 of 3"); a = good;
        a.d.pos[2] = -1; refused(e, a, "byte pattern", "B at byte -1"); a = good;
        a.d.pitch[1] = 25; refused(e, a, "one plane", "two pitches of a packed format"); a = good;
        a.d.offset[2] = 1; refused(e, a, "one plane", "two offsets of a packed format"); a = good;
        a.H = 0; refused(e, a, ">= 1", "empty picture"); a = good;
        a.n = 0; refused(e, a, ">= 1", "no frames"); a = good;
        a.H = 1 << 15; a.W = 1 << 15; refused(e, a, "2^29", "huge picture"); a = good;
        a.d.offset[0] = a.d.offset[1] = a.d.offset[2] = -1; refused(e, a, "negative", "negative offset"); a = good;
        a.d.pitch[0] = a.d.pitch[1] = -24; refused(e, a, "negative", "negative pitch"); a = good;
        a.d.frame_stride = -192; refused(e, a, "negative", "negative stride"); a = good;
        a.d.pitch[0] = a.d.pitch[1] = 23; refused(e, a, "below", "pitch below a row"); a = good;
        a.d.pitch[0] = a.d.pitch[1] = 0; refused(e, a, "below", "pitch 0"); a = good;
        a.d.frame_stride = 191; refused(e, a, "past frame_stride", "plane past the stride"); a = good;
        a.d.offset[0] = a.d.offset[1] = a.d.offset[2] = 1; refused(e, a, "past frame_stride", "offset pushes the plane out"); a = good;
        a.d.offset[0] = a.d.offset[1] = a.d.offset[2] = 193; refused(e, a, "past frame_stride", "offset past the stride"); a = good;
        a.bytes = 191; refused(e, a, "frames_bytes", "one frame, one byte short"); a = good;
        a.n = 2; refused(e, a, "frames_bytes", "two frames in the bytes of one"); a = good;
        a.n = 2; a.bytes = 383; refused(e, a, "frames_bytes", "two frames, one byte short"); a = good;
        a.bytes = 0; refused(e, a, "frames_bytes", "no bytes"); a = good;
        // values that would wrap if they were multiplied up
        a.d.frame_stride = big; refused(e, a, "2^40", "stride 2^62"); a = good;
        a.n = 5; a.d.frame_stride = big; a.bytes = 192; refused(e, a, "2^40", "five frames of stride 2^62: 4 * 2^62 wraps to 0"); a = good;
        a.d.pitch[0] = a.d.pitch[1] = big; refused(e, a, "2^40", "pitch 2^62"); a = good;
        a.d.offset[0] = a.d.offset[1] = a.d.offset[2] = big; refused(e, a, "2^40", "offset 2^62"); a = good;
        a.d.frame_stride = INT64_MAX; refused(e, a, "2^40", "stride INT64_MAX"); a = good;
        a.d.frame_stride = (int64_t)1 << 40; refused(e, a, "2^40", "stride 2^40"); a = good;
        a.n = 65535; a.d.frame_stride = ((int64_t)1 << 40) - 1; a.bytes = 192; refused(e, a, "frames_bytes", "65535 frames of stride 2^40 - 1");
        a = good;
        a.H = 1 << 20; a.W = 8; a.d.pitch[0] = a.d.pitch[1] = ((int64_t)1 << 40) - 1; a.d.frame_stride = ((int64_t)1 << 40) - 1;
        refused(e, a, "past frame_stride", "2^20 rows of pitch 2^40 - 1"); a = good;
        // 4:2:0
        a.d = nv12; a.bytes = 96;
        Args g420 = a;
        a.H = 7; refused(e, a, "even", "odd H"); a = g420;
        a.W = 9; refused(e, a, "even", "odd W"); a = g420;
        a.d.step[1] = 3; refused(e, a, "byte pattern", "chroma step 3"); a = g420;
        a.d.pos[1] = 1; refused(e, a, "byte pattern", "a position under 4:2:0"); a = g420;
        a.d.pitch[1] = 7; refused(e, a, "below", "chroma pitch below a row"); a = g420;
        a.d.offset[2] = 66; refused(e, a, "past frame_stride", "V one byte past the frame"); a = g420;
        a.d.offset[1] = big; refused(e, a, "2^40", "chroma offset 2^62"); a = g420;
        a.bytes = 95; refused(e, a, "frames_bytes", "one byte short"); a = g420;
        // 4:2:2
        a.d = yuyv; a.bytes = 128;
        Args g422 = a;
        a.W = 7; refused(e, a, "even", "odd W"); a = g422;
        a.d.pos[0] = 2; refused(e, a, "byte pattern", "Y0 at byte 2"); a = g422;
        a.d.pos[2] = 4; refused(e, a, "byte pattern", "V at byte 4"); a = g422;
        a.d.pitch[0] = a.d.pitch[1] = 15; refused(e, a, "below", "pitch below a row"); a = g422;
        a.bytes = 127; refused(e, a, "frames_bytes", "one byte short"); a = good;
        // what the sibling refuses is refused too (the unboxed pair in the sibling's words)
        a.crop = 7; refused(e, a, e < 2 ? "frames" : "exceeds size", "crop > size", e >= 2); a = good;
        if (e & 1) {
            a.Rf = 6; refused(e, a, "power of two", "ring of 6", e >= 2); a = good;
        }
    }
    if (failures) {
        std::printf("%d of %d cases failed\n", failures, cases);
        return 1;
    }
    std::printf("ok: %d refusals\n", cases);
    return 0;
}
