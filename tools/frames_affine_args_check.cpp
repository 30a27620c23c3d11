// frames_affine_args_check.cpp -- a stand-alone host program that drives the argument checks of the four affine entries
// (csrc/frames_affine.hip) with bad arguments.  Every call below must be refused before any GPU call, with the entry's own
// name at the head of cer_last_error(); the pointers handed over are never dereferenced.  Meant to be compiled together with
// frames_affine.hip and cer_common.hip under the host sanitizers and run on a machine without a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/frames_affine_args_check.cpp <pkg>/csrc/frames_affine.hip <pkg>/csrc/cer_common.hip -o frames_affine_args_check
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
    const double *affines;
    const int32_t *bounds, *coef, *crop_xyf, *row_stream, *row_pos;
    float *out;
    uint8_t *ring;
    const cer_yuv420 *yuv;
    int n = 1, H = 8, W = 8, ks = 3, align = 8, span = 8, size = 6, crop = 4, group = 1, rows = 1, max_count = 1, S = 1, Rf = 8;
    float stdv = 0.5f;
};

int call(int entry, const Args &a) {
    switch (entry) {
    case 0:
        return cer_frames_transform_affine(a.frames, a.n, a.H, a.W, a.affines, a.bounds, a.coef, a.ks, a.align, a.span, a.size, a.crop,
                                           a.crop_xyf, a.group, 0.5f, a.stdv, a.out, nullptr, nullptr);
    case 1:
        return cer_frames_stream_append_affine(a.frames, a.n, a.H, a.W, a.affines, a.bounds, a.coef, a.ks, a.align, a.span, a.size,
                                               a.crop, a.crop_xyf, a.row_stream, a.row_pos, a.rows, a.max_count, a.ring, a.S, a.Rf,
                                               nullptr);
    case 2:
        return cer_frames_transform_affine_yuv(a.frames, a.yuv, a.n, a.H, a.W, a.affines, a.bounds, a.coef, a.ks, a.align, a.span,
                                               a.size, a.crop, a.crop_xyf, a.group, 0.5f, a.stdv, a.out, nullptr, nullptr);
    default:
        return cer_frames_stream_append_affine_yuv(a.frames, a.yuv, a.n, a.H, a.W, a.affines, a.bounds, a.coef, a.ks, a.align, a.span,
                                                   a.size, a.crop, a.crop_xyf, a.row_stream, a.row_pos, a.rows, a.max_count, a.ring,
                                                   a.S, a.Rf, nullptr);
    }
}

const char *const NAMES[4] = {"frames_transform_affine:", "frames_stream_append_affine:", "frames_transform_affine_yuv:",
                              "frames_stream_append_affine_yuv:"};

void refused(int entry, const Args &a, const char *text, const char *what) {
    ++cases;
    const int rc = call(entry, a);
    const char *msg = cer_last_error();
    if (rc == 0 || !msg || std::strncmp(msg, NAMES[entry], std::strlen(NAMES[entry])) != 0 || !std::strstr(msg, text)) {
        std::printf("FAIL %s %s: rc = %d, message = %s\n", NAMES[entry], what, rc, msg ? msg : "(none)");
        ++failures;
    }
}

}  // namespace

int main() {
    alignas(16) static unsigned char buf[256];
    static const cer_yuv420 desc = {CER_YUV_NV12, 19077, 26149, -6419, -13320, 33050, 16};
    Args good;
    good.frames = buf;
    good.affines = reinterpret_cast<const double *>(buf);
    good.bounds = good.coef = good.crop_xyf = good.row_stream = good.row_pos = reinterpret_cast<const int32_t *>(buf);
    good.out = reinterpret_cast<float *>(buf);
    good.ring = buf;
    good.yuv = &desc;
    for (int e = 0; e < 4; ++e) {
        const bool ring = e & 1, yuv = e >= 2;
        Args a = good;
        a.frames = nullptr; refused(e, a, "null", "frames"); a = good;
        a.affines = nullptr; refused(e, a, "null", "affines"); a = good;
        a.bounds = nullptr; refused(e, a, "null", "bounds"); a = good;
        a.coef = nullptr; refused(e, a, "null", "coef"); a = good;
        a.crop_xyf = nullptr; refused(e, a, "null", "crop_xyf"); a = good;
        a.affines = reinterpret_cast<const double *>(buf + 4); refused(e, a, "8-byte aligned", "misaligned affines"); a = good;
        a.n = 0; refused(e, a, ">= 1", "no frames"); a = good;
        a.n = 65536; a.rows = 65536; refused(e, a, "65535", "too many frames"); a = good;
        a.crop = 7; refused(e, a, "exceeds size", "crop > size"); a = good;
        a.align = 0; refused(e, a, "align_size", "align_size 0"); a = good;
        a.align = -4; refused(e, a, "align_size", "negative align_size"); a = good;
        a.align = (1 << 14) + 1; refused(e, a, "align_size", "align_size above 2^14"); a = good;
        a.span = 9; refused(e, a, "align_size", "band rows above align_size"); a = good;
        a.ks = 20; refused(e, a, "align_size", "more taps than align_size can need"); a = good;
        a.align = 2048; a.span = 430; a.ks = 87; a.size = 48; a.crop = 40; refused(e, a, "LDS", "align_size beyond the LDS"); a = good;
        if (!yuv) {
            a.H = 0; refused(e, a, ">= 1", "empty frames"); a = good;
            a.H = 1 << 15; a.W = 1 << 15; refused(e, a, "2^29", "huge frames"); a = good;
        } else {
            a.yuv = nullptr; refused(e, a, "null", "descriptor"); a = good;
            a.H = 7; refused(e, a, "even", "odd picture"); a = good;
            a.H = 0; refused(e, a, "even", "empty picture"); a = good;
        }
        if (ring) {
            a.ring = nullptr; refused(e, a, "null", "ring"); a = good;
            a.row_stream = nullptr; refused(e, a, "null", "row_stream"); a = good;
            a.row_pos = nullptr; refused(e, a, "null", "row_pos"); a = good;
            a.rows = 0; refused(e, a, ">= 1", "no rows"); a = good;
            a.rows = -3; refused(e, a, ">= 1", "negative rows"); a = good;
            a.Rf = 6; refused(e, a, "power of two", "ring of 6"); a = good;
            a.Rf = 0; refused(e, a, "power of two", "ring of 0"); a = good;
            a.max_count = 9; refused(e, a, "exceed Rf", "more new frames than slots"); a = good;
            a.S = 0; refused(e, a, ">= 1", "no streams"); a = good;
        } else {
            a.out = nullptr; refused(e, a, "null", "out"); a = good;
            a.group = 0; refused(e, a, ">= 1", "frames per group 0"); a = good;
            a.stdv = 0.f; refused(e, a, "std", "std 0"); a = good;
        }
    }
    if (failures) {
        std::printf("%d of %d cases failed\n", failures, cases);
        return 1;
    }
    std::printf("ok: %d refusals\n", cases);
    return 0;
}
