// feature_norm_args_check.cpp -- a stand-alone host program that drives the argument checks of cer_feature_moments_update and
// cer_standardize_rows (csrc/feature_norm.hip) with bad pointers, sizes and alignments.  Every call below must be refused
// before any GPU call, with the entry's own name at the head of cer_last_error(); the pointers handed over are never
// dereferenced.  The M * C < 2^31 rule is driven at 2^62-scale row counts: it must refuse them and not wrap.  Meant to be
// compiled together with the translation unit and cer_common.hip under the host sanitizers and run on a machine without a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/feature_norm_args_check.cpp <pkg>/csrc/feature_norm.hip <pkg>/csrc/cer_common.hip -o feature_norm_args_check
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
    const float *x;
    int64_t M = 4;
    int C = 8;
    double *acc;
    const float *mean, *std;
    float *out;
};

const char *const NAMES[2] = {"feature_moments_update:", "standardize_rows:"};

int call(int entry, const Args &a) {
    return entry == 0 ? cer_feature_moments_update(a.x, a.M, a.C, a.acc, nullptr)
                      : cer_standardize_rows(a.x, a.M, a.C, a.mean, a.std, a.out, nullptr);
}

void refused(int entry, const Args &a, const char *text, const char *what) {
    ++cases;
    const int rc = call(entry, a);
    const char *msg = cer_last_error();
    if (rc != CER_ERR_INVALID_ARG || !msg || std::strncmp(msg, NAMES[entry], std::strlen(NAMES[entry])) != 0 || !std::strstr(msg, text)) {
        std::printf("FAIL %s %s: rc = %d, message = %s\n", NAMES[entry], what, rc, msg ? msg : "(none)");
        ++failures;
    }
}

}  // namespace

int main() {
    alignas(16) static unsigned char buf[256];
    const int64_t big = (int64_t)1 << 62;
    Args good;
    good.x = reinterpret_cast<const float *>(buf);
    good.acc = reinterpret_cast<double *>(buf);
    good.mean = good.std = reinterpret_cast<const float *>(buf);
    good.out = reinterpret_cast<float *>(buf);
    for (int e = 0; e < 2; ++e) {
        Args a = good;
        a.x = nullptr; refused(e, a, "null", "null rows"); a = good;
        a.M = 0; refused(e, a, ">= 1", "no rows"); a = good;
        a.M = -1; refused(e, a, ">= 1", "M = -1"); a = good;
        a.M = INT64_MIN; refused(e, a, ">= 1", "M = INT64_MIN"); a = good;
        a.C = 0; refused(e, a, "columns", "C = 0"); a = good;
        a.C = -4; refused(e, a, "columns", "C = -4"); a = good;
        a.C = INT32_MIN; refused(e, a, "columns", "C = INT32_MIN"); a = good;
        a.C = (1 << 20) + 4; refused(e, a, "columns", "C above 2^20"); a = good;
        a.C = INT32_MAX - 3; refused(e, a, "columns", "C = INT32_MAX - 3"); a = good;
        // M * C: the largest product that passes is 2^31 - 1; these must be refused without the product being formed
        a.M = (int64_t)1 << 28; a.C = 8; refused(e, a, "2^31", "M * C = 2^31"); a = good;
        a.M = ((int64_t)1 << 31) / 768 + 1; a.C = 768; refused(e, a, "2^31", "M * 768 just above 2^31"); a = good;
        a.M = (int64_t)1 << 31; a.C = 4; refused(e, a, "2^31", "M = 2^31"); a = good;
        a.M = big; a.C = 4; refused(e, a, "2^31", "M = 2^62: M * 4 wraps to 0"); a = good;
        a.M = big; a.C = 1 << 20; refused(e, a, "2^31", "M = 2^62, C = 2^20"); a = good;
        a.M = INT64_MAX; a.C = 1 << 20; refused(e, a, "2^31", "M = INT64_MAX"); a = good;
        a.x = reinterpret_cast<const float *>(buf + 2); refused(e, a, "aligned", "rows at an odd address"); a = good;
    }
    Args a = good;
    a.acc = nullptr; refused(0, a, "null", "null acc"); a = good;
    a.acc = reinterpret_cast<double *>(buf + 4); refused(0, a, "aligned", "acc at 4 mod 8"); a = good;
    a.mean = nullptr; refused(1, a, "null", "null mean"); a = good;
    a.std = nullptr; refused(1, a, "null", "null std"); a = good;
    a.out = nullptr; refused(1, a, "null", "null out"); a = good;
    a.C = 6; refused(1, a, "multiple of 4", "C = 6"); a = good;
    a.C = 3; refused(1, a, "multiple of 4", "C = 3"); a = good;
    a.C = 1; refused(1, a, "multiple of 4", "C = 1"); a = good;
    a.x = reinterpret_cast<const float *>(buf + 4); refused(1, a, "aligned", "x at 4 mod 16"); a = good;
    a.mean = reinterpret_cast<const float *>(buf + 8); refused(1, a, "aligned", "mean at 8 mod 16"); a = good;
    a.std = reinterpret_cast<const float *>(buf + 4); refused(1, a, "aligned", "std at 4 mod 16"); a = good;
    a.out = reinterpret_cast<float *>(buf + 12); refused(1, a, "aligned", "out at 12 mod 16"); a = good;
    if (failures) {
        std::printf("%d of %d cases failed\n", failures, cases);
        return 1;
    }
    std::printf("ok: %d refusals\n", cases);
    return 0;
}
