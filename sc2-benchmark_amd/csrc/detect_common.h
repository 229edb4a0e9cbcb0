// What the detection kernels share (detect.hip, det_post.hip): the f32 IoU that include/sc2_bottleneck.h states for sc2_nms, the
// alignment tests of their entry points and the check of a caller's host copy of per-image offsets.
// Every includer turns contraction off (`#pragma clang fp contract(off)`) before it includes this: `area_a + area_b - w * h` is
// rounded step by step, as the restatement does.
#pragma once
#include "sc2_common.h"

namespace {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// IoU in f32, each operation rounded once (contraction is off in the includer; `/` is the correctly rounded IEEE division)
__device__ __forceinline__ float box_iou(const float4 a, const float area_a, const float4 b, const float area_b) {
    const float w = fmaxf(0.0f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
    const float h = fmaxf(0.0f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}
__device__ __forceinline__ float box_area(const float4 b) { return (b.z - b.x) * (b.w - b.y); }

// the bounds of image `img` in an array of `total` rows, from the device's offsets: clamped, so that whatever they hold stays inside
__device__ __forceinline__ void match_range(const int32_t *off, int img, int total, int &b, int &e) {
    b = min(max(off[img], 0), total);
    e = min(max(off[img + 1], b), total);
}

// offsets as the caller's host copy states them: start at 0, never decrease, end at the total
inline bool match_offsets_ok(const int32_t *off, int n_img, int total, int &longest) {
    if (off[0] != 0) return false;
    longest = 0;
    for (int i = 0; i < n_img; ++i) {
        if (off[i + 1] < off[i] || off[i + 1] > total) return false;
        longest = off[i + 1] - off[i] > longest ? off[i + 1] - off[i] : longest;
    }
    return off[n_img] == total;
}

}  // namespace
