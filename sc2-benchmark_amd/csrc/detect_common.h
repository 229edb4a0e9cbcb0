// What the detection kernels share (detect.hip, det_post.hip, rpn_post.hip): the f32 IoU that include/sc2_bottleneck.h states for
// sc2_nms, BoxCoder's decode with the clip to the image, the alignment tests of their entry points and the check of a caller's host
// copy of per-image offsets.
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

// torch.clamp's semantics (a NaN stays a NaN: both comparisons are false)
__device__ __forceinline__ float clamp_max(float v, float hi) { return v > hi ? hi : v; }
__device__ __forceinline__ float clamp_box(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

// BoxCoder.decode_single of one (box p, deltas dl) in that function's order, then clip_boxes_to_image: every operation rounded
// once (contraction is off in the includer), the weights w = (wx, wy, ww, wh), dw and dh cut at `clip`
__device__ __forceinline__ float4 decode_clip_box(const float4 p, const float4 dl, const float4 w, float clip, float img_w, float img_h) {
    const float widths = p.z - p.x, heights = p.w - p.y;
    const float ctr_x = p.x + 0.5f * widths, ctr_y = p.y + 0.5f * heights;
    const float dx = dl.x / w.x, dy = dl.y / w.y;
    const float dw = clamp_max(dl.z / w.z, clip), dh = clamp_max(dl.w / w.w, clip);
    const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y;
    const float half_w = 0.5f * (expf(dw) * widths), half_h = 0.5f * (expf(dh) * heights);
    float4 b;
    b.x = clamp_box(pcx - half_w, img_w);
    b.y = clamp_box(pcy - half_h, img_h);
    b.z = clamp_box(pcx + half_w, img_w);
    b.w = clamp_box(pcy + half_h, img_h);
    return b;
}

// a float's bits mapped so that unsigned order is the floats' order (-0 below +0, NaNs by their bits: callers that care map them first)
__device__ __forceinline__ unsigned float_order_bits(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

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
