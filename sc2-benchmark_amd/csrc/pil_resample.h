// Pillow's 8-bit bilinear resample as the input kernels share it (seg_augment.hip, cls_input.hip): the per-axis bounds and 22-bit
// fixed-point coefficients of ImagingResample, and the load of one RGB pixel.  tests/ref_pil_resize.py restates the arithmetic.
#pragma once
#include <stdint.h>
#include <stddef.h>

#pragma clang fp contract(off)   // int() truncates and the sums are ordered: a fused multiply-add in `center` moves xmin for some sizes

constexpr int PIL_TAPS = 9;      // ksize at filterscale 4
constexpr int PIL_BITS = 22;     // Pillow's PRECISION_BITS for 8-bit channels

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output index xx of an axis n_in -> n_out with the bilinear filter:
// e[0] = first source index, e[1] = count, e[2 .. 2 + PIL_TAPS) = the coefficients (0 behind count).
__device__ __forceinline__ void pil_coeffs(int n_in, int n_out, int xx, int32_t *e) {
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs, ss = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    xmax -= xmin;
    if (xmax > PIL_TAPS) xmax = PIL_TAPS;      // (cannot happen at filterscale <= 4: 2 * support + 1 <= 9)
    if (xmax < 0) xmax = 0;
    double wt[PIL_TAPS];
    double ww = 0.0;
#pragma unroll
    for (int x = 0; x < PIL_TAPS; ++x) {
        const double v = fabs(((double)(x + xmin) - center + 0.5) * ss);
        wt[x] = (x < xmax && v < 1.0) ? 1.0 - v : 0.0;
        if (x < xmax) ww += wt[x];
    }
    e[0] = xmin;
    e[1] = xmax;
#pragma unroll
    for (int x = 0; x < PIL_TAPS; ++x) {
        const double p = ww != 0.0 ? wt[x] / ww : wt[x];
        e[2 + x] = x < xmax ? (int)(0.5 + p * (double)(1 << PIL_BITS)) : 0;
    }
}

// The three bytes of the pixel at byte offset `off` of an image of `bytes` bytes, R in the low byte: one unaligned four-byte load where
// the byte behind the pixel is still the image's (every pixel but the last), three byte loads otherwise.
__device__ __forceinline__ uint32_t pil_pixel(const uint8_t *img, size_t off, size_t bytes) {
    if (off + 4 <= bytes) {
        uint32_t v;
        __builtin_memcpy(&v, img + off, 4);
        return v;
    }
    return (uint32_t)img[off] | (uint32_t)img[off + 1] << 8 | (uint32_t)img[off + 2] << 16;
}
