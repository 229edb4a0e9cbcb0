// What the device input kernels share (seg_augment.hip, cls_input.hip, det_input.hip, rcnn_input.hip):
//   Pillow's 8-bit bilinear resample (seg_augment, cls_input): the per-axis bounds and 22-bit fixed-point coefficients of ImagingResample,
//       the load of one RGB pixel (det_input too), the two passes of one output pixel through the LDS band, and the tile both kernels
//       cut the output into.  tests/ref_pil_resize.py restates the arithmetic.
//   aten's bilinear axis (det_input, rcnn_input).
//   The argument checks and the mean / std block of the entries that take a source buffer (seg_augment, cls_input, det_input).
#pragma once
#include "sc2_common.h"
#include <stddef.h>

#pragma clang fp contract(off)   // int() truncates and the sums are ordered: a fused multiply-add in `center` moves xmin for some sizes

constexpr int PIL_TAPS = 9;      // ksize at filterscale 4
constexpr int PIL_BITS = 22;     // Pillow's PRECISION_BITS for 8-bit channels
constexpr int PIL_TH = 16, PIL_TW = 64;                  // output rows and columns of a tile
constexpr int PIL_THREADS = 256;                         // a wave owns a row of the tile, its lanes the columns
constexpr int PIL_ROWS = 4 * PIL_TH + PIL_TAPS;          // source rows a band can need: (TH - 1) * 4 + 2 * 4 + 1 and some

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
// the byte behind the pixel is still the image's (every pixel but the last), three byte loads otherwise.  Off: size_t in the Pillow
// kernels; int in det_input_kernel, whose offsets lie below 2^31 and which holds the byte count in one scalar register that way (the
// 64-bit comparison costs it a register pair: 34 SGPRs against 32).
template <typename Off>
__device__ __forceinline__ uint32_t pil_pixel(const uint8_t *img, Off off, Off bytes) {
    if (off + 4 <= bytes) {
        uint32_t v;
        __builtin_memcpy(&v, img + off, 4);
        return v;
    }
    return (uint32_t)img[off] | (uint32_t)img[off + 1] << 8 | (uint32_t)img[off + 2] << 16;
}

__device__ __forceinline__ int pil_clip8(int acc) { return min(max(acc >> PIL_BITS, 0), 255); }

// The horizontal pass of one output column on source row sr of an h x w image of img_bytes bytes: `count` taps from column `first`
// (both clamped to the row) with the coefficients k, as R | G << 8 | B << 16.
__device__ __forceinline__ uint32_t pil_hpass(const uint8_t *img, size_t img_bytes, int w, int sr, int first, int count,
                                              const int (&k)[PIL_TAPS]) {
    int acc0 = 1 << (PIL_BITS - 1), acc1 = acc0, acc2 = acc0;
#pragma unroll
    for (int t = 0; t < PIL_TAPS; ++t) {
        if (t < count) {
            const uint32_t p = pil_pixel(img, ((size_t)sr * w + min(max(first + t, 0), w - 1)) * 3, img_bytes);
            acc0 += (int)(p & 0xFFu) * k[t];
            acc1 += (int)((p >> 8) & 0xFFu) * k[t];
            acc2 += (int)((p >> 16) & 0xFFu) * k[t];
        }
    }
    return (uint32_t)pil_clip8(acc0) | (uint32_t)pil_clip8(acc1) << 8 | (uint32_t)pil_clip8(acc2) << 16;
}

// The vertical pass of one output pixel out of the band hbuf [ROWS][TW] of pil_hpass words, column lx: the taps of the row entry e
// (e[1] of them, coefficients from e[2]) from band row `first` (clamped to the band), then `(p / 255 - mean) / std` per channel.
template <int ROWS, int TW>
__device__ __forceinline__ void pil_vpass(const uint32_t *hbuf, int lx, const int32_t *e, int first, const float (&mean)[3],
                                          const float (&std)[3], float &v0, float &v1, float &v2) {
    const int count = e[1];
    int acc0 = 1 << (PIL_BITS - 1), acc1 = acc0, acc2 = acc0;
#pragma unroll
    for (int t = 0; t < PIL_TAPS; ++t) {
        if (t < count) {
            const int kt = e[2 + t];
            const uint32_t p = hbuf[min(max(first + t, 0), ROWS - 1) * TW + lx];
            acc0 += (int)(p & 0xFFu) * kt;
            acc1 += (int)((p >> 8) & 0xFFu) * kt;
            acc2 += (int)((p >> 16) & 0xFFu) * kt;
        }
    }
    v0 = __fdiv_rn(__fdiv_rn((float)pil_clip8(acc0), 255.0f) - mean[0], std[0]);
    v1 = __fdiv_rn(__fdiv_rn((float)pil_clip8(acc1), 255.0f) - mean[1], std[1]);
    v2 = __fdiv_rn(__fdiv_rn((float)pil_clip8(acc2), 255.0f) - mean[2], std[2]);
}

// aten's upsample_bilinear2d index and weight of output index d (align_corners=False, no given scale factor), in f32
__device__ __forceinline__ void aten_axis(int d, float scale, int in, int &i0, int &i1, float &l1) {
    const float src = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.0f);
    i0 = min((int)src, in - 1);
    i1 = min(i0 + 1, in - 1);
    l1 = src - (float)i0;
}

// (The guarded 4-wide store of a padded float row stays with its two kernels: det_input_kernel decides once for the three planes of a
// pixel, from the row's address and the plane's pitch, rcnn_normalize_pad_kernel per address.  One routine would take that verdict as
// a flag, or decide per plane, which costs det_input_kernel four scalar registers.)

// mean / std as the kernels' argument structs carry them, and what the entries with a source buffer check in front of their launches,
// in the entries' order: the buffer's size, the pointers (`set` / `aligned`: the entry's own verdict on all of its pointers, mean and
// std among them), a non-zero std.  -> SC2_OK with mean / std copied in, else the error code with the message set.
struct InputNorm {
    float mean[3], std[3];

    int take(const char *who, long long nbytes, bool set, bool aligned, const float *mean_in, const float *std_in) {
        SC2_REQUIRE(nbytes >= 1 && nbytes <= 0x7FFFFFFFLL, SC2_ERR_UNSUPPORTED, "%s: a source buffer of %lld bytes (1..2^31-1)", who, nbytes);
        SC2_REQUIRE(set, SC2_ERR_INVALID_ARG, "%s: null pointer", who);
        SC2_REQUIRE(aligned, SC2_ERR_INVALID_ARG, "%s: misaligned pointer", who);
        for (int c = 0; c < 3; ++c) {
            SC2_REQUIRE(std_in[c] != 0.0f, SC2_ERR_INVALID_ARG, "%s: std[%d] is zero", who, c);
            mean[c] = mean_in[c];
            std[c] = std_in[c];
        }
        return SC2_OK;
    }
};
