// What the detection transform does around the JPEG image codec, per image (sc2bench/models/detection/transform.py:
// RCNNTransformWithCompression): bilinear resize of the float image, `mul(255).byte()`, [codec], `/ 255`, normalise, copy into the
// zero-padded batch.  Two streaming kernels close the gap on both sides of sc2_jpeg_image_codec:
//   sc2_rcnn_resize_u8     f32 image (any strides) -> u8 [C,oh,ow], the resized pixels as 8-bit already
//   sc2_rcnn_normalize_pad u8 [C,h,w] (the codec's recon) -> one f32 slot [C,Hp,Wp] of the batch tensor, every element written
// include/sc2_bottleneck.h states the contract; tests/ref_rcnn_input.py restates it.
// Plain kernels: every index checked against its array before use, no LDS, no atomics, no workgroup waits for another.
// Shared through input_common.h with det_input.hip: aten's bilinear axis (aten_axis).
#include "input_common.h"

#pragma clang fp contract(off)   // every product, sum and quotient rounded once, as the host's operator-by-operator arithmetic

namespace {

constexpr int RI_LANES = 64, RI_WAVES = 4;       // a workgroup: 64 lanes across the columns, 4 waves down the rows
constexpr int RI_PX = 4;                         // adjacent output pixels of a row per lane
constexpr int RI_TW = RI_LANES * RI_PX;          // 256 output columns per column tile
constexpr int RI_ROWS = 4;                       // rows per lane of the resize kernel: its x indices and weights are reused over them
constexpr int RI_TH = RI_WAVES * RI_ROWS;        // 16 output rows per row tile
constexpr int RI_MAX_PAD_SIDE = 4 * SC2_JPEG_IMAGE_MAX_SIDE;

struct ResizeArgs {
    const float *x;
    uint8_t *out;
    int *status;
    long long sc, sh, sw;
    int C, H, W, oh, ow;
};

__device__ __forceinline__ bool ri_in_unit(float v) { return v >= 0.0f && v <= 1.0f; }      // false for NaN

__global__ __launch_bounds__(RI_LANES * RI_WAVES) void rcnn_resize_u8_kernel(const ResizeArgs a) {
    const int c = blockIdx.z;
    const int x0 = blockIdx.x * RI_TW + threadIdx.x * RI_PX;
    if (x0 >= a.ow) return;
    const float scale_x = __fdiv_rn((float)a.W, (float)a.ow), scale_y = __fdiv_rn((float)a.H, (float)a.oh);
    long long xa[RI_PX], xb[RI_PX];      // element offsets of the two source columns
    float lx[RI_PX];
#pragma unroll
    for (int j = 0; j < RI_PX; ++j) {
        int i0, i1;
        aten_axis(min(x0 + j, a.ow - 1), scale_x, a.W, i0, i1, lx[j]);      // (a column beyond the row repeats the last one: not stored)
        xa[j] = i0 * a.sw;
        xb[j] = i1 * a.sw;
    }
    const float *plane = a.x + c * a.sc;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < RI_ROWS; ++r) {
        const int y = blockIdx.y * RI_TH + r * RI_WAVES + threadIdx.y;
        if (y >= a.oh) break;
        int j0, j1;
        float ly1;
        aten_axis(y, scale_y, a.H, j0, j1, ly1);
        const float ly0 = 1.0f - ly1;
        const float *row0 = plane + j0 * a.sh, *row1 = plane + j1 * a.sh;
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < RI_PX; ++j) {
            const float p = row0[xa[j]], q = row0[xb[j]], s = row1[xa[j]], t = row1[xb[j]];
            bad |= !(ri_in_unit(p) && ri_in_unit(q) && ri_in_unit(s) && ri_in_unit(t));
            const float lx1 = lx[j], lx0 = 1.0f - lx1;
            const float v = ly0 * (lx0 * p + lx1 * q) + ly1 * (lx0 * s + lx1 * t);
            // values in [0, 1] give 0..255; anything else is reported through `status` and its byte is unspecified
            const int b = (int)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f);
            packed |= (uint32_t)(b & 0xFF) << (8 * j);
        }
        uint8_t *dst = a.out + ((size_t)c * a.oh + y) * a.ow + x0;
        const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 3u);      // the same for every lane of the row
        if (x0 + RI_PX <= a.ow && mis == 0) {
            *reinterpret_cast<uint32_t *>(dst) = packed;
        } else if (x0 + RI_PX <= a.ow && mis == 2) {
            reinterpret_cast<uint16_t *>(dst)[0] = (uint16_t)(packed & 0xFFFFu);
            reinterpret_cast<uint16_t *>(dst)[1] = (uint16_t)(packed >> 16);
        } else {
#pragma unroll
            for (int j = 0; j < RI_PX; ++j)
                if (x0 + j < a.ow) dst[j] = (uint8_t)(packed >> (8 * j));
        }
    }
    if (bad) *a.status = 1;      // a vector store of the lanes that met such a value; the word was cleared before the launch
}

struct NormArgs {
    const uint8_t *px;
    float *out;
    float mean[3], std[3];
    int C, h, w, Hp, Wp;
};

__global__ __launch_bounds__(RI_LANES * RI_WAVES) void rcnn_normalize_pad_kernel(const NormArgs a) {
    const int c = blockIdx.z;
    const int y = blockIdx.y * RI_WAVES + threadIdx.y;
    const int x0 = blockIdx.x * RI_TW + threadIdx.x * RI_PX;
    if (y >= a.Hp || x0 >= a.Wp) return;
    const float mean = a.mean[c], sd = a.std[c];
    float v[RI_PX] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (y < a.h && x0 < a.w) {
        const uint8_t *src = a.px + ((size_t)c * a.h + y) * a.w + x0;
        uint32_t p4 = 0;
        if (x0 + RI_PX <= a.w && (reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
            p4 = *reinterpret_cast<const uint32_t *>(src);
        } else {
#pragma unroll
            for (int j = 0; j < RI_PX; ++j)
                if (x0 + j < a.w) p4 |= (uint32_t)src[j] << (8 * j);
        }
#pragma unroll
        for (int j = 0; j < RI_PX; ++j)
            if (x0 + j < a.w) v[j] = __fdiv_rn(__fdiv_rn((float)((p4 >> (8 * j)) & 0xFFu), 255.0f) - mean, sd);
    }
    float *dst = a.out + ((size_t)c * a.Hp + y) * a.Wp + x0;
    if (x0 + RI_PX <= a.Wp && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < RI_PX; ++j)
            if (x0 + j < a.Wp) dst[j] = v[j];
    }
}

}  // namespace

extern "C" int sc2_rcnn_resize_u8(const float *x, long long sc, long long sh, long long sw, int C, int H, int W, uint8_t *out, int oh,
                                  int ow, int32_t *status, void *stream) {
    SC2_REQUIRE(C == 1 || C == 3, SC2_ERR_UNSUPPORTED, "rcnn_resize_u8: %d channels (1 or 3)", C);
    SC2_REQUIRE(H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && H <= SC2_JPEG_IMAGE_MAX_SIDE && W <= SC2_JPEG_IMAGE_MAX_SIDE &&
                    oh <= SC2_JPEG_IMAGE_MAX_SIDE && ow <= SC2_JPEG_IMAGE_MAX_SIDE,
                SC2_ERR_UNSUPPORTED, "rcnn_resize_u8: %dx%d -> %dx%d (sides 1..%d)", H, W, oh, ow, SC2_JPEG_IMAGE_MAX_SIDE);
    SC2_REQUIRE(x && out && status, SC2_ERR_INVALID_ARG, "rcnn_resize_u8: null pointer");
    SC2_REQUIRE(sc >= 0 && sh >= 0 && sw >= 0, SC2_ERR_INVALID_ARG, "rcnn_resize_u8: negative stride");
    SC2_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(status)) & 3u) == 0, SC2_ERR_INVALID_ARG,
                "rcnn_resize_u8: misaligned pointer");
    ResizeArgs a;
    a.x = x; a.out = out; a.status = status;
    a.sc = sc; a.sh = sh; a.sw = sw;
    a.C = C; a.H = H; a.W = W; a.oh = oh; a.ow = ow;
    const dim3 grid((unsigned)((ow + RI_TW - 1) / RI_TW), (unsigned)((oh + RI_TH - 1) / RI_TH), (unsigned)C);
    hipLaunchKernelGGL(rcnn_resize_u8_kernel, grid, dim3(RI_LANES, RI_WAVES), 0, static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_rcnn_normalize_pad(const uint8_t *pixels, int C, int h, int w, const float *mean, const float *std, float *out,
                                      int Hp, int Wp, void *stream) {
    SC2_REQUIRE(C == 1 || C == 3, SC2_ERR_UNSUPPORTED, "rcnn_normalize_pad: %d channels (1 or 3)", C);
    SC2_REQUIRE(h >= 1 && w >= 1 && h <= SC2_JPEG_IMAGE_MAX_SIDE && w <= SC2_JPEG_IMAGE_MAX_SIDE, SC2_ERR_UNSUPPORTED,
                "rcnn_normalize_pad: %dx%d image (sides 1..%d)", h, w, SC2_JPEG_IMAGE_MAX_SIDE);
    SC2_REQUIRE(Hp <= RI_MAX_PAD_SIDE && Wp <= RI_MAX_PAD_SIDE, SC2_ERR_UNSUPPORTED, "rcnn_normalize_pad: %dx%d slot (at most %d per side)",
                Hp, Wp, RI_MAX_PAD_SIDE);
    SC2_REQUIRE(Hp >= h && Wp >= w, SC2_ERR_INVALID_ARG, "rcnn_normalize_pad: a %dx%d slot for a %dx%d image", Hp, Wp, h, w);
    SC2_REQUIRE(pixels && mean && std && out, SC2_ERR_INVALID_ARG, "rcnn_normalize_pad: null pointer");
    SC2_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, SC2_ERR_INVALID_ARG, "rcnn_normalize_pad: misaligned pointer");
    NormArgs a;
    a.px = pixels; a.out = out;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = c < C ? mean[c] : 0.0f;
        a.std[c] = c < C ? std[c] : 1.0f;
    }
    a.C = C; a.h = h; a.w = w; a.Hp = Hp; a.Wp = Wp;
    const dim3 grid((unsigned)((Wp + RI_TW - 1) / RI_TW), (unsigned)((Hp + RI_WAVES - 1) / RI_WAVES), (unsigned)C);
    hipLaunchKernelGGL(rcnn_normalize_pad_kernel, grid, dim3(RI_LANES, RI_WAVES), 0, static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
