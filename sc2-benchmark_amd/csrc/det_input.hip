// The detector's input transform of a whole batch, from the packed source bytes to the finished padded batch tensor
// (torchvision's GeneralizedRCNNTransform behind ToTensor and the optional horizontal flip of the COCO loader: normalise, bilinear
// resize, copy into the zero-padded batch):
//   sc2_det_input   u8 [h,w,3] sources of n samples in one buffer -> f32 [n,3,Hp,Wp], every element written exactly once
// One launch per call.  A workgroup owns a 16 x 256 output tile of one sample and produces all three channels of it: the source is
// interleaved, so one set of indices and weights serves three planes.  The 3 x 256 table of normalised byte values is built once per
// workgroup in LDS.  include/sc2_bottleneck.h states the contract; tests/ref_det_input.py restates the arithmetic.
// Plain kernel: every index checked against its array before use, no atomics, no workgroup waits for another.
// Shared through input_common.h with rcnn_input.hip: aten's bilinear axis (aten_axis); with seg_augment.hip and cls_input.hip: the
// pixel load (pil_pixel, here over int offsets) and the entry's checks (InputNorm).
#include "input_common.h"

#pragma clang fp contract(off)   // every product, sum and quotient rounded once, as the host's operator-by-operator arithmetic

namespace {

constexpr int DI_LANES = 64, DI_WAVES = 4;       // a workgroup: 64 lanes across the columns, 4 waves down the rows
constexpr int DI_PX = 4;                         // adjacent output pixels of a row per lane
constexpr int DI_TW = SC2_DET_INPUT_TILE_W;      // 256 output columns per tile
constexpr int DI_ROWS = 4;                       // rows per lane: its column indices and weights are reused over them
constexpr int DI_TH = SC2_DET_INPUT_TILE_H;      // 16 output rows per tile
constexpr int DI_MAX_SIDE = SC2_JPEG_IMAGE_MAX_SIDE;
constexpr int DI_MAX_PAD_SIDE = 4 * SC2_JPEG_IMAGE_MAX_SIDE;
static_assert(DI_TW == DI_LANES * DI_PX && DI_TH == DI_WAVES * DI_ROWS, "tile sizes of the header");
static_assert(DI_LANES * DI_WAVES == 256, "one thread per table entry of a channel");

struct DetRow {
    int off, h, w, oh, ow, flip;
};
static_assert(sizeof(DetRow) == SC2_DET_INPUT_ROW_INTS * sizeof(int32_t), "a descriptor row of the header");

struct DetArgs {
    const uint8_t *buf;
    float *out;
    long long nbytes;
    InputNorm norm;
    int n, Hp, Wp;
    DetRow row[SC2_DET_INPUT_MAX_BATCH];
};

// 0: the row may be launched; else the error code of the entry
__host__ __device__ inline int di_row_status(const DetRow &s, long long nbytes, int Hp, int Wp) {
    if (s.h < 1 || s.w < 1 || s.oh < 1 || s.ow < 1 || s.h > DI_MAX_SIDE || s.w > DI_MAX_SIDE || s.oh > DI_MAX_SIDE || s.ow > DI_MAX_SIDE)
        return SC2_ERR_UNSUPPORTED;
    if (s.off < 0 || (long long)s.off + 3LL * s.h * s.w > nbytes || s.oh > Hp || s.ow > Wp || (s.flip != 0 && s.flip != 1))
        return SC2_ERR_INVALID_ARG;
    return 0;
}

__global__ __launch_bounds__(DI_LANES * DI_WAVES) void det_input_kernel(const DetArgs a) {
    __shared__ float nrm[3 * 256];      // [channel][byte]: ((b / 255) - mean) / std
    const int tid = threadIdx.y * DI_LANES + threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) nrm[c * 256 + tid] = __fdiv_rn(__fdiv_rn((float)tid, 255.0f) - a.norm.mean[c], a.norm.std[c]);
    __syncthreads();
    const int i = blockIdx.z;
    const int x0 = blockIdx.x * DI_TW + threadIdx.x * DI_PX;
    if (i >= a.n || x0 >= a.Wp) return;
    const DetRow s = a.row[i];
    // (the entry refuses such a row before the launch; here it shows as padding and moves no address)
    const bool ok = di_row_status(s, a.nbytes, a.Hp, a.Wp) == 0;
    const int oh = ok ? s.oh : 0, ow = ok ? s.ow : 0;
    const int h = ok ? s.h : 1, w = ok ? s.w : 1;
    const uint8_t *img = a.buf + (ok ? s.off : 0);
    const int img_bytes = ok ? 3 * h * w : 0;
    const bool live = x0 < ow;       // some column of this lane shows resized pixels
    int xa[DI_PX], xb[DI_PX];        // byte offsets of the two source columns in a row
    float lx[DI_PX];
    if (live) {
        const float scale_x = __fdiv_rn((float)w, (float)ow);
#pragma unroll
        for (int j = 0; j < DI_PX; ++j) {
            int i0, i1;
            aten_axis(min(x0 + j, ow - 1), scale_x, w, i0, i1, lx[j]);      // (a column beyond the image repeats the last one: not stored)
            xa[j] = 3 * (s.flip ? w - 1 - i0 : i0);
            xb[j] = 3 * (s.flip ? w - 1 - i1 : i1);
        }
    } else {
#pragma unroll
        for (int j = 0; j < DI_PX; ++j) {
            xa[j] = xb[j] = 0;
            lx[j] = 0.0f;
        }
    }
    const float scale_y = live ? __fdiv_rn((float)h, (float)oh) : 1.0f;
    const size_t plane = (size_t)a.Hp * a.Wp;
    float *slot = a.out + (size_t)i * 3 * plane;
#pragma unroll
    for (int r = 0; r < DI_ROWS; ++r) {
        const int y = blockIdx.y * DI_TH + r * DI_WAVES + threadIdx.y;
        if (y >= a.Hp) break;
        float v[3][DI_PX];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < DI_PX; ++j) v[c][j] = 0.0f;
        if (live && y < oh) {
            int j0, j1;
            float ly1;
            aten_axis(y, scale_y, h, j0, j1, ly1);
            const float ly0 = 1.0f - ly1;
            const int r0 = j0 * w * 3, r1 = j1 * w * 3;
#pragma unroll
            for (int j = 0; j < DI_PX; ++j) {
                if (x0 + j < ow) {
                    const uint32_t p = pil_pixel(img, r0 + xa[j], img_bytes), q = pil_pixel(img, r0 + xb[j], img_bytes),
                                   u = pil_pixel(img, r1 + xa[j], img_bytes), t = pil_pixel(img, r1 + xb[j], img_bytes);
                    const float lx1 = lx[j], lx0 = 1.0f - lx1;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float *tab = nrm + c * 256;
                        const float fp = tab[(p >> (8 * c)) & 0xFFu], fq = tab[(q >> (8 * c)) & 0xFFu], fu = tab[(u >> (8 * c)) & 0xFFu],
                                    ft = tab[(t >> (8 * c)) & 0xFFu];
                        v[c][j] = ly0 * (lx0 * fp + lx1 * fq) + ly1 * (lx0 * fu + lx1 * ft);
                    }
                }
            }
        }
        float *dst = slot + (size_t)y * a.Wp + x0;
        const bool wide = x0 + DI_PX <= a.Wp && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0 && ((plane * sizeof(float)) & 15u) == 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float *d = dst + c * plane;
            if (wide) {
                *reinterpret_cast<float4 *>(d) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            } else {
#pragma unroll
                for (int j = 0; j < DI_PX; ++j)
                    if (x0 + j < a.Wp) d[j] = v[c][j];
            }
        }
    }
}

}  // namespace

extern "C" int sc2_det_input(const uint8_t *buf, long long nbytes, const int32_t *rows, int n, const float *mean, const float *std,
                             float *out, int Hp, int Wp, void *stream) {
    SC2_REQUIRE(n >= 1 && n <= SC2_DET_INPUT_MAX_BATCH, SC2_ERR_UNSUPPORTED, "det_input: %d samples (1..%d per launch)", n,
                SC2_DET_INPUT_MAX_BATCH);
    SC2_REQUIRE(Hp >= 1 && Wp >= 1 && Hp <= DI_MAX_PAD_SIDE && Wp <= DI_MAX_PAD_SIDE, SC2_ERR_UNSUPPORTED,
                "det_input: a %dx%d batch (sides 1..%d)", Hp, Wp, DI_MAX_PAD_SIDE);
    DetArgs a;
    const int rc = a.norm.take("det_input", nbytes, buf && rows && mean && std && out, (reinterpret_cast<uintptr_t>(out) & 3u) == 0, mean,
                               std);
    if (rc != SC2_OK) return rc;
    for (int i = 0; i < SC2_DET_INPUT_MAX_BATCH; ++i) {
        DetRow &s = a.row[i];
        if (i < n) {
            const int32_t *d = rows + (size_t)i * SC2_DET_INPUT_ROW_INTS;
            s.off = d[0]; s.h = d[1]; s.w = d[2]; s.oh = d[3]; s.ow = d[4]; s.flip = d[5];
            const int st = di_row_status(s, nbytes, Hp, Wp);      // every row is checked before anything is launched
            SC2_REQUIRE(st == 0, st, "det_input: sample %d: offset %d, %dx%d -> %dx%d, flip %d in %lld bytes and a %dx%d batch (sides 1..%d)",
                        i, s.off, s.h, s.w, s.oh, s.ow, s.flip, nbytes, Hp, Wp, DI_MAX_SIDE);
        } else {
            s.off = 0; s.h = 0; s.w = 0; s.oh = 0; s.ow = 0; s.flip = 0;
        }
    }
    a.buf = buf; a.out = out; a.nbytes = nbytes;
    a.n = n; a.Hp = Hp; a.Wp = Wp;
    const dim3 grid((unsigned)((Wp + DI_TW - 1) / DI_TW), (unsigned)((Hp + DI_TH - 1) / DI_TH), (unsigned)n);
    hipLaunchKernelGGL(det_input_kernel, grid, dim3(DI_LANES, DI_WAVES), 0, static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
