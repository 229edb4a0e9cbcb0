// Segmentation tail: low-resolution class logits -> labels of the bilinearly resized map and the confusion counts against a target
// map, in one launch (sc2_seg_predict).  The reference's evaluate() forms `interpolate(logits, size)`, takes `argmax(1)` and feeds
// SegEvaluator.update: three passes over a [N,C,H,W] tensor that nothing else needs.  include/sc2_bottleneck.h states the contract;
// tests/ref_seg.py restates it in float64.
// Plain kernels: every index checked against its array before use, one kind of global atomic (a 64-bit integer vector add per
// non-zero bin of a workgroup's histogram), no workgroup waits for another.
#include "seg_common.h"      // the axis map, the class loads and the resized value, shared with seg_loss.hip

namespace {

constexpr int SEG_TW = 32, SEG_TH = 8;       // output pixels of one tile: a wave covers two rows of 32
constexpr int SEG_THREADS = SEG_TW * SEG_TH;
constexpr long long SEG_MAX_TILES_PER_WG = 1ll << 22;      // x 256 pixels: a workgroup's int32 bins cannot overflow

struct SegArgs {
    const void *logits;
    const long long *targets;
    long long *labels;
    unsigned long long *mat;
    long long sN, sC, sH, sW;      // element strides of the logits
    long long n_tiles;
    int N, C, h, w, H, W, tiles_x, tiles_y;
};

// first index holding the maximum, a NaN larger than any number and the first NaN final (torch.argmax)
__device__ __forceinline__ void seg_take(float v, int c, float &best, int &label) {
    if (v > best || (v != v && best == best)) {
        best = v;
        label = c;
    }
}

// One output pixel per lane over 32 x 8 tiles of one image; a workgroup walks tiles blockIdx.x, + gridDim.x, ...  The four source
// pixels of a lane are shared with its neighbours (an 8-fold upsampling reads ~ 5 x 2 source pixels per tile): they come from
// L1 / L2.  VEC: the classes of a pixel are consecutive in memory (channel stride 1, the NHWC view) and readable in whole 16-byte
// pieces.  HIST: targets and the matrix are given; bins are counted in LDS (C * C int32) and the non-zero ones added to the global
// matrix at the end.
template <bool BF16, bool VEC, bool HIST>
__global__ __launch_bounds__(SEG_THREADS) void seg_predict_kernel(const SegArgs a) {
    extern __shared__ __attribute__((aligned(16))) int hist[];
    const int tid = threadIdx.x;
    const int bins = a.C * a.C;
    if (HIST) {
        for (int i = tid; i < bins; i += SEG_THREADS) hist[i] = 0;
        __syncthreads();
    }
    const int lx_in_tile = tid % SEG_TW, ly_in_tile = tid / SEG_TW;
    for (long long tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long per_image = (long long)a.tiles_x * a.tiles_y;
        const int n = (int)(tile / per_image);
        const int r = (int)(tile - (long long)n * per_image);
        const int ty = r / a.tiles_x, tx = r - ty * a.tiles_x;
        const int oy = ty * SEG_TH + ly_in_tile, ox = tx * SEG_TW + lx_in_tile;
        if (oy >= a.H || ox >= a.W) continue;      // (no barrier inside the tile loop)
        int y0, y1, x0, x1;
        float ly, lx;
        seg_axis(oy, a.h, a.H, y0, y1, ly);
        seg_axis(ox, a.w, a.W, x0, x1, lx);
        const float hy = 1.0f - ly, hx = 1.0f - lx;
        const long long img = (long long)n * a.sN;
        const long long p00 = img + y0 * a.sH + x0 * a.sW, p01 = img + y0 * a.sH + x1 * a.sW;
        const long long p10 = img + y1 * a.sH + x0 * a.sW, p11 = img + y1 * a.sH + x1 * a.sW;
        float best = 0.0f;
        int label = 0;
        seg_for_each_class<BF16, VEC>(a.logits, a.C, a.sC, p00, p01, p10, p11, hy, hx, ly, lx, [&](int c, float val) {
            if (c == 0)
                best = val;
            else
                seg_take(val, c, best, label);
        });
        const long long at = ((long long)n * a.H + oy) * a.W + ox;
        if (a.labels) a.labels[at] = label;
        if (HIST) {
            const long long t = a.targets[at];
            if (t >= 0 && t < a.C) atomicAdd(&hist[(int)t * a.C + label], 1);
        }
    }
    if (HIST) {
        __syncthreads();
        for (int i = tid; i < bins; i += SEG_THREADS) {
            const int v = hist[i];
            if (v) atomicAdd(&a.mat[i], (unsigned long long)v);
        }
    }
}

template <bool BF16, bool VEC>
void seg_launch(const SegArgs &a, bool hist, unsigned grid, hipStream_t s) {
    if (hist)
        hipLaunchKernelGGL((seg_predict_kernel<BF16, VEC, true>), dim3(grid), dim3(SEG_THREADS), (size_t)a.C * a.C * sizeof(int), s, a);
    else
        hipLaunchKernelGGL((seg_predict_kernel<BF16, VEC, false>), dim3(grid), dim3(SEG_THREADS), 0, s, a);
}

}  // namespace

extern "C" int sc2_seg_predict(const void *logits, int is_bf16, int N, int C, int h, int w, long long stride_n, long long stride_c,
                               long long stride_h, long long stride_w, int c_readable, int H, int W, const long long *targets,
                               long long *labels, long long *mat, void *stream) {
    SC2_REQUIRE(N > 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0, SC2_ERR_INVALID_ARG, "seg_predict: bad dims N=%d C=%d %dx%d -> %dx%d",
                N, C, h, w, H, W);
    SC2_REQUIRE(C <= SC2_SEG_MAX_CLASSES, SC2_ERR_UNSUPPORTED, "seg_predict: %d classes (at most %d)", C, SC2_SEG_MAX_CLASSES);
    SC2_REQUIRE(h <= SEG_MAX_DIM && w <= SEG_MAX_DIM && H <= SEG_MAX_DIM && W <= SEG_MAX_DIM, SC2_ERR_UNSUPPORTED,
                "seg_predict: %dx%d -> %dx%d (at most %d per side)", h, w, H, W, SEG_MAX_DIM);
    SC2_REQUIRE(logits, SC2_ERR_INVALID_ARG, "seg_predict: null logits");
    SC2_REQUIRE(stride_n >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, SC2_ERR_INVALID_ARG, "seg_predict: negative stride");
    const bool hist = targets != nullptr && mat != nullptr;
    SC2_REQUIRE(labels || hist, SC2_ERR_INVALID_ARG, "seg_predict: nothing to write (no labels, and no targets + matrix pair)");
    const size_t esize = is_bf16 ? 2 : 4;
    SC2_REQUIRE((reinterpret_cast<uintptr_t>(logits) & (esize - 1)) == 0 && (reinterpret_cast<uintptr_t>(targets) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(labels) & 7u) == 0 && (reinterpret_cast<uintptr_t>(mat) & 7u) == 0,
                SC2_ERR_INVALID_ARG, "seg_predict: misaligned pointer");
    SegArgs a;
    a.logits = logits;
    a.targets = targets;
    a.labels = labels;
    a.mat = reinterpret_cast<unsigned long long *>(mat);
    a.sN = stride_n; a.sC = stride_c; a.sH = stride_h; a.sW = stride_w;
    a.N = N; a.C = C; a.h = h; a.w = w; a.H = H; a.W = W;
    a.tiles_x = (W + SEG_TW - 1) / SEG_TW;
    a.tiles_y = (H + SEG_TH - 1) / SEG_TH;
    a.n_tiles = (long long)N * a.tiles_x * a.tiles_y;
    const bool vec = seg_vec_ok(logits, is_bf16, C, stride_n, stride_c, stride_h, stride_w, c_readable);
    const long long cap = (long long)sc2_device_cus() * 8;
    long long grid = a.n_tiles < cap ? a.n_tiles : cap;
    const long long floor_wgs = (a.n_tiles + SEG_MAX_TILES_PER_WG - 1) / SEG_MAX_TILES_PER_WG;
    if (grid < floor_wgs) grid = floor_wgs;
    SC2_REQUIRE(grid <= 0x7FFFFFFFll, SC2_ERR_UNSUPPORTED, "seg_predict: %lld tiles in one call", a.n_tiles);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (is_bf16) {
        if (vec) seg_launch<true, true>(a, hist, (unsigned)grid, s);
        else seg_launch<true, false>(a, hist, (unsigned)grid, s);
    } else {
        if (vec) seg_launch<false, true>(a, hist, (unsigned)grid, s);
        else seg_launch<false, false>(a, hist, (unsigned)grid, s);
    }
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
