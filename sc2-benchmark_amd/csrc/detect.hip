// Detection tail (Faster R-CNN behind the feature pyramid): the two operations of torchvision's inference path that have no
// torch-op equivalent -- greedy non-maximum suppression with groups (`batched_nms`, run per pyramid level on the RPN's proposals
// and per class on the detections) and multi-level RoIAlign (`MultiScaleRoIAlign`, aligned=False).  include/sc2_bottleneck.h
// states the contract; tests/ref_detection.py restates it sequentially.
// Plain kernels: no atomics on global memory, no workgroup waits for another, every index checked against its array before use.
#include "sc2_common.h"

#pragma clang fp contract(off)   // `area_a + area_b - w * h`, `start + p * bin + ...`: every step rounded once, as the restatement does

namespace {

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// ------------------------------------------------------------------------------------------------------------------ NMS
constexpr int NMS_BLOCK = 64;       // boxes per mask word
constexpr int NMS_SCAN_THREADS = 256;

// IoU in f32, each operation rounded once (contraction is off above; `/` is the correctly rounded IEEE division)
__device__ __forceinline__ float box_iou(const float4 a, const float area_a, const float4 b, const float area_b) {
    const float w = fmaxf(0.0f, fminf(a.z, b.z) - fmaxf(a.x, b.x));
    const float h = fmaxf(0.0f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}
__device__ __forceinline__ float box_area(const float4 b) { return (b.z - b.x) * (b.w - b.y); }

// Launch 1: workgroup (cb, rb), cb >= rb, compares the 64 boxes of row block rb (one per lane) with the 64 boxes of column block cb
// (staged in LDS) and writes one word per row: bit c set iff box cb*64+c comes later in the order, is of the row's group and
// overlaps it by more than the threshold.  Words left of the diagonal are never written and never read.
__global__ __launch_bounds__(NMS_BLOCK) void nms_mask_kernel(const float4 *__restrict__ boxes, const int32_t *__restrict__ groups,
                                                             unsigned long long *__restrict__ mask, int n, int n_blocks, float thr) {
    const int cb = blockIdx.x, rb = blockIdx.y;
    if (cb < rb) return;
    __shared__ float4 cbox[NMS_BLOCK];
    __shared__ int32_t cgrp[NMS_BLOCK];
    const int t = threadIdx.x;
    const int j0 = cb * NMS_BLOCK;
    const int n_col = min(NMS_BLOCK, n - j0);
    if (t < n_col) {
        cbox[t] = boxes[j0 + t];
        cgrp[t] = groups[j0 + t];
    }
    __syncthreads();
    const int i = rb * NMS_BLOCK + t;
    if (i >= n) return;
    const float4 a = boxes[i];
    const int32_t g = groups[i];
    const float area_a = box_area(a);
    unsigned long long bits = 0;
    for (int c = (cb == rb ? t + 1 : 0); c < n_col; ++c) {
        const float4 b = cbox[c];
        if (cgrp[c] == g && box_iou(a, area_a, b, box_area(b)) > thr) bits |= 1ull << c;
    }
    mask[(size_t)i * n_blocks + cb] = bits;
}

// Launch 2: ONE workgroup walks the row blocks in order.  `removed` (one bit per box, LDS) holds what the kept boxes so far
// suppress.  Per row block: every wave resolves the 64 rows of the block against each other from the block's diagonal words (the
// same 64-step walk in each wave: no barrier inside it), then all threads OR the rows that were kept into `removed` to the right of
// the diagonal -- (row, word) pairs dealt over the workgroup with the word index fastest, so that a wave reads runs of one mask
// row -- and one barrier closes the block.  The next block's diagonal words are loaded before the OR phase.
__global__ __launch_bounds__(NMS_SCAN_THREADS) void nms_scan_kernel(const unsigned long long *__restrict__ mask, uint8_t *__restrict__ keep,
                                                                    int32_t *__restrict__ count, int n, int n_blocks) {
    __shared__ unsigned long long removed[256];     // n <= 16 384
    const int tid = threadIdx.x, lane = tid & 63;
    for (int w = tid; w < n_blocks; w += NMS_SCAN_THREADS) removed[w] = 0;
    __syncthreads();
    int kept_total = 0;
    unsigned long long diag = lane < n ? mask[(size_t)lane * n_blocks] : 0ull;
    for (int rb = 0; rb < n_blocks; ++rb) {
        const int r0 = rb * NMS_BLOCK;
        const int rows = min(NMS_BLOCK, n - r0);
        unsigned long long next_diag = 0;
        if (rb + 1 < n_blocks && r0 + NMS_BLOCK + lane < n) next_diag = mask[(size_t)(r0 + NMS_BLOCK + lane) * n_blocks + rb + 1];
        unsigned long long cur = removed[rb], keepbits = 0;
        for (int t = 0; t < rows; ++t) {
            // (t is the same in every lane: two v_readlane, and the walk itself runs on the scalar unit)
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)diag, t);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(diag >> 32), t);
            if (!((cur >> t) & 1ull)) {
                keepbits |= 1ull << t;
                cur |= ((unsigned long long)hi << 32) | lo;
            }
        }
        kept_total += __popcll(keepbits);
        if (tid < rows) keep[r0 + tid] = (uint8_t)((keepbits >> tid) & 1ull);
        const int nw = n_blocks - rb - 1;      // words right of the diagonal
        if (nw > 0) {
            const int pairs = rows * nw;
            for (int p = tid; p < pairs; p += NMS_SCAN_THREADS) {
                const int t = p / nw, w = rb + 1 + (p - t * nw);
                if ((keepbits >> t) & 1ull) {
                    const unsigned long long m = mask[(size_t)(r0 + t) * n_blocks + w];
                    if (m) atomicOr(&removed[w], m);
                }
            }
        }
        __syncthreads();
        diag = next_diag;
    }
    if (tid == 0) *count = kept_total;
}

// ------------------------------------------------------------------------------------------------------------ RoIAlign
constexpr int ROI_THREADS = 256;
constexpr int ROI_LDS_BYTES = 60 * 1024;      // the [channels, P, P] tile of one chunk of channels

struct RoiArgs {
    sc2_roi_levels lv;
    const float *rois;
    const int32_t *levels;
    float *out;
    int n_levels, N, C, K, P, S, chunk;
};

template <bool BF16>
struct RoiVec;
template <>
struct RoiVec<false> {     // 4 f32 channels per 16-byte load
    static constexpr int V = 4;
    __device__ static __forceinline__ void load(const void *base, long long elem, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4 *>(static_cast<const float *>(base) + elem);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
};
template <>
struct RoiVec<true> {      // 8 bf16 channels per 16-byte load
    static constexpr int V = 8;
    __device__ static __forceinline__ void load(const void *base, long long elem, float (&v)[8]) {
        const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(base) + elem);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __builtin_bit_cast(float, w[i] << 16);
            v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xFFFF0000u);
        }
    }
};

// one axis of a bilinear sample (torchvision's bilinear_interpolate): -> false if the sample lies outside [-1, size] and counts 0
__device__ __forceinline__ bool roi_axis(float y, int size, int &low, int &high, float &l, float &h) {
    if (y < -1.0f || y > (float)size) return false;
    if (y <= 0.0f) y = 0.0f;
    low = max((int)y, 0);     // (y >= 0 here unless it is NaN: whatever the conversion makes of that stays inside the map)
    if (low >= size - 1) {
        high = low = size - 1;
        y = (float)low;
    } else {
        high = low + 1;
    }
    l = y - (float)low;
    h = 1.0f - l;
    return true;     // (a NaN coordinate passes both tests above and lands on pixel 0: inside the map)
}

// One workgroup per RoI.  Work items are (bin, channel vector) with the channel vector fastest: the lanes of a wave read runs of
// consecutive channels of one pixel (16 bytes each).  Results go to an LDS tile laid out [channel][bin] -- the order of the
// output -- which the workgroup then stores as one contiguous run of floats.  Channels are walked in chunks that fit the tile.
template <bool BF16>
__global__ __launch_bounds__(ROI_THREADS) void roi_align_kernel(const RoiArgs a) {
    constexpr int V = RoiVec<BF16>::V;
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int k = blockIdx.x;
    const int PP = a.P * a.P;
    float *out = a.out + (size_t)k * a.C * PP;
    const int lev = a.levels[k];
    const float *roi = a.rois + (size_t)k * 5;
    const float fimg = roi[0];
    const int img = (int)fimg;
    // the level's descriptor by comparison, not by a runtime index into the kernel argument (which would go through scratch)
    const void *data = nullptr;
    int H = 0, W = 0;
    float scale = 0.0f;
#pragma unroll
    for (int l = 0; l < SC2_ROI_MAX_LEVELS; ++l)
        if (l == lev && l < a.n_levels) {
            data = a.lv.level[l].data;
            H = a.lv.level[l].H;
            W = a.lv.level[l].W;
            scale = a.lv.level[l].spatial_scale;
        }
    if (data == nullptr || !(fimg >= 0.0f) || img >= a.N) {     // a level or an image that does not exist: NaN, and nothing is read
        const float qnan = __builtin_nanf("");
        for (int i = threadIdx.x; i < a.C * PP; i += ROI_THREADS) out[i] = qnan;
        return;
    }
    const float start_w = roi[1] * scale, start_h = roi[2] * scale, end_w = roi[3] * scale, end_h = roi[4] * scale;
    const float roi_w = fmaxf(end_w - start_w, 1.0f), roi_h = fmaxf(end_h - start_h, 1.0f);
    const float bin_w = roi_w / (float)a.P, bin_h = roi_h / (float)a.P;
    const float count = (float)(a.S * a.S);
    const long long img_base = (long long)img * H * W * a.C;

    for (int c0 = 0; c0 < a.C; c0 += a.chunk) {
        const int cc = min(a.chunk, a.C - c0);
        const int ncv = cc / V;                 // (C and the chunk are multiples of 8)
        const int items = PP * ncv;
        for (int it = threadIdx.x; it < items; it += ROI_THREADS) {
            const int bin = it / ncv, cv = it - bin * ncv;
            const int ph = bin / a.P, pw = bin - ph * a.P;
            const long long ch = img_base + c0 + cv * V;
            float acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.0f;
            for (int iy = 0; iy < a.S; ++iy) {
                const float y = start_h + (float)ph * bin_h + ((float)iy + 0.5f) * bin_h / (float)a.S;
                int yl, yh;
                float ly, hy;
                const bool y_in = roi_axis(y, H, yl, yh, ly, hy);
                for (int ix = 0; ix < a.S; ++ix) {
                    const float x = start_w + (float)pw * bin_w + ((float)ix + 0.5f) * bin_w / (float)a.S;
                    int xl, xh;
                    float lx, hx;
                    if (!roi_axis(x, W, xl, xh, lx, hx) || !y_in) continue;
                    const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                    float v1[V], v2[V], v3[V], v4[V];
                    RoiVec<BF16>::load(data, ch + ((long long)yl * W + xl) * a.C, v1);
                    RoiVec<BF16>::load(data, ch + ((long long)yl * W + xh) * a.C, v2);
                    RoiVec<BF16>::load(data, ch + ((long long)yh * W + xl) * a.C, v3);
                    RoiVec<BF16>::load(data, ch + ((long long)yh * W + xh) * a.C, v4);
#pragma unroll
                    for (int v = 0; v < V; ++v) acc[v] += w1 * v1[v] + w2 * v2[v] + w3 * v3[v] + w4 * v4[v];
                }
            }
#pragma unroll
            for (int v = 0; v < V; ++v) tile[(cv * V + v) * PP + bin] = acc[v] / count;
        }
        __syncthreads();
        float *dst = out + (size_t)c0 * PP;
        for (int i = threadIdx.x; i < cc * PP; i += ROI_THREADS) dst[i] = tile[i];
        __syncthreads();     // (the next chunk writes the tile again)
    }
}

inline int roi_chunk_channels(int C, int P) {
    int chunk = ROI_LDS_BYTES / (P * P * (int)sizeof(float)) / 8 * 8;
    return chunk > C ? C : chunk;
}

}  // namespace

extern "C" long long sc2_nms_ws_bytes(int n) {
    if (n <= 0 || n > SC2_NMS_MAX_BOXES) return 0;
    const long long nb = (n + NMS_BLOCK - 1) / NMS_BLOCK;
    return (long long)n * nb * 8;
}

extern "C" int sc2_nms(const float *boxes, const int32_t *groups, int n, float iou_threshold, uint8_t *keep, int32_t *count, void *ws,
                       void *stream) {
    SC2_REQUIRE(n >= 0, SC2_ERR_INVALID_ARG, "nms: n=%d", n);
    SC2_REQUIRE(n <= SC2_NMS_MAX_BOXES, SC2_ERR_UNSUPPORTED, "nms: %d boxes in one call (at most %d: split the input by group)", n,
                SC2_NMS_MAX_BOXES);
    SC2_REQUIRE(count, SC2_ERR_INVALID_ARG, "nms: null count");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {     // nothing is launched: the count is cleared by a stream-ordered fill
        if (hipMemsetAsync(count, 0, sizeof(int32_t), s) != hipSuccess) {
            sc2_set_error("nms: cannot clear the count");
            return SC2_ERR_LAUNCH;
        }
        return SC2_OK;
    }
    SC2_REQUIRE(boxes && groups && keep && ws, SC2_ERR_INVALID_ARG, "nms: null argument");
    SC2_REQUIRE(aligned16(boxes) && aligned8(ws), SC2_ERR_INVALID_ARG, "nms: boxes must be 16-byte and the workspace 8-byte aligned");
    SC2_REQUIRE(iou_threshold == iou_threshold, SC2_ERR_INVALID_ARG, "nms: the threshold is NaN");
    const int nb = (n + NMS_BLOCK - 1) / NMS_BLOCK;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(nb, nb), dim3(NMS_BLOCK), 0, s, reinterpret_cast<const float4 *>(boxes), groups,
                       static_cast<unsigned long long *>(ws), n, nb, iou_threshold);
    SC2_CHECK_LAUNCH();
    hipLaunchKernelGGL(nms_scan_kernel, dim3(1), dim3(NMS_SCAN_THREADS), 0, s, static_cast<const unsigned long long *>(ws), keep, count, n,
                       nb);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_roi_align(sc2_roi_levels lv, int n_levels, int N, int C, int is_bf16, const float *rois, const int32_t *levels, int K,
                             int P, int sampling_ratio, float *out, void *stream) {
    SC2_REQUIRE(n_levels >= 1 && n_levels <= SC2_ROI_MAX_LEVELS, SC2_ERR_INVALID_ARG, "roi_align: %d levels (1..%d)", n_levels,
                SC2_ROI_MAX_LEVELS);
    SC2_REQUIRE(N > 0 && C > 0 && C % 8 == 0, SC2_ERR_INVALID_ARG, "roi_align: bad dims N=%d C=%d (C %% 8 == 0)", N, C);
    SC2_REQUIRE(P >= 1 && P <= 14, SC2_ERR_INVALID_ARG, "roi_align: pooled size %d (1..14)", P);
    SC2_REQUIRE(sampling_ratio >= 1 && sampling_ratio <= 16, SC2_ERR_INVALID_ARG,
                "roi_align: sampling_ratio %d (1..16; the adaptive form, <= 0, is not built)", sampling_ratio);
    SC2_REQUIRE(K >= 0, SC2_ERR_INVALID_ARG, "roi_align: K=%d", K);
    for (int l = 0; l < n_levels; ++l) {
        const sc2_roi_level &d = lv.level[l];
        SC2_REQUIRE(d.data && aligned16(d.data), SC2_ERR_INVALID_ARG, "roi_align: level %d: null or not 16-byte aligned", l);
        SC2_REQUIRE(d.H > 0 && d.W > 0 && d.spatial_scale > 0.0f, SC2_ERR_INVALID_ARG, "roi_align: level %d: H=%d W=%d scale=%g", l, d.H,
                    d.W, (double)d.spatial_scale);
    }
    if (K == 0) return SC2_OK;
    SC2_REQUIRE(rois && levels && out, SC2_ERR_INVALID_ARG, "roi_align: null argument");
    RoiArgs a;
    a.lv = lv;
    a.rois = rois;
    a.levels = levels;
    a.out = out;
    a.n_levels = n_levels;
    a.N = N;
    a.C = C;
    a.K = K;
    a.P = P;
    a.S = sampling_ratio;
    a.chunk = roi_chunk_channels(C, P);
    const size_t lds = (size_t)a.chunk * P * P * sizeof(float);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (is_bf16)
        hipLaunchKernelGGL(roi_align_kernel<true>, dim3((unsigned)K), dim3(ROI_THREADS), lds, s, a);
    else
        hipLaunchKernelGGL(roi_align_kernel<false>, dim3((unsigned)K), dim3(ROI_THREADS), lds, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
