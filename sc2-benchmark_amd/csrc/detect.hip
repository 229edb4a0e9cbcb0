// Detection tail (Faster R-CNN behind the feature pyramid): the two operations of torchvision's inference path that have no
// torch-op equivalent -- greedy non-maximum suppression with groups (`batched_nms`, run per pyramid level on the RPN's proposals
// and per class on the detections) and multi-level RoIAlign (`MultiScaleRoIAlign`, aligned=False) -- and the two of its training
// path that have no reasonable one: the proposal matcher (`Matcher` over `box_iou`, without the IoU matrix) and the backward of
// RoIAlign.  include/sc2_bottleneck.h states the contract; tests/ref_detection.py and tests/ref_det_train.py restate it.
// Plain kernels: no atomics on global memory, no workgroup waits for another, every index checked against its array before use.
#include "sc2_common.h"

#pragma clang fp contract(off)   // `area_a + area_b - w * h`, `start + p * bin + ...`: every step rounded once, as the restatement does

#include "detect_common.h"      // box_iou / box_area, the alignment tests, match_range / match_offsets_ok (shared with det_post.hip)

namespace {

// ------------------------------------------------------------------------------------------------------------------ NMS
constexpr int NMS_BLOCK = 64;       // boxes per mask word
constexpr int NMS_SCAN_THREADS = 256;

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

// --------------------------------------------------------------------------------------------------- RoIAlign backward
// The adjoint of roi_align_kernel with respect to the f32 maps, as a GATHER: one workgroup owns an 8 x 8 pixel tile of one
// (level, image) map for every channel and walks those of the map's RoIs that can touch the tile in ascending index (the caller bins them: `order` lists the RoI
// indices bin by bin, bin = level * N + image, `bin_off` the bins' bounds).  The validity of a sample is the AND of its two axes and
// its bilinear weight the product of two axis weights, so a RoI's contribution to pixel (y, x) is
//     sum_{ph, pw}  By[y][ph] * Bx[x][pw] * g[k, c, ph, pw] / S^2,      By[y][ph] = sum_i (weight of sample (ph, i) on row y)
// with both weight tables a few dozen floats per RoI (LDS) from the forward's own roi_axis.  g[k] of one channel chunk is staged in
// LDS as it lies in memory ([channel][bin]: one contiguous run, read back with the channel across the lanes at the odd stride P * P).
// Every element of every map is written exactly once, by one thread, from sums taken in a fixed order: no atomics, same bits each call.
constexpr int RB_THREADS = 256;
constexpr int RB_TILE = 8;                    // pixels per tile side (the weight tables' thread layout is written for 8)
constexpr int RB_MAX_CHUNK = 256;             // channels per pass: 64 pixels x 64 channel vectors = 16 float4 accumulators per thread
constexpr int RB_ITEMS = RB_TILE * RB_TILE * (RB_MAX_CHUNK / 4) / RB_THREADS;
constexpr int RB_LDS_BYTES = 50 * 1024;       // g of one RoI and channel chunk: 256 x 49 floats at P = 7

struct RoiBwdArgs {
    sc2_roi_levels lv;                        // data: the gradient maps (written)
    int tile_start[SC2_ROI_MAX_LEVELS + 1];   // first workgroup of each level; [n_levels] = the grid
    const float *grad_out;
    const float *rois;
    const int32_t *levels;
    const int32_t *order;
    const int32_t *bin_off;
    int n_levels, N, C, K, P, S, chunk;
};

__global__ __launch_bounds__(RB_THREADS) void roi_align_backward_kernel(const RoiBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gtile[];     // [chunk][P * P], already divided by S^2
    __shared__ float By[RB_TILE][14], Bx[RB_TILE][14];
    __shared__ unsigned long long hits[RB_THREADS / 64], wmask[RB_THREADS / 64];
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    float *data = nullptr;
    int H = 0, W = 0, lev = -1, first = 0;
    float scale = 0.0f;
#pragma unroll
    for (int l = 0; l < SC2_ROI_MAX_LEVELS; ++l)
        if (l < a.n_levels && wg >= a.tile_start[l] && wg < a.tile_start[l + 1]) {
            data = static_cast<float *>(const_cast<void *>(a.lv.level[l].data));
            H = a.lv.level[l].H;
            W = a.lv.level[l].W;
            scale = a.lv.level[l].spatial_scale;
            lev = l;
            first = a.tile_start[l];
        }
    if (lev < 0) return;
    const int tiles_x = (W + RB_TILE - 1) / RB_TILE, tiles_y = (H + RB_TILE - 1) / RB_TILE;
    const int rel = wg - first;
    const int img = rel / (tiles_x * tiles_y);
    if (img >= a.N) return;
    const int tile = rel - img * tiles_x * tiles_y;
    const int ty0 = tile / tiles_x * RB_TILE, tx0 = (tile - tile / tiles_x * tiles_x) * RB_TILE;
    const int bin = lev * a.N + img;
    const int j0 = min(max(a.bin_off[bin], 0), a.K), j1 = min(max(a.bin_off[bin + 1], j0), a.K);
    const int PP = a.P * a.P;
    const float count = (float)(a.S * a.S);
    float *map = data + (size_t)img * H * W * a.C;

    for (int c0 = 0; c0 < a.C; c0 += a.chunk) {
        const int cc = min(a.chunk, a.C - c0);
        const int ncv = cc / 4;
        const int items = RB_TILE * RB_TILE * ncv;
        float acc[RB_ITEMS][4];
#pragma unroll
        for (int i = 0; i < RB_ITEMS; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[i][v] = 0.0f;
        for (int base = j0; base < j1; base += RB_THREADS) {
            // 256 RoIs of the bin at a time, one per thread: which of them can touch the tile at all?  The answers go to LDS as one
            // ballot per wave, and the workgroup then takes the hits in ascending order.
            {
                bool hit = false;
                const int jj = base + tid;
                if (jj < j1) {
                    const int kk = a.order[jj];
                    if (kk >= 0 && kk < a.K) {
                        const float *r = a.rois + (size_t)kk * 5;
                        const float fi = r[0];
                        if (a.levels[kk] == lev && fi >= 0.0f && (int)fi == img) {     // (a bin that lists a stranger: nothing of it counts)
                            const float sw = r[1] * scale, sh = r[2] * scale;
                            const float rw = fmaxf(r[3] * scale - sw, 1.0f), rh = fmaxf(r[4] * scale - sh, 1.0f);
                            // every sample lies inside [start, start + size] up to rounding, and touches floor(y) and floor(y) + 1
                            // after the clamps: two pixels of slack on either side cover both
                            hit = sh - 2.0f <= (float)(ty0 + RB_TILE - 1) && sh + rh + 2.0f >= (float)ty0 &&
                                  sw - 2.0f <= (float)(tx0 + RB_TILE - 1) && sw + rw + 2.0f >= (float)tx0;
                        }
                    }
                }
                const unsigned long long wave_hits = __ballot(hit);
                __syncthreads();     // the previous batch's ballots are read no more
                if ((tid & 63) == 0) hits[tid >> 6] = wave_hits;
                __syncthreads();
            }
            for (int wv = 0; wv < RB_THREADS / 64; ++wv) {
                unsigned long long todo = hits[wv];
                while (todo) {
                    const int j = base + wv * 64 + __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const int k = a.order[j];      // (checked by the thread that voted for it)
                    const float *roi = a.rois + (size_t)k * 5;
                    const float start_w = roi[1] * scale, start_h = roi[2] * scale, end_w = roi[3] * scale, end_h = roi[4] * scale;
                    const float roi_w = fmaxf(end_w - start_w, 1.0f), roi_h = fmaxf(end_h - start_h, 1.0f);
                    const float bin_w = roi_w / (float)a.P, bin_h = roi_h / (float)a.P;
                    __syncthreads();     // the previous RoI's tables and tile are read no more
                    {     // thread (axis, pixel r of the tile, bin p): waves 0 - 1 hold the rows, 2 - 3 the columns, 4 pixels x 16 bins each
                        const bool is_x = tid >= RB_THREADS / 2;
                        const int r = (tid >> 4) & (RB_TILE - 1), p = tid & 15;
                        const int pix = (is_x ? tx0 : ty0) + r, size = is_x ? W : H;
                        const float start = is_x ? start_w : start_h, bsz = is_x ? bin_w : bin_h;
                        float wsum = 0.0f;
                        if (p < a.P) {
                            for (int i = 0; i < a.S; ++i) {
                                const float y = start + (float)p * bsz + ((float)i + 0.5f) * bsz / (float)a.S;     // the forward's expression
                                int lo, hi;
                                float l, h;
                                if (!roi_axis(y, size, lo, hi, l, h)) continue;
                                if (lo == pix) wsum += h;
                                if (hi == pix) wsum += l;
                            }
                            if (is_x) Bx[r][p] = wsum; else By[r][p] = wsum;
                        }
                        const unsigned long long nonzero = __ballot(wsum != 0.0f);     // which bins reach which pixel: 16 bits per pixel
                        if ((tid & 63) == 0) wmask[tid >> 6] = nonzero;
                    }
                    const float *g = a.grad_out + ((size_t)k * a.C + c0) * PP;
                    for (int i = tid; i < cc * PP; i += RB_THREADS) gtile[i] = g[i] / count;
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < RB_ITEMS; ++i) {
                        const int it = tid + i * RB_THREADS;
                        if (it >= items) continue;
                        const int pix = it / ncv, cv = it - pix * ncv;
                        const int r = pix / RB_TILE, cx = pix - r * RB_TILE;
                        const float *gc = gtile + cv * 4 * PP;
                        const unsigned my = (unsigned)(wmask[r >> 2] >> ((r & 3) * 16)) & 0xFFFFu;
                        const unsigned mx = (unsigned)(wmask[2 + (cx >> 2)] >> ((cx & 3) * 16)) & 0xFFFFu;
                        if (mx == 0) continue;
                        for (unsigned m = my; m; m &= m - 1) {      // ascending bins with a weight on this pixel
                            const int ph = __ffs((int)m) - 1;
                            const float wy = By[r][ph];
                            for (unsigned n = mx; n; n &= n - 1) {
                                const int pw = __ffs((int)n) - 1;
                                const float w = wy * Bx[cx][pw];
                                const int b = ph * a.P + pw;
#pragma unroll
                                for (int v = 0; v < 4; ++v) acc[i][v] += w * gc[v * PP + b];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < RB_ITEMS; ++i) {
            const int it = tid + i * RB_THREADS;
            if (it >= items) continue;
            const int pix = it / ncv, cv = it - pix * ncv;
            const int y = ty0 + pix / RB_TILE, x = tx0 + pix % RB_TILE;
            if (y < H && x < W)
                *reinterpret_cast<float4 *>(map + ((size_t)y * W + x) * a.C + c0 + cv * 4) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        }
    }
}

inline int roi_bwd_chunk_channels(int C, int P) {
    int chunk = RB_LDS_BYTES / (P * P * (int)sizeof(float)) / 8 * 8;
    if (chunk > RB_MAX_CHUNK) chunk = RB_MAX_CHUNK;
    return chunk > C ? C : chunk;
}

// ------------------------------------------------------------------------------------------------------------ box matcher
constexpr int MATCH_THREADS = 256;
constexpr int MATCH_GT_TILE = 64;             // gt boxes staged in LDS at a time
constexpr int MATCH_MAX_PER_THREAD = 8;       // launch 1: candidates a thread holds in registers
constexpr int MATCH_MAX_CHUNK = MATCH_THREADS * MATCH_MAX_PER_THREAD;     // ... and a workgroup covers (SC2_MATCH_CHUNK)
constexpr int MATCH_CAND_PER_THREAD = 4;
constexpr int MATCH_CAND_PER_WG = MATCH_THREADS * MATCH_CAND_PER_THREAD;   // launch 2: candidates per workgroup
static_assert(MATCH_MAX_CHUNK == SC2_MATCH_CHUNK, "the workspace is sized by SC2_MATCH_CHUNK");

struct MatchArgs {
    const float4 *gt, *cand;
    const int32_t *gt_off, *cand_off;
    float *ws;                 // [chunk of the image][total_gt]: per-gt maxima over one chunk of candidates
    int32_t *matches;
    float *best_iou;
    int n_img, total_gt, total_cand, allow_low_quality, ws_rows;     // ws_rows: the chunks the workspace holds
    float low, high;
};

// Launch 1: workgroup (chunk, image): the maximum IoU of every gt box of the image over candidates [chunk * 2048, +2048) of it.
// A thread holds eight candidates in registers; per gt box a wave reduces by shuffles, the four waves through LDS.
__global__ __launch_bounds__(MATCH_THREADS) void match_gtmax_kernel(const MatchArgs a) {
    __shared__ float4 gbox[MATCH_GT_TILE];
    __shared__ float wmax[MATCH_THREADS / 64][MATCH_GT_TILE];
    const int img = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    int g0, g1, a0, a1;
    match_range(a.gt_off, img, a.total_gt, g0, g1);
    match_range(a.cand_off, img, a.total_cand, a0, a1);
    const long long cbeg = (long long)a0 + (long long)chunk * MATCH_MAX_CHUNK;
    if (g1 == g0 || cbeg >= a1) return;
    const int n = (int)min((long long)MATCH_MAX_CHUNK, (long long)a1 - cbeg);
    float4 c[MATCH_MAX_PER_THREAD];
    float area[MATCH_MAX_PER_THREAD];
#pragma unroll
    for (int i = 0; i < MATCH_MAX_PER_THREAD; ++i) {
        const int q = i * MATCH_THREADS + tid;
        c[i] = q < n ? a.cand[cbeg + q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        area[i] = box_area(c[i]);
    }
    const float ninf = -__builtin_inff();
    for (int t0 = g0; t0 < g1; t0 += MATCH_GT_TILE) {
        const int ng = min(MATCH_GT_TILE, g1 - t0);
        __syncthreads();
        if (tid < ng) gbox[tid] = a.gt[t0 + tid];
        __syncthreads();
        for (int g = 0; g < ng; ++g) {
            const float4 b = gbox[g];
            const float area_b = box_area(b);
            float m = ninf;
#pragma unroll
            for (int i = 0; i < MATCH_MAX_PER_THREAD; ++i) {
                const float v = box_iou(b, area_b, c[i], area[i]);
                if (i * MATCH_THREADS + tid < n && v > m) m = v;     // (NaN > m is false: never the maximum)
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));     // (no NaN among them)
            if ((tid & 63) == 0) wmax[tid >> 6][g] = m;
        }
        __syncthreads();
        if (tid < ng) {
            float m = wmax[0][tid];
#pragma unroll
            for (int w = 1; w < MATCH_THREADS / 64; ++w) m = fmaxf(m, wmax[w][tid]);
            a.ws[(size_t)chunk * a.total_gt + t0 + tid] = m;
        }
    }
}

// Launch 2: workgroup (block of 1024 candidates, image).  Per gt tile: the boxes and their maxima over the image's candidates (the
// chunks of launch 1 folded: a max, whose order does not matter) go to LDS, then every thread walks the tile for its four candidates.
__global__ __launch_bounds__(MATCH_THREADS) void match_assign_kernel(const MatchArgs a) {
    __shared__ float4 gbox[MATCH_GT_TILE];
    __shared__ float gmax[MATCH_THREADS / 64][MATCH_GT_TILE];
    const int img = blockIdx.y, tid = threadIdx.x;
    int g0, g1, a0, a1;
    match_range(a.gt_off, img, a.total_gt, g0, g1);
    match_range(a.cand_off, img, a.total_cand, a0, a1);
    const long long cbeg = (long long)a0 + (long long)blockIdx.x * MATCH_CAND_PER_WG;
    if (cbeg >= a1) return;
    const int n = (int)min((long long)MATCH_CAND_PER_WG, (long long)a1 - cbeg);
    if (g1 == g0) {     // no gt box: everything is background, and nothing of the gt array is read
        for (int q = tid; q < n; q += MATCH_THREADS) {
            a.matches[cbeg + q] = -1;
            if (a.best_iou) a.best_iou[cbeg + q] = 0.0f;
        }
        return;
    }
    const int n_chunks = min((a1 - a0 + MATCH_MAX_CHUNK - 1) / MATCH_MAX_CHUNK, a.ws_rows);
    float4 c[MATCH_CAND_PER_THREAD];
    float area[MATCH_CAND_PER_THREAD], best[MATCH_CAND_PER_THREAD];
    int idx[MATCH_CAND_PER_THREAD];
    bool restore[MATCH_CAND_PER_THREAD];
#pragma unroll
    for (int i = 0; i < MATCH_CAND_PER_THREAD; ++i) {
        const int q = i * MATCH_THREADS + tid;
        c[i] = q < n ? a.cand[cbeg + q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        area[i] = box_area(c[i]);
        best[i] = -__builtin_inff();
        idx[i] = 0;
        restore[i] = false;
    }
    for (int t0 = g0; t0 < g1; t0 += MATCH_GT_TILE) {
        const int ng = min(MATCH_GT_TILE, g1 - t0);
        __syncthreads();
        {
            const int g = tid & 63, part = tid >> 6;
            float m = -__builtin_inff();
            if (g < ng && a.allow_low_quality)
                for (int ch = part; ch < n_chunks; ch += MATCH_THREADS / 64) m = fmaxf(m, a.ws[(size_t)ch * a.total_gt + t0 + g]);
            gmax[part][g] = m;
            if (tid < ng) gbox[tid] = a.gt[t0 + tid];
        }
        __syncthreads();
        for (int g = 0; g < ng; ++g) {
            const float4 b = gbox[g];
            const float area_b = box_area(b);
            const float top = fmaxf(fmaxf(gmax[0][g], gmax[1][g]), fmaxf(gmax[2][g], gmax[3][g]));
#pragma unroll
            for (int i = 0; i < MATCH_CAND_PER_THREAD; ++i) {
                const float v = box_iou(b, area_b, c[i], area[i]);     // the operand order of launch 1: the same bits
                if (v > best[i]) {      // strictly: a tie stays with the lower gt index, a NaN never wins
                    best[i] = v;
                    idx[i] = t0 - g0 + g;
                }
                if (a.allow_low_quality && v == top) restore[i] = true;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MATCH_CAND_PER_THREAD; ++i) {
        const int q = i * MATCH_THREADS + tid;
        if (q >= n) continue;
        int m = best[i] < a.low ? -1 : (best[i] < a.high ? -2 : idx[i]);
        if (restore[i]) m = idx[i];
        a.matches[cbeg + q] = m;
        if (a.best_iou) a.best_iou[cbeg + q] = best[i];
    }
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

extern "C" long long sc2_box_match_ws_bytes(int total_gt, int max_candidates) {
    if (total_gt <= 0 || max_candidates <= 0) return 0;
    const long long chunks = ((long long)max_candidates + SC2_MATCH_CHUNK - 1) / SC2_MATCH_CHUNK;
    return chunks * total_gt * (long long)sizeof(float);
}

extern "C" int sc2_box_match(const float *gt, const int32_t *gt_off, const float *cand, const int32_t *cand_off, const int32_t *gt_off_host,
                             const int32_t *cand_off_host, int n_img, int total_gt, int total_cand, float low, float high,
                             int allow_low_quality, int32_t *matches, float *best_iou, void *ws, void *stream) {
    SC2_REQUIRE(n_img >= 0 && n_img <= 65535, SC2_ERR_INVALID_ARG, "box_match: %d images (0..65535)", n_img);
    SC2_REQUIRE(total_gt >= 0 && total_cand >= 0, SC2_ERR_INVALID_ARG, "box_match: totals %d, %d", total_gt, total_cand);
    SC2_REQUIRE(gt_off_host && cand_off_host, SC2_ERR_INVALID_ARG, "box_match: the host copy of the offsets is missing");
    SC2_REQUIRE(low == low && high == high, SC2_ERR_INVALID_ARG, "box_match: a threshold is NaN");
    int longest_gt = 0, longest = 0;
    SC2_REQUIRE(match_offsets_ok(gt_off_host, n_img, total_gt, longest_gt), SC2_ERR_INVALID_ARG,
                "box_match: gt offsets must start at 0, never decrease and end at %d", total_gt);
    SC2_REQUIRE(match_offsets_ok(cand_off_host, n_img, total_cand, longest), SC2_ERR_INVALID_ARG,
                "box_match: candidate offsets must start at 0, never decrease and end at %d", total_cand);
    if (n_img == 0 || total_cand == 0) return SC2_OK;
    SC2_REQUIRE(cand && gt_off && cand_off && matches, SC2_ERR_INVALID_ARG, "box_match: null argument");
    SC2_REQUIRE(aligned16(cand), SC2_ERR_INVALID_ARG, "box_match: candidates must be 16-byte aligned");
    SC2_REQUIRE(total_gt == 0 || (gt && aligned16(gt) && ws), SC2_ERR_INVALID_ARG, "box_match: gt boxes (16-byte aligned) or workspace missing");
    MatchArgs a;
    a.gt = reinterpret_cast<const float4 *>(gt);
    a.cand = reinterpret_cast<const float4 *>(cand);
    a.gt_off = gt_off;
    a.cand_off = cand_off;
    a.ws = static_cast<float *>(ws);
    a.matches = matches;
    a.best_iou = best_iou;
    a.n_img = n_img;
    a.total_gt = total_gt;
    a.total_cand = total_cand;
    a.allow_low_quality = allow_low_quality ? 1 : 0;
    a.low = low;
    a.high = high;
    a.ws_rows = (longest + MATCH_MAX_CHUNK - 1) / MATCH_MAX_CHUNK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (total_gt > 0 && a.allow_low_quality) {
        hipLaunchKernelGGL(match_gtmax_kernel, dim3((unsigned)a.ws_rows, (unsigned)n_img),
                           dim3(MATCH_THREADS), 0, s, a);
        SC2_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(match_assign_kernel, dim3((unsigned)((longest + MATCH_CAND_PER_WG - 1) / MATCH_CAND_PER_WG), (unsigned)n_img),
                       dim3(MATCH_THREADS), 0, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_roi_align_backward(sc2_roi_levels lv, int n_levels, int N, int C, const float *grad_out, const float *rois,
                                      const int32_t *levels, const int32_t *order, const int32_t *bin_off, int K, int P, int sampling_ratio,
                                      void *stream) {
    SC2_REQUIRE(n_levels >= 1 && n_levels <= SC2_ROI_MAX_LEVELS, SC2_ERR_INVALID_ARG, "roi_align_backward: %d levels (1..%d)", n_levels,
                SC2_ROI_MAX_LEVELS);
    SC2_REQUIRE(N > 0 && C > 0 && C % 8 == 0, SC2_ERR_INVALID_ARG, "roi_align_backward: bad dims N=%d C=%d (C %% 8 == 0)", N, C);
    SC2_REQUIRE(P >= 1 && P <= 14, SC2_ERR_INVALID_ARG, "roi_align_backward: pooled size %d (1..14)", P);
    SC2_REQUIRE(sampling_ratio >= 1 && sampling_ratio <= 16, SC2_ERR_INVALID_ARG, "roi_align_backward: sampling_ratio %d (1..16)",
                sampling_ratio);
    SC2_REQUIRE(K >= 0, SC2_ERR_INVALID_ARG, "roi_align_backward: K=%d", K);
    SC2_REQUIRE(bin_off, SC2_ERR_INVALID_ARG, "roi_align_backward: null bin offsets");
    SC2_REQUIRE(K == 0 || (grad_out && rois && levels && order), SC2_ERR_INVALID_ARG, "roi_align_backward: null argument");
    RoiBwdArgs a;
    long long tiles = 0;
    for (int l = 0; l < n_levels; ++l) {
        const sc2_roi_level &d = lv.level[l];
        SC2_REQUIRE(d.data && aligned16(d.data), SC2_ERR_INVALID_ARG, "roi_align_backward: level %d: null or not 16-byte aligned", l);
        SC2_REQUIRE(d.H > 0 && d.W > 0 && d.spatial_scale > 0.0f, SC2_ERR_INVALID_ARG, "roi_align_backward: level %d: H=%d W=%d scale=%g", l,
                    d.H, d.W, (double)d.spatial_scale);
        a.tile_start[l] = (int)tiles;
        tiles += (long long)N * ((d.H + RB_TILE - 1) / RB_TILE) * ((d.W + RB_TILE - 1) / RB_TILE);
        SC2_REQUIRE(tiles < (1ll << 31), SC2_ERR_UNSUPPORTED, "roi_align_backward: more than 2^31 pixel tiles");
    }
    for (int l = n_levels; l <= SC2_ROI_MAX_LEVELS; ++l) a.tile_start[l] = (int)tiles;
    a.lv = lv;
    a.grad_out = grad_out;
    a.rois = rois;
    a.levels = levels;
    a.order = order;
    a.bin_off = bin_off;
    a.n_levels = n_levels;
    a.N = N;
    a.C = C;
    a.K = K;
    a.P = P;
    a.S = sampling_ratio;
    a.chunk = roi_bwd_chunk_channels(C, P);
    const size_t lds = (size_t)a.chunk * P * P * sizeof(float);
    hipLaunchKernelGGL(roi_align_backward_kernel, dim3((unsigned)tiles), dim3(RB_THREADS), lds, static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
