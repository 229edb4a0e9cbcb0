// The RoI heads' post-processing (torchvision's `RoIHeads.postprocess_detections`) for a whole batch in three launches: from the
// box predictor's two outputs to the padded per-image detections, nothing of it on the host.  include/sc2_bottleneck.h states
// the contract (sc2_det_postprocess); tests/ref_det_post.py restates it.
//   launch 1  a wave per proposal row: softmax, per-class decode, clip -> the candidate table [R, C-1] and a survivor bitmap per row
//   launch 2  a workgroup per (image, class): the class's survivors sorted by (score descending, flat index ascending) in LDS,
//             greedy NMS in that order, the keys of the first D kept
//   launch 3  a workgroup per image: the classes' kept lists (each in order already) merged into the first D of the image
// Plain kernels, as detect.hip's: no atomics on global memory, no workgroup waits for another, every index checked against its
// array before use.  A candidate's place in every list follows from its key alone (score bits, then flat index: unique within an
// image), so two calls give the same bits.
#include "sc2_common.h"

#pragma clang fp contract(off)   // BoxCoder.decode_single's `dx * widths + ctr_x` and the IoU: every step rounded once

#include "detect_common.h"

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_ROWS_PER_WG = DP_THREADS / 64;     // launch 1: one wave per row
constexpr int DP_SEG = SC2_DETPOST_MAX_SEG;         // launch 2: survivors of one (image, class) held in LDS
constexpr int DP_HEAD = 16;                         // launch 3: keys of a class's kept list staged in LDS at a time
static_assert((DP_SEG & (DP_SEG - 1)) == 0, "the segment is sorted as a power of two");
static_assert(SC2_DETPOST_MAX_CLASSES <= 128, "a lane of launch 1 and launch 3 owns classes lane and lane + 64");

struct DetPostArgs {
    const float *logits, *deltas;
    const float4 *proposals;
    const int32_t *off, *sizes;
    float *cand_scores;               // [R, C-1]     (the workspace's, or the caller's test hook)
    float4 *cand_boxes;               // [R, C-1]
    unsigned long long *bitmap;       // [R, 2]: bit c-1 of a row set iff candidate (row, c) survives
    unsigned long long *keys;         // [n, C-1, D]: the first D kept of a class, in order
    int32_t *seg_count, *kept_count;  // [n, C-1]: survivors / kept (at most D) of a class
    float *boxes, *scores;
    int64_t *labels;
    int32_t *count, *status;
    int R, C, n, D;
    float wx, wy, ww, wh, clip, score_thresh, min_size, nms_thresh;
};

// 64-bit key of a survivor: greater = earlier.  High word: the score's bits mapped so that unsigned order is the floats' order;
// low word: the complement of the flat index r_local * (C-1) + (c-1), so that of two equal scores the LOWER index is greater.
__device__ __forceinline__ unsigned long long cand_key(float score, unsigned flat) {
    return ((unsigned long long)float_order_bits(score) << 32) | (0xFFFFFFFFu - flat);
}
__device__ __forceinline__ unsigned key_flat(unsigned long long k) { return 0xFFFFFFFFu - (unsigned)k; }

// Launch 1.  Lane l owns classes l and l + 64 of its wave's row.  Maximum and sum go through the same xor butterfly in every lane
// (both operands of each step are the two lanes' values: commutative, so all lanes hold the same bits): a fixed tree.
__global__ __launch_bounds__(DP_THREADS) void detpost_rows_kernel(const DetPostArgs a) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * DP_ROWS_PER_WG + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int C = a.C, nc = C - 1;
    // the row's image: the last i with off[i] <= r (offsets clamped to 0..R; a row behind off[n] belongs to no image)
    int lo = 0, hi = a.n;     // invariant: off[lo] <= r (off[0] is read as 0), off[hi + 1 ...] > r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (min(max(a.off[mid], 0), a.R) <= r) lo = mid; else hi = mid - 1;
    }
    const bool has_image = lo < a.n;
    float img_h = 0.0f, img_w = 0.0f;
    if (has_image) {
        img_h = (float)a.sizes[2 * lo];
        img_w = (float)a.sizes[2 * lo + 1];
    }
    const float *lg = a.logits + (size_t)r * C;
    const int c0 = lane, c1 = lane + 64;
    const float ninf = -__builtin_inff();
    const float l0 = c0 < C ? lg[c0] : ninf, l1 = c1 < C ? lg[c1] : ninf;
    float m = fmaxf(l0, l1);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    // (a NaN logit drops out of the maximum and comes back through its own exponential: the sum, hence every score, is NaN)
    const float e0 = c0 < C ? expf(l0 - m) : 0.0f, e1 = c1 < C ? expf(l1 - m) : 0.0f;
    float s = e0 + e1;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d, 64);
    const float4 p = a.proposals[r];
    const float4 weights = make_float4(a.wx, a.wy, a.ww, a.wh);
    bool pass[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = h ? c1 : c0;
        pass[h] = false;
        if (c < 1 || c >= C) continue;
        const float score = (h ? e1 : e0) / s;
        const float4 dl = *reinterpret_cast<const float4 *>(a.deltas + ((size_t)r * C + c) * 4);
        const float4 b = decode_clip_box(p, dl, weights, a.clip, img_w, img_h);
        const size_t at = (size_t)r * nc + (c - 1);
        a.cand_scores[at] = score;
        a.cand_boxes[at] = b;
        pass[h] = has_image && score > a.score_thresh && (b.z - b.x) >= a.min_size && (b.w - b.y) >= a.min_size;
    }
    const unsigned long long b0 = __ballot(pass[0]), b1 = __ballot(pass[1]);     // bit l: class l / class l + 64
    if (lane == 0) {
        a.bitmap[2 * (size_t)r] = (b0 >> 1) | (b1 << 63);      // bit c - 1
        a.bitmap[2 * (size_t)r + 1] = b1 >> 1;
    }
}

// Launch 2: workgroup (class - 1, image).
__global__ __launch_bounds__(DP_THREADS) void detpost_class_kernel(const DetPostArgs a) {
    __shared__ unsigned long long key[DP_SEG];
    __shared__ float4 box[DP_SEG];
    __shared__ uint8_t sup[DP_SEG];
    __shared__ int members;
    const int cls = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const int nc = a.C - 1;
    int r0, r1;
    match_range(a.off, img, a.R, r0, r1);
    if (tid == 0) members = 0;
    __syncthreads();
    // the class's survivors, in whatever order the threads arrive: their place afterwards follows from the keys alone
    const int word = cls >> 6, bit = cls & 63;
    for (int rr = tid; rr < r1 - r0; rr += DP_THREADS) {
        const size_t row = (size_t)r0 + rr;
        if (!((a.bitmap[2 * row + word] >> bit) & 1ull)) continue;
        const int slot = atomicAdd(&members, 1);     // (LDS)
        if (slot < DP_SEG) key[slot] = cand_key(a.cand_scores[row * nc + cls], (unsigned)rr * (unsigned)nc + (unsigned)cls);
    }
    __syncthreads();
    const int m = members;
    const size_t list = (size_t)img * nc + cls;
    if (tid == 0) a.seg_count[list] = m;
    if (m == 0 || m > DP_SEG) {     // nothing to do / above the segment cap: launch 3 sets the image's status from the count
        if (tid == 0) a.kept_count[list] = 0;
        return;
    }
    int P = 1;
    while (P < m) P <<= 1;
    for (int t = m + tid; t < P; t += DP_THREADS) key[t] = 0;     // (below every key)
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)     // bitonic sort, descending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P; t += DP_THREADS) {
                const int u = t ^ j;
                if (u > t) {
                    const unsigned long long x = key[t], y = key[u];
                    if ((x < y) == ((t & k) == 0)) {
                        key[t] = y;
                        key[u] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (int t = tid; t < m; t += DP_THREADS) {
        const unsigned rr = key_flat(key[t]) / (unsigned)nc;      // (< r1 - r0: the key was made from it)
        box[t] = a.cand_boxes[((size_t)r0 + rr) * nc + cls];
        sup[t] = 0;
    }
    __syncthreads();
    // Greedy walk.  sup[i] is final when i is reached: every kept box before it marked its victims ahead of a barrier.  A kept box
    // marks the later boxes it overlaps (sc2_nms's test, the earlier box first); the first D kept are all that launch 3 can use.
    unsigned long long *out = a.keys + list * a.D;
    int kept = 0;
    for (int i = 0; i < m; ++i) {
        if (sup[i]) continue;
        if (tid == 0) out[kept] = key[i];
        if (++kept == a.D) break;
        const float4 bi = box[i];
        const float area_i = box_area(bi);
        for (int j = i + 1 + tid; j < m; j += DP_THREADS) {
            const float4 bj = box[j];
            if (box_iou(bi, area_i, bj, box_area(bj)) > a.nms_thresh) sup[j] = 1;
        }
        __syncthreads();
    }
    if (tid == 0) a.kept_count[list] = kept;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// Launch 3: one workgroup per image.  Wave 0 merges the classes' lists -- lane l holds the heads of classes l and l + 64 and
// reads its lists through a DP_HEAD-key window in LDS that only it writes and reads -- taking the greatest head D times; then
// all threads write the image's D slots, detections first and zeros behind them.
__global__ __launch_bounds__(DP_THREADS) void detpost_merge_kernel(const DetPostArgs a) {
    __shared__ unsigned long long window[SC2_DETPOST_MAX_CLASSES][DP_HEAD];
    __shared__ unsigned long long chosen[SC2_DETPOST_MAX_DET];
    __shared__ int total[DP_THREADS / 64], over[DP_THREADS / 64], found;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nc = a.C - 1, D = a.D;
    int r0, r1;
    match_range(a.off, img, a.R, r0, r1);
    {   // the image's survivors against the two caps
        int sum = 0, big = 0;
        for (int c = tid; c < nc; c += DP_THREADS) {
            const int s = a.seg_count[(size_t)img * nc + c];
            sum += s;
            big |= s > DP_SEG;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            sum += __shfl_xor(sum, d, 64);
            big |= __shfl_xor(big, d, 64);
        }
        if (lane == 0) {
            total[tid >> 6] = sum;
            over[tid >> 6] = big;
        }
        if (tid == 0) found = 0;
    }
    __syncthreads();
    int status = 0;
    {
        long long sum = 0;
        int big = 0;
        for (int w = 0; w < DP_THREADS / 64; ++w) {
            sum += total[w];
            big |= over[w];
        }
        status = (sum > SC2_DETPOST_MAX_CAND ? SC2_DETPOST_OVER_CAND : 0) | (big ? SC2_DETPOST_OVER_SEG : 0);
    }
    if (status == 0 && tid < 64) {
        unsigned long long cur[2];
        int pos[2], cnt[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            pos[h] = 0;
            cnt[h] = c < nc ? min(max(a.kept_count[(size_t)img * nc + c], 0), D) : 0;
            const unsigned long long *src = a.keys + ((size_t)img * nc + c) * D;
            for (int k = 0; k < DP_HEAD && k < cnt[h]; ++k) window[c][k] = src[k];
            cur[h] = cnt[h] > 0 ? window[c][0] : 0ull;
        }
        int d = 0;
        for (; d < D; ++d) {
            const unsigned long long mine = cur[0] > cur[1] ? cur[0] : cur[1];
            const unsigned long long best = wave_max_u64(mine);
            if (best == 0ull) break;      // (every key is above 0: every list is spent)
            if (mine == best) {           // one lane: keys are unique within an image
                chosen[d] = best;
                const int h = cur[0] == best ? 0 : 1;
                const int c = lane + 64 * h;
                const int q = ++pos[h];
                if (q >= cnt[h]) {
                    cur[h] = 0ull;
                } else {
                    if ((q & (DP_HEAD - 1)) == 0) {
                        const unsigned long long *src = a.keys + ((size_t)img * nc + c) * D + q;
                        for (int k = 0; k < DP_HEAD && q + k < cnt[h]; ++k) window[c][k] = src[k];
                    }
                    cur[h] = window[c][q & (DP_HEAD - 1)];
                }
            }
        }
        if (lane == 0) found = d;
    }
    __syncthreads();
    const int n_det = found;
    if (tid == 0) {
        a.count[img] = n_det;
        a.status[img] = status;
    }
    for (int d = tid; d < D; d += DP_THREADS) {
        float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float score = 0.0f;
        int64_t label = 0;
        if (d < n_det) {
            const unsigned flat = key_flat(chosen[d]);
            const unsigned rr = flat / (unsigned)nc, c = flat - rr * (unsigned)nc;
            if ((long long)r0 + rr < r1) {      // (always: the key was made from a row of the image)
                const size_t at = ((size_t)r0 + rr) * nc + c;
                b = a.cand_boxes[at];
                score = a.cand_scores[at];
                label = (int64_t)c + 1;
            }
        }
        const size_t o = (size_t)img * D + d;
        reinterpret_cast<float4 *>(a.boxes)[o] = b;
        a.scores[o] = score;
        a.labels[o] = label;
    }
}

inline long long round16(long long v) { return (v + 15) / 16 * 16; }

// the workspace's parts, each starting on a multiple of 16 bytes
struct DetPostLayout {
    long long boxes, keys, bitmap, scores, seg_count, kept_count, bytes;
};
inline DetPostLayout detpost_layout(long long R, long long C, long long n, long long D) {
    DetPostLayout l;
    const long long cand = R * (C - 1), lists = n * (C - 1);
    l.boxes = 0;
    l.keys = l.boxes + round16(cand * 16);
    l.bitmap = l.keys + round16(lists * D * 8);
    l.scores = l.bitmap + round16(R * 16);
    l.seg_count = l.scores + round16(cand * 4);
    l.kept_count = l.seg_count + round16(lists * 4);
    l.bytes = l.kept_count + round16(lists * 4);
    return l;
}
inline bool detpost_dims_ok(int R, int C, int n, int D) {
    return R >= 0 && n >= 0 && n <= 65535 && C >= 2 && C <= SC2_DETPOST_MAX_CLASSES && D >= 1 && D <= SC2_DETPOST_MAX_DET &&
           (long long)R * (C - 1) < (1ll << 31);
}

}  // namespace

extern "C" long long sc2_det_postprocess_ws_bytes(int R, int C, int n, int D) {
    if (!detpost_dims_ok(R, C, n, D)) return 0;
    return detpost_layout(R, C, n, D).bytes;
}

extern "C" int sc2_det_postprocess(const float *logits, const float *deltas, const float *proposals, const int32_t *offsets,
                                   const int32_t *offsets_host, const int32_t *image_sizes, int R, int C, int n, float wx, float wy,
                                   float ww, float wh, float bbox_xform_clip, float score_thresh, float min_size, float nms_thresh, int D,
                                   float *boxes, float *scores, int64_t *labels, int32_t *count, int32_t *status, float *cand_scores,
                                   float *cand_boxes, void *ws, void *stream) {
    SC2_REQUIRE(R >= 0 && n >= 0 && n <= 65535, SC2_ERR_INVALID_ARG, "det_postprocess: %d proposals, %d images (0..65535)", R, n);
    SC2_REQUIRE(C >= 2 && C <= SC2_DETPOST_MAX_CLASSES, SC2_ERR_UNSUPPORTED, "det_postprocess: %d classes (2..%d)", C,
                SC2_DETPOST_MAX_CLASSES);
    SC2_REQUIRE(D >= 1 && D <= SC2_DETPOST_MAX_DET, SC2_ERR_UNSUPPORTED, "det_postprocess: %d detections per image (1..%d)", D,
                SC2_DETPOST_MAX_DET);
    SC2_REQUIRE((long long)R * (C - 1) < (1ll << 31), SC2_ERR_UNSUPPORTED, "det_postprocess: %d x %d candidates (below 2^31)", R, C - 1);
    SC2_REQUIRE(offsets_host, SC2_ERR_INVALID_ARG, "det_postprocess: the host copy of the offsets is missing");
    SC2_REQUIRE(score_thresh == score_thresh && min_size == min_size && nms_thresh == nms_thresh && bbox_xform_clip == bbox_xform_clip,
                SC2_ERR_INVALID_ARG, "det_postprocess: a threshold is NaN");
    int longest = 0;
    SC2_REQUIRE(match_offsets_ok(offsets_host, n, R, longest), SC2_ERR_INVALID_ARG,
                "det_postprocess: offsets must start at 0, never decrease and end at %d", R);
    if (n == 0) return SC2_OK;
    SC2_REQUIRE(offsets && image_sizes && boxes && scores && labels && count && status && ws, SC2_ERR_INVALID_ARG,
                "det_postprocess: null argument");
    SC2_REQUIRE(R == 0 || (logits && deltas && proposals), SC2_ERR_INVALID_ARG, "det_postprocess: null input");
    SC2_REQUIRE((cand_scores == nullptr) == (cand_boxes == nullptr), SC2_ERR_INVALID_ARG,
                "det_postprocess: the candidate table's two parts come together or not at all");
    SC2_REQUIRE(aligned16(deltas) && aligned16(proposals) && aligned16(boxes) && aligned16(cand_boxes) && aligned16(ws) && aligned8(labels),
                SC2_ERR_INVALID_ARG, "det_postprocess: deltas, proposals, boxes, cand_boxes and the workspace must be 16-byte aligned");
    const DetPostLayout l = detpost_layout(R, C, n, D);
    char *w = static_cast<char *>(ws);
    DetPostArgs a;
    a.logits = logits;
    a.deltas = deltas;
    a.proposals = reinterpret_cast<const float4 *>(proposals);
    a.off = offsets;
    a.sizes = image_sizes;
    a.cand_scores = cand_scores ? cand_scores : reinterpret_cast<float *>(w + l.scores);
    a.cand_boxes = reinterpret_cast<float4 *>(cand_boxes ? cand_boxes : reinterpret_cast<float *>(w + l.boxes));
    a.bitmap = reinterpret_cast<unsigned long long *>(w + l.bitmap);
    a.keys = reinterpret_cast<unsigned long long *>(w + l.keys);
    a.seg_count = reinterpret_cast<int32_t *>(w + l.seg_count);
    a.kept_count = reinterpret_cast<int32_t *>(w + l.kept_count);
    a.boxes = boxes;
    a.scores = scores;
    a.labels = labels;
    a.count = count;
    a.status = status;
    a.R = R;
    a.C = C;
    a.n = n;
    a.D = D;
    a.wx = wx;
    a.wy = wy;
    a.ww = ww;
    a.wh = wh;
    a.clip = bbox_xform_clip;
    a.score_thresh = score_thresh;
    a.min_size = min_size;
    a.nms_thresh = nms_thresh;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R > 0) {
        hipLaunchKernelGGL(detpost_rows_kernel, dim3((unsigned)((R + DP_ROWS_PER_WG - 1) / DP_ROWS_PER_WG)), dim3(DP_THREADS), 0, s, a);
        SC2_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(detpost_class_kernel, dim3((unsigned)(C - 1), (unsigned)n), dim3(DP_THREADS), 0, s, a);
    SC2_CHECK_LAUNCH();
    hipLaunchKernelGGL(detpost_merge_kernel, dim3((unsigned)n), dim3(DP_THREADS), 0, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
