// The RPN's proposal selection (torchvision's `RegionProposalNetwork.filter_proposals` with the decode in front of it) for a whole
// batch in three launches: from the RPN head's raw per-level maps, read in place, to the padded per-image proposals.
// include/sc2_bottleneck.h states the contract (sc2_rpn_proposals); tests/ref_rpn_post.py restates it.
//   launch 1  a workgroup per (level, image): the k_l greatest logits of the level by a radix select over the ordered key bits
//             (four 8-bit digits, LDS histograms), the ties at the cut picked by ascending index, the selection sorted into its
//             ranks in LDS; then sigmoid, decode and clip of the selected anchors only -> the candidate table [N, L, K]
//   launch 2  a workgroup per (level, image): the level's survivors sorted by (score descending, rank ascending) in LDS, greedy
//             NMS in that order, the keys of the first P kept
//   launch 3  a workgroup per image: the levels' kept lists (each in order already) merged -- a key's place is the number of keys
//             above it, counted by binary search in every other list -- into the first P of the image, zeros behind them
// Plain kernels, as det_post.hip's: no atomics on global memory, no workgroup waits for another, every index checked against its
// array before use.  A candidate's place in every list follows from its key alone (unique within an image), so two calls give
// the same bits.
#include "sc2_common.h"

#pragma clang fp contract(off)   // BoxCoder.decode_single's `dx * widths + ctr_x` and the IoU: every step rounded once

#include "detect_common.h"

namespace {

constexpr int RP_SELECT_THREADS = 1024;
constexpr int RP_SELECT_WAVES = RP_SELECT_THREADS / 64;
constexpr int RP_NMS_THREADS = 256;
constexpr int RP_MERGE_THREADS = 1024;
constexpr int RP_K = SC2_RPNPOST_MAX_PRE_NMS;       // one level's selection, sorted and suppressed in LDS
constexpr int RP_LEVELS = SC2_RPNPOST_MAX_LEVELS;
constexpr int RP_KEYS = SC2_RPNPOST_MAX_KEYS;       // launch 3: the kept keys of an image's levels, all in LDS
constexpr int RP_RANK_BITS = 11;                    // a key's low word: (level << 11) | rank, complemented
static_assert((RP_K & (RP_K - 1)) == 0 && RP_K == (1 << RP_RANK_BITS), "the selection is sorted as a power of two; a rank takes 11 bits");
static_assert(RP_KEYS * 8 + 1024 <= 160 * 1024, "launch 3 holds the image's keys in one workgroup's LDS");

struct RpnPostArgs {
    const float *obj[RP_LEVELS], *del[RP_LEVELS];     // [N, A_l, H_l, W_l] and [N, 4 A_l, H_l, W_l], as the head writes them
    int A[RP_LEVELS], HW[RP_LEVELS], n_l[RP_LEVELS];  // n_l = A_l * HW_l
    int anchor_off[RP_LEVELS];                        // level l's first anchor
    const float4 *anchors;
    const int32_t *sizes;
    int32_t *cand_index;              // [N, L, K]    (the workspace's, or the caller's test hook): level-local index by rank, -1 behind k_l
    float *cand_scores;               // [N, L, K]
    float4 *cand_boxes;               // [N, L, K]
    int32_t *cand_k;                  // [N, L] or null
    unsigned long long *keys;         // [N, L, KP]: the first KP = min(K, P) kept of a level, in order
    int32_t *kept_count;              // [N, L]
    float *boxes, *scores;
    int32_t *count;
    int L, N, K, P, KP;
    float4 w;
    float clip, score_thresh, min_size, nms_thresh;
};

// A logit's place in torch.topk's order as an unsigned number: every NaN above every number (and all NaNs equal), -0 equal to +0
__device__ __forceinline__ unsigned logit_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    if (v == 0.0f) return 0x80000000u;
    return float_order_bits(v);
}
__device__ __forceinline__ unsigned long long pack_key(unsigned ord, unsigned low) { return ((unsigned long long)ord << 32) | (0xFFFFFFFFu - low); }
__device__ __forceinline__ unsigned key_low(unsigned long long k) { return 0xFFFFFFFFu - (unsigned)k; }
__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// One histogram vote per DISTINCT digit of a wave instead of one per lane (the logits of a level crowd into a few top digits: the
// lanes' atomics on one LDS word would go one after the other).  Called by all lanes of a wave together.
__device__ __forceinline__ void hist_add(unsigned *hist, unsigned digit, bool valid, int lane) {
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned d = (unsigned)__shfl((int)digit, leader, 64);
        const unsigned long long same = __ballot(valid && digit == d);
        if (lane == leader) atomicAdd(&hist[d & 255u], (unsigned)__popcll(same));     // (LDS)
        todo &= ~same;
    }
}

// descending bitonic sort of key[0 .. m) in LDS (m <= RP_K; the pad is 0, below every key)
template <int THREADS>
__device__ __forceinline__ void sort_keys_desc(unsigned long long *key, int m, int tid) {
    int P2 = 1;
    while (P2 < m) P2 <<= 1;
    for (int t = m + tid; t < P2; t += THREADS) key[t] = 0;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P2; t += THREADS) {
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
}

// Launch 1: workgroup (level, image).
__global__ __launch_bounds__(RP_SELECT_THREADS) void rpnpost_select_kernel(const RpnPostArgs a) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sel[RP_K];
    __shared__ unsigned wave_ties[RP_SELECT_WAVES];
    __shared__ unsigned s_prefix, s_need, s_members;
    const int lvl = blockIdx.x, img = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int A = a.A[lvl], HW = a.HW[lvl], n = a.n_l[lvl];
    const int k = min(min(a.K, n), RP_K);
    const float *obj = a.obj[lvl] + (size_t)img * n;
    if (tid == 0) s_members = 0;
    // The k-th greatest key, digit by digit from the top: `prefix` holds the digits found, `need` how many of the elements that
    // share them are still to be taken.  The histograms are read in memory order: their counts do not depend on the order.
    unsigned prefix = 0, need = (unsigned)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const unsigned above = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int base = 0; base < n; base += RP_SELECT_THREADS) {
            const int m = base + tid;
            const bool valid = m < n;
            const unsigned key = valid ? logit_key(obj[m]) : 0u;
            hist_add(hist, (key >> shift) & 255u, valid && (key & above) == prefix, lane);
        }
        __syncthreads();
        if (tid < 64) {     // lane l: bins 255 - 4 l .. 252 - 4 l, the greatest digit first
            unsigned c[4], sum = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                c[q] = hist[255 - 4 * lane - q];
                sum += c[q];
            }
            unsigned incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = (unsigned)__shfl_up((int)incl, d, 64);
                if (lane >= d) incl += v;
            }
            unsigned run = incl - sum;
            if (run < need && need <= incl) {     // one lane: the bins hold at least `need` elements
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (need <= run + c[q]) {
                        s_prefix = prefix | ((unsigned)(255 - 4 * lane - q) << shift);
                        s_need = need - run;
                        break;
                    }
                    run += c[q];
                }
            }
        }
        __syncthreads();
        prefix = s_prefix;
        need = s_need;
    }
    // `prefix` is the k-th key now; `need` of the elements equal to it are taken, those of the lowest indices.  Each wave walks a
    // contiguous stretch of the level in INDEX order t = (h W + w) A + a: everything above the cut goes into the selection at once,
    // the ties are counted, and once every wave knows how many ties lie before its stretch it picks its share of them.
    const unsigned cut = prefix, n_ties = need;
    const int seg = (n + RP_SELECT_THREADS - 1) / RP_SELECT_THREADS * 64;
    const int w_beg = min(wave * seg, n), w_end = min(w_beg + seg, n);
    unsigned ties = 0;
    for (int t0 = w_beg; t0 < w_end; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < w_end;
        unsigned key = 0;
        if (valid) {
            const unsigned p = (unsigned)t / (unsigned)A, an = (unsigned)t - p * (unsigned)A;
            key = logit_key(obj[(size_t)an * HW + p]);
        }
        const bool over = valid && key > cut;
        const unsigned long long mask = __ballot(over);
        if (mask) {
            unsigned first = 0;
            if (lane == 0) first = atomicAdd(&s_members, (unsigned)__popcll(mask));     // (LDS)
            first = (unsigned)__shfl((int)first, 0, 64);
            const unsigned slot = first + lanes_below(mask, lane);
            if (over && slot < (unsigned)RP_K) sel[slot] = pack_key(key, (unsigned)t);
        }
        ties += (unsigned)__popcll(__ballot(valid && key == cut));
    }
    if (lane == 0) wave_ties[wave] = ties;
    __syncthreads();
    const unsigned greater = s_members;      // (= k - n_ties)
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += wave_ties[w];
    for (int t0 = w_beg; t0 < w_end && before < n_ties; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < w_end;
        unsigned key = 0;
        if (valid) {
            const unsigned p = (unsigned)t / (unsigned)A, an = (unsigned)t - p * (unsigned)A;
            key = logit_key(obj[(size_t)an * HW + p]);
        }
        const bool tie = valid && key == cut;
        const unsigned long long mask = __ballot(tie);
        const unsigned pos = before + lanes_below(mask, lane);
        if (tie && pos < n_ties && greater + pos < (unsigned)RP_K) sel[greater + pos] = pack_key(cut, (unsigned)t);
        before += (unsigned)__popcll(mask);
    }
    __syncthreads();
    sort_keys_desc<RP_SELECT_THREADS>(sel, k, tid);      // (key descending, index ascending): position = rank
    // the selected anchors alone: sigmoid, decode, clip
    const float img_h = (float)a.sizes[2 * img], img_w = (float)a.sizes[2 * img + 1];
    const size_t slot0 = ((size_t)img * a.L + lvl) * a.K;
    const float *del = a.del[lvl] + (size_t)img * n * 4;
    for (int j = tid; j < a.K; j += RP_SELECT_THREADS) {
        int index = -1;
        float score = 0.0f;
        float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < k) {
            const unsigned t = key_low(sel[j]);
            if (t < (unsigned)n) {      // (always: the key was made from an index of the level)
                const unsigned p = t / (unsigned)A, an = t - p * (unsigned)A;
                const float logit = obj[(size_t)an * HW + p];
                const float *d = del + (size_t)an * 4 * HW + p;
                const float4 dl = make_float4(d[0], d[(size_t)HW], d[2 * (size_t)HW], d[3 * (size_t)HW]);
                index = (int)t;
                score = 1.0f / (1.0f + expf(-logit));
                box = decode_clip_box(a.anchors[(size_t)a.anchor_off[lvl] + t], dl, a.w, a.clip, img_w, img_h);
            }
        }
        a.cand_index[slot0 + j] = index;
        a.cand_scores[slot0 + j] = score;
        a.cand_boxes[slot0 + j] = box;
    }
    if (tid == 0 && a.cand_k) a.cand_k[(size_t)img * a.L + lvl] = k;
}

// Launch 2: workgroup (level, image).
__global__ __launch_bounds__(RP_NMS_THREADS) void rpnpost_level_kernel(const RpnPostArgs a) {
    __shared__ unsigned long long key[RP_K];
    __shared__ float4 box[RP_K];
    __shared__ uint8_t sup[RP_K];
    __shared__ int members;
    const int lvl = blockIdx.x, img = blockIdx.y, tid = threadIdx.x;
    const int k = min(min(a.K, a.n_l[lvl]), RP_K);
    const size_t list = (size_t)img * a.L + lvl, slot0 = list * a.K;
    if (tid == 0) members = 0;
    __syncthreads();
    // the level's survivors (the RPN's rule: both tests inclusive; a NaN fails), in whatever order the threads arrive
    for (int j = tid; j < k; j += RP_NMS_THREADS) {
        const float score = a.cand_scores[slot0 + j];
        const float4 b = a.cand_boxes[slot0 + j];
        if (!(score >= a.score_thresh && (b.z - b.x) >= a.min_size && (b.w - b.y) >= a.min_size)) continue;
        const int slot = atomicAdd(&members, 1);     // (LDS)
        if (slot < RP_K) key[slot] = pack_key(float_order_bits(score), ((unsigned)lvl << RP_RANK_BITS) | (unsigned)j);
    }
    __syncthreads();
    const int m = min(members, RP_K);
    if (m == 0) {
        if (tid == 0) a.kept_count[list] = 0;
        return;
    }
    sort_keys_desc<RP_NMS_THREADS>(key, m, tid);
    for (int t = tid; t < m; t += RP_NMS_THREADS) {
        const unsigned j = key_low(key[t]) & (unsigned)(RP_K - 1);      // (< k: the key was made from it)
        box[t] = a.cand_boxes[slot0 + j];
        sup[t] = 0;
    }
    __syncthreads();
    // Greedy walk, as detpost_class_kernel's: sup[i] is final when i is reached.  The first KP = min(K, P) kept are all that the
    // image's first P can hold of this level.
    unsigned long long *out = a.keys + list * a.KP;
    int kept = 0;
    for (int i = 0; i < m; ++i) {
        if (sup[i]) continue;
        if (tid == 0) out[kept] = key[i];
        if (++kept == a.KP) break;
        const float4 bi = box[i];
        const float area_i = box_area(bi);
        for (int j = i + 1 + tid; j < m; j += RP_NMS_THREADS) {
            const float4 bj = box[j];
            if (box_iou(bi, area_i, bj, box_area(bj)) > a.nms_thresh) sup[j] = 1;
        }
        __syncthreads();
    }
    if (tid == 0) a.kept_count[list] = kept;
}

// Launch 3: one workgroup per image.
__global__ __launch_bounds__(RP_MERGE_THREADS) void rpnpost_merge_kernel(const RpnPostArgs a) {
    __shared__ unsigned long long key[RP_KEYS];
    __shared__ int first[RP_LEVELS + 1];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int L = a.L, P = a.P;
    if (tid == 0) {
        int run = 0;
        for (int l = 0; l < L; ++l) {     // (a level keeps at most min(K, n_l, P): the host checked that the sum fits RP_KEYS)
            first[l] = run;
            run = min(run + min(max(a.kept_count[(size_t)img * L + l], 0), min(a.KP, a.n_l[l])), RP_KEYS);
        }
        first[L] = run;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        const unsigned long long *src = a.keys + ((size_t)img * L + l) * a.KP;
        const int b = first[l], e = first[l + 1];
        for (int q = b + tid; q < e; q += RP_MERGE_THREADS) key[q] = src[q - b];
    }
    __syncthreads();
    const int total = first[L], n_out = min(total, P);
    for (int e = tid; e < total; e += RP_MERGE_THREADS) {
        const unsigned long long mine = key[e];
        int pos = 0;
        for (int l = 0; l < L; ++l) {
            const int b = first[l], c = first[l + 1] - b;
            if (e >= b && e < b + c) {     // its own list: the keys before it
                pos += e - b;
                continue;
            }
            int lo = 0, hi = c;            // the keys of list l above `mine` (the list descends; keys are unique within an image)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key[b + mid] > mine) lo = mid + 1; else hi = mid;
            }
            pos += lo;
        }
        if (pos >= P) continue;
        const unsigned low = key_low(mine), lvl = low >> RP_RANK_BITS, rank = low & (unsigned)(RP_K - 1);
        float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float score = 0.0f;
        if (lvl < (unsigned)L && rank < (unsigned)a.K) {      // (always: the key was made from them)
            const size_t at = ((size_t)img * L + lvl) * a.K + rank;
            b = a.cand_boxes[at];
            score = a.cand_scores[at];
        }
        const size_t o = (size_t)img * P + pos;
        reinterpret_cast<float4 *>(a.boxes)[o] = b;
        a.scores[o] = score;
    }
    for (int d = n_out + tid; d < P; d += RP_MERGE_THREADS) {
        const size_t o = (size_t)img * P + d;
        reinterpret_cast<float4 *>(a.boxes)[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        a.scores[o] = 0.0f;
    }
    if (tid == 0) a.count[img] = n_out;
}

inline long long round16(long long v) { return (v + 15) / 16 * 16; }

// the workspace's parts, each starting on a multiple of 16 bytes
struct RpnPostLayout {
    long long boxes, keys, scores, index, kept_count, bytes;
};
inline RpnPostLayout rpnpost_layout(long long N, long long L, long long K, long long P) {
    RpnPostLayout l;
    const long long cand = N * L * K, KP = K < P ? K : P;
    l.boxes = 0;
    l.keys = l.boxes + round16(cand * 16);
    l.scores = l.keys + round16(N * L * KP * 8);
    l.index = l.scores + round16(cand * 4);
    l.kept_count = l.index + round16(cand * 4);
    l.bytes = l.kept_count + round16(N * L * 4);
    return l;
}
inline bool rpnpost_dims_ok(int N, int L, int K, int P) {
    return N >= 0 && N <= 65535 && L >= 1 && L <= SC2_RPNPOST_MAX_LEVELS && K >= 1 && K <= SC2_RPNPOST_MAX_PRE_NMS && P >= 1 &&
           P <= SC2_RPNPOST_MAX_POST_NMS;
}

}  // namespace

extern "C" long long sc2_rpn_proposals_ws_bytes(int N, int L, int K, int P) {
    if (!rpnpost_dims_ok(N, L, K, P)) return 0;
    return rpnpost_layout(N, L, K, P).bytes;
}

extern "C" int sc2_rpn_proposals(const float *const *objectness, const float *const *deltas, const int32_t *num_anchors,
                                 const int32_t *heights, const int32_t *widths, int L, const float *anchors, const int32_t *image_sizes,
                                 int N, int K, int P, float nms_thresh, float score_thresh, float min_size, float wx, float wy, float ww,
                                 float wh, float bbox_xform_clip, float *boxes, float *scores, int32_t *count, int32_t *cand_index,
                                 float *cand_scores, float *cand_boxes, int32_t *cand_k, void *ws, void *stream) {
    SC2_REQUIRE(N >= 0 && N <= 65535, SC2_ERR_INVALID_ARG, "rpn_proposals: %d images (0..65535)", N);
    SC2_REQUIRE(L >= 1 && L <= SC2_RPNPOST_MAX_LEVELS, SC2_ERR_UNSUPPORTED, "rpn_proposals: %d levels (1..%d)", L, SC2_RPNPOST_MAX_LEVELS);
    SC2_REQUIRE(K >= 1 && K <= SC2_RPNPOST_MAX_PRE_NMS, SC2_ERR_UNSUPPORTED, "rpn_proposals: pre-NMS top-n %d per level (1..%d)", K,
                SC2_RPNPOST_MAX_PRE_NMS);
    SC2_REQUIRE(P >= 1 && P <= SC2_RPNPOST_MAX_POST_NMS, SC2_ERR_UNSUPPORTED, "rpn_proposals: post-NMS top-n %d (1..%d)", P,
                SC2_RPNPOST_MAX_POST_NMS);
    SC2_REQUIRE(objectness && deltas && num_anchors && heights && widths, SC2_ERR_INVALID_ARG, "rpn_proposals: the level tables are missing");
    SC2_REQUIRE(score_thresh == score_thresh && min_size == min_size && nms_thresh == nms_thresh && bbox_xform_clip == bbox_xform_clip,
                SC2_ERR_INVALID_ARG, "rpn_proposals: a threshold is NaN");
    RpnPostArgs a;
    long long total = 0, budget = 0;
    for (int l = 0; l < L; ++l) {
        SC2_REQUIRE(num_anchors[l] >= 1 && heights[l] >= 1 && widths[l] >= 1, SC2_ERR_INVALID_ARG,
                    "rpn_proposals: level %d is %d x %d x %d (all at least 1)", l, num_anchors[l], heights[l], widths[l]);
        const long long hw = (long long)heights[l] * widths[l], n = hw * num_anchors[l];
        SC2_REQUIRE(total + n < SC2_RPNPOST_MAX_ANCHORS, SC2_ERR_UNSUPPORTED, "rpn_proposals: the anchors of an image (below 2^31 / 4)");
        a.A[l] = num_anchors[l];
        a.HW[l] = (int)hw;
        a.n_l[l] = (int)n;
        a.anchor_off[l] = (int)total;
        total += n;
        budget += n < K ? n : K;
    }
    SC2_REQUIRE(budget <= SC2_RPNPOST_MAX_KEYS, SC2_ERR_UNSUPPORTED,
                "rpn_proposals: the levels select %lld anchors of an image together (at most %d)", budget, SC2_RPNPOST_MAX_KEYS);
    if (N == 0) return SC2_OK;
    SC2_REQUIRE(anchors && image_sizes && boxes && scores && count && ws, SC2_ERR_INVALID_ARG, "rpn_proposals: null argument");
    SC2_REQUIRE((cand_index == nullptr) == (cand_scores == nullptr) && (cand_index == nullptr) == (cand_boxes == nullptr) &&
                    (cand_index == nullptr) == (cand_k == nullptr),
                SC2_ERR_INVALID_ARG, "rpn_proposals: the candidate table's four parts come together or not at all");
    bool maps_ok = true;
    for (int l = 0; l < L; ++l) maps_ok = maps_ok && objectness[l] && deltas[l] && aligned16(objectness[l]) && aligned16(deltas[l]);
    SC2_REQUIRE(maps_ok && aligned16(anchors) && aligned16(image_sizes) && aligned16(boxes) && aligned16(scores) && aligned16(count) &&
                    aligned16(cand_index) && aligned16(cand_scores) && aligned16(cand_boxes) && aligned16(cand_k) && aligned16(ws),
                SC2_ERR_INVALID_ARG, "rpn_proposals: every pointer must be non-null and 16-byte aligned");
    const RpnPostLayout lay = rpnpost_layout(N, L, K, P);
    char *w = static_cast<char *>(ws);
    for (int l = 0; l < RP_LEVELS; ++l) {
        a.obj[l] = l < L ? objectness[l] : nullptr;
        a.del[l] = l < L ? deltas[l] : nullptr;
        if (l >= L) a.A[l] = a.HW[l] = a.n_l[l] = a.anchor_off[l] = 0;
    }
    a.anchors = reinterpret_cast<const float4 *>(anchors);
    a.sizes = image_sizes;
    a.cand_index = cand_index ? cand_index : reinterpret_cast<int32_t *>(w + lay.index);
    a.cand_scores = cand_scores ? cand_scores : reinterpret_cast<float *>(w + lay.scores);
    a.cand_boxes = reinterpret_cast<float4 *>(cand_boxes ? cand_boxes : reinterpret_cast<float *>(w + lay.boxes));
    a.cand_k = cand_k;
    a.keys = reinterpret_cast<unsigned long long *>(w + lay.keys);
    a.kept_count = reinterpret_cast<int32_t *>(w + lay.kept_count);
    a.boxes = boxes;
    a.scores = scores;
    a.count = count;
    a.L = L;
    a.N = N;
    a.K = K;
    a.P = P;
    a.KP = K < P ? K : P;
    a.w = make_float4(wx, wy, ww, wh);
    a.clip = bbox_xform_clip;
    a.score_thresh = score_thresh;
    a.min_size = min_size;
    a.nms_thresh = nms_thresh;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(rpnpost_select_kernel, dim3((unsigned)L, (unsigned)N), dim3(RP_SELECT_THREADS), 0, s, a);
    SC2_CHECK_LAUNCH();
    hipLaunchKernelGGL(rpnpost_level_kernel, dim3((unsigned)L, (unsigned)N), dim3(RP_NMS_THREADS), 0, s, a);
    SC2_CHECK_LAUNCH();
    hipLaunchKernelGGL(rpnpost_merge_kernel, dim3((unsigned)N), dim3(RP_MERGE_THREADS), 0, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
