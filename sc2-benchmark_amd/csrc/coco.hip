// COCO box AP: detection-to-ground-truth matching of every (image, category) segment in one launch (sc2_coco_match) and the
// precision / recall curves of every (category, area range, maxDet) in one launch (sc2_coco_accumulate).  The reference's evaluator
// moves every output to the host and runs pycocotools' Python loops there; here detections stay on the device.
// include/sc2_bottleneck.h states the protocol; tests/ref_coco.py restates it as a sequential float64 loop, and both kernels
// reproduce it bit for bit: f64 arithmetic without contraction, IEEE division, integer counts.
// Plain kernels: every index checked against its array before use, no global atomics, no workgroup waits for another.
#include "sc2_common.h"

#pragma clang fp contract(off)   // `dw*dh + gw*gh - i`: every step rounded once

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_DT = SC2_COCO_TILE_DETS, CM_GT = SC2_COCO_TILE_GTS;
constexpr int CM_LANES = SC2_COCO_AREAS * SC2_COCO_THRS;     // 40 walks: lane = area range * 10 + threshold

struct CocoMatchArgs {
    const double *dets, *gts, *gt_area, *iou_thrs, *area_rng;
    const uint8_t *gt_crowd;
    const int32_t *det_off, *gt_off;
    int32_t *flags, *npig;
    uint8_t *ws;
    int n_det, n_gt;
};

// Python's min(a, b) / max(a, b): the first argument unless the second is strictly smaller / larger
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

__device__ __forceinline__ double coco_iou(const double *d, const double *g, bool crowd) {
    const double w = py_min(d[0] + d[2], g[0] + g[2]) - py_max(d[0], g[0]);
    const double h = py_min(d[1] + d[3], g[1] + g[3]) - py_max(d[1], g[1]);
    if (w <= 0.0 || h <= 0.0) return 0.0;
    const double i = w * h;
    const double u = crowd ? d[2] * d[3] : d[2] * d[3] + g[2] * g[3] - i;
    return i / u;
}

// One workgroup per segment.  Phase 1 (all lanes): the IoU of the first CM_DT x CM_GT pairs into LDS.  Phase 2 (forty lanes of wave
// 0): the greedy walk of one (area range, threshold) per lane over the detections in order.  A lane's matched marks are bytes only that
// lane reads and writes (mark[g * 40 + lane]): LDS up to CM_GT ground truths, the caller's workspace beyond.
__global__ __launch_bounds__(CM_THREADS) void coco_match_kernel(const CocoMatchArgs a) {
    __shared__ double tile[CM_DT * CM_GT];
    __shared__ uint8_t mark_lds[CM_GT * CM_LANES];
    const int seg = blockIdx.x, tid = threadIdx.x;
    int d0 = a.det_off[seg], D = a.det_off[seg + 1] - d0;
    int g0 = a.gt_off[seg], G = a.gt_off[seg + 1] - g0;
    if (d0 < 0 || D < 0 || (long long)d0 + D > a.n_det) D = 0, d0 = 0;      // offsets that leave the arrays: an empty segment
    if (g0 < 0 || G < 0 || (long long)g0 + G > a.n_gt) G = 0, g0 = 0;
    const double *gts = a.gts + (size_t)g0 * 4, *dets = a.dets + (size_t)d0 * 4;
    const double *gt_area = a.gt_area + g0;
    const uint8_t *gt_crowd = a.gt_crowd + g0;
    if (tid < SC2_COCO_AREAS) {
        const double lo = a.area_rng[2 * tid], hi = a.area_rng[2 * tid + 1];
        int n = 0;
        for (int g = 0; g < G; ++g) n += !(gt_crowd[g] || gt_area[g] < lo || gt_area[g] > hi);
        a.npig[(size_t)seg * SC2_COCO_AREAS + tid] = n;
    }
    if (D == 0) return;      // (the whole workgroup: no barrier is skipped by a part of it)
    const int Dt = D < CM_DT ? D : CM_DT, Gt = G < CM_GT ? G : CM_GT;
    for (int i = tid; i < Dt * Gt; i += CM_THREADS) {
        const int d = i / Gt, g = i - d * Gt;
        tile[d * CM_GT + g] = coco_iou(dets + 4 * d, gts + 4 * g, gt_crowd[g] != 0);
    }
    __syncthreads();
    if (tid >= 64) return;
    const int lane = tid;
    const bool act = lane < CM_LANES;
    const int ar = act ? lane / SC2_COCO_THRS : 0, t = act ? lane % SC2_COCO_THRS : 0;
    const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
    const double thr = py_min(a.iou_thrs[t], 1.0 - 1e-10);
    uint8_t *mark = G <= CM_GT ? mark_lds : a.ws + (size_t)g0 * CM_LANES;
    if (act)
        for (int g = 0; g < G; ++g) mark[g * CM_LANES + lane] = 0;
    for (int d = 0; d < D; ++d) {
        const double *db = dets + 4 * d;
        int m = -1, m_ig = 0;
        if (act) {
            double best = thr;
            for (int pass = 0; pass < 2; ++pass) {      // the non-ignored ground truths, then the ignored ones, each in given order
                if (pass == 1 && m >= 0) break;         // a non-ignored match is not given up for an ignored ground truth
                for (int g = 0; g < G; ++g) {
                    const bool crowd = gt_crowd[g] != 0;
                    const double ga = gt_area[g];
                    const int ig = (crowd || ga < lo || ga > hi) ? 1 : 0;
                    if (ig != pass) continue;
                    if (mark[g * CM_LANES + lane] && !crowd) continue;
                    const double iou = (d < CM_DT && g < CM_GT) ? tile[d * CM_GT + g] : coco_iou(db, gts + 4 * g, crowd);
                    if (iou < best) continue;
                    best = iou;
                    m = g;
                    m_ig = ig;
                }
            }
            if (m >= 0) mark[m * CM_LANES + lane] = 1;
        }
        const double da = db[2] * db[3];
        const bool matched = act && m >= 0;
        const bool ign = act && (m >= 0 ? m_ig != 0 : (da < lo || da > hi));
        const unsigned long long bm = __ballot(matched), bi = __ballot(ign);
        if (lane < SC2_COCO_AREAS) {
            const unsigned mm = (unsigned)(bm >> (SC2_COCO_THRS * lane)) & 1023u, ii = (unsigned)(bi >> (SC2_COCO_THRS * lane)) & 1023u;
            a.flags[((size_t)d0 + d) * SC2_COCO_AREAS + lane] = (int32_t)(mm | (ii << SC2_COCO_THRS));
        }
    }
}

constexpr int CA_THREADS = 256, CA_ITEMS = SC2_COCO_SCAN_CHUNK / CA_THREADS, CA_WAVES = CA_THREADS / 64;
constexpr int CA_BINS = SC2_COCO_RECS + 1;
static_assert(CA_ITEMS * CA_THREADS == SC2_COCO_SCAN_CHUNK, "scan chunk");

struct CocoAccArgs {
    const int32_t *order, *cat_off, *flags, *rank, *npig, *max_dets;
    const double *rec_thrs;
    double *precision, *recall;
    int K, n_order, n_det;
};

// One workgroup per (category, area range, maxDet).  Per threshold: the packed (tp << 32 | fp) counts of the category's detections are
// scanned chunk by chunk (wave shuffles, wave totals through LDS, a carried total); every true positive takes pr to the bin counting
// the recall thresholds its rc reaches; precision[r] = the maximum over the bins above r.
__global__ __launch_bounds__(CA_THREADS) void coco_accumulate_kernel(const CocoAccArgs a) {
    __shared__ unsigned long long binmax[CA_BINS];
    __shared__ unsigned long long wave_tot[CA_WAVES];
    __shared__ double rec[SC2_COCO_RECS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int k = b / (SC2_COCO_AREAS * SC2_COCO_MAXDETS), ar = (b / SC2_COCO_MAXDETS) % SC2_COCO_AREAS, md = b % SC2_COCO_MAXDETS;
    const size_t kam = ((size_t)k * SC2_COCO_AREAS + ar) * SC2_COCO_MAXDETS + md, tstride = (size_t)a.K * SC2_COCO_AREAS * SC2_COCO_MAXDETS;
    const int np = a.npig[k * SC2_COCO_AREAS + ar];
    if (np <= 0) {      // no ground truth to find: -1 everywhere
        for (int i = tid; i < SC2_COCO_THRS * SC2_COCO_RECS; i += CA_THREADS) a.precision[(size_t)i * tstride + kam] = -1.0;
        if (tid < SC2_COCO_THRS) a.recall[(size_t)tid * tstride + kam] = -1.0;
        return;
    }
    const int n0 = a.cat_off[k];
    int n = a.cat_off[k + 1] - n0;
    if (n0 < 0 || n < 0 || (long long)n0 + n > a.n_order) n = 0;
    const int max_det = a.max_dets[md];
    if (tid < SC2_COCO_RECS) rec[tid] = a.rec_thrs[tid];
    const double dnp = (double)np;
    for (int t = 0; t < SC2_COCO_THRS; ++t) {
        if (tid < CA_BINS) binmax[tid] = 0ull;
        __syncthreads();
        unsigned long long carry = 0ull;
        for (int base = 0; base < n; base += SC2_COCO_SCAN_CHUNK) {
            unsigned long long v[CA_ITEMS], s = 0ull;
#pragma unroll
            for (int j = 0; j < CA_ITEMS; ++j) {
                const int i = base + tid * CA_ITEMS + j;
                v[j] = 0ull;
                if (i < n) {
                    const unsigned o = (unsigned)a.order[n0 + i];
                    if (o < (unsigned)a.n_det && a.rank[o] < max_det) {
                        const unsigned f = (unsigned)a.flags[(size_t)o * SC2_COCO_AREAS + ar];
                        if (!((f >> (SC2_COCO_THRS + t)) & 1u)) v[j] = ((f >> t) & 1u) ? (1ull << 32) : 1ull;
                    }
                }
                s += v[j];
            }
            unsigned long long incl = s;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            if (lane == 63) wave_tot[wave] = incl;
            __syncthreads();
            unsigned long long before = carry, total = 0ull;
#pragma unroll
            for (int w = 0; w < CA_WAVES; ++w) {
                const unsigned long long wt = wave_tot[w];
                if (w < wave) before += wt;
                total += wt;
            }
            unsigned long long run = before + (incl - s);
#pragma unroll
            for (int j = 0; j < CA_ITEMS; ++j) {
                run += v[j];
                if (v[j] >> 32) {      // a true positive: the only entries that can raise a bin's maximum
                    const double tp = (double)(unsigned)(run >> 32), fp = (double)(unsigned)(run & 0xFFFFFFFFull);
                    const double rc = tp / dnp;
                    const double pr = tp / (fp + tp + 0x1p-52);
                    int lo = 0, hi = SC2_COCO_RECS;      // the number of thresholds with rec[r] <= rc
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (rec[mid] <= rc) lo = mid + 1;
                        else hi = mid;
                    }
                    atomicMax(&binmax[lo], (unsigned long long)__double_as_longlong(pr));
                }
            }
            carry += total;
            __syncthreads();      // wave_tot is rewritten by the next chunk; binmax is read below
        }
        if (tid < SC2_COCO_RECS) {
            unsigned long long q = 0ull;
            for (int c = tid + 1; c < CA_BINS; ++c) q = binmax[c] > q ? binmax[c] : q;
            a.precision[((size_t)t * SC2_COCO_RECS + tid) * tstride + kam] = __longlong_as_double((long long)q);
        }
        if (tid == 0) a.recall[(size_t)t * tstride + kam] = (double)(unsigned)(carry >> 32) / dnp;
        __syncthreads();      // binmax is cleared by the next threshold
    }
}

bool aligned_to(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

extern "C" long long sc2_coco_match_ws_bytes(long long n_gt) { return n_gt > 0 ? (n_gt * CM_LANES + 15) / 16 * 16 : 0; }

extern "C" int sc2_coco_match(const double *dets, const double *gts, const double *gt_area, const uint8_t *gt_crowd, const int32_t *det_off,
                              const int32_t *gt_off, int n_seg, int n_det, int n_gt, const double *iou_thrs, const double *area_rng,
                              int32_t *flags, int32_t *npig, void *ws, void *stream) {
    SC2_REQUIRE(n_seg >= 0 && n_det >= 0 && n_gt >= 0, SC2_ERR_INVALID_ARG, "coco_match: negative count (n_seg=%d n_det=%d n_gt=%d)", n_seg,
                n_det, n_gt);
    if (n_seg == 0) return SC2_OK;
    SC2_REQUIRE(det_off && gt_off && iou_thrs && area_rng && npig, SC2_ERR_INVALID_ARG, "coco_match: null offsets, tables or npig");
    SC2_REQUIRE(n_det == 0 || (dets && flags), SC2_ERR_INVALID_ARG, "coco_match: null detections or flags");
    SC2_REQUIRE(n_gt == 0 || (gts && gt_area && gt_crowd && ws), SC2_ERR_INVALID_ARG, "coco_match: null ground truth or workspace");
    SC2_REQUIRE(aligned_to(dets, 8) && aligned_to(gts, 8) && aligned_to(gt_area, 8) && aligned_to(iou_thrs, 8) && aligned_to(area_rng, 8) &&
                    aligned_to(det_off, 4) && aligned_to(gt_off, 4) && aligned_to(flags, 4) && aligned_to(npig, 4),
                SC2_ERR_INVALID_ARG, "coco_match: misaligned pointer");
    CocoMatchArgs a;
    a.dets = dets; a.gts = gts; a.gt_area = gt_area; a.iou_thrs = iou_thrs; a.area_rng = area_rng;
    a.gt_crowd = gt_crowd; a.det_off = det_off; a.gt_off = gt_off; a.flags = flags; a.npig = npig;
    a.ws = static_cast<uint8_t *>(ws);
    a.n_det = n_det; a.n_gt = n_gt;
    hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)n_seg), dim3(CM_THREADS), 0, static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_coco_accumulate(const int32_t *order, const int32_t *cat_off, const int32_t *flags, const int32_t *rank, const int32_t *npig,
                                   const double *rec_thrs, const int32_t *max_dets, int K, int n_order, int n_det, double *precision,
                                   double *recall, void *stream) {
    SC2_REQUIRE(K >= 0 && n_det >= 0 && n_order >= 0, SC2_ERR_INVALID_ARG, "coco_accumulate: negative count (K=%d n_order=%d n_det=%d)", K,
                n_order, n_det);
    if (K == 0) return SC2_OK;
    SC2_REQUIRE(K <= 0x7FFFFFFF / (SC2_COCO_AREAS * SC2_COCO_MAXDETS), SC2_ERR_UNSUPPORTED, "coco_accumulate: %d categories", K);
    SC2_REQUIRE(cat_off && npig && rec_thrs && max_dets && precision && recall, SC2_ERR_INVALID_ARG, "coco_accumulate: null pointer");
    SC2_REQUIRE(n_order == 0 || (order && flags && rank), SC2_ERR_INVALID_ARG, "coco_accumulate: null detections");
    SC2_REQUIRE(aligned_to(order, 4) && aligned_to(cat_off, 4) && aligned_to(flags, 4) && aligned_to(rank, 4) && aligned_to(npig, 4) &&
                    aligned_to(max_dets, 4) && aligned_to(rec_thrs, 8) && aligned_to(precision, 8) && aligned_to(recall, 8),
                SC2_ERR_INVALID_ARG, "coco_accumulate: misaligned pointer");
    CocoAccArgs a;
    a.order = order; a.cat_off = cat_off; a.flags = flags; a.rank = rank; a.npig = npig; a.max_dets = max_dets;
    a.rec_thrs = rec_thrs; a.precision = precision; a.recall = recall;
    a.K = K; a.n_order = n_order; a.n_det = n_det;
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(K * SC2_COCO_AREAS * SC2_COCO_MAXDETS)), dim3(CA_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
