// The ImageNet input chains of a batch, from the source bytes to the classifier's float32 batch (configs/ilsvrc2012/** of the reference:
// RandomResizedCrop -> RandomHorizontalFlip -> ToTensor -> Normalize in training, Resize -> CenterCrop -> ToTensor -> Normalize in
// evaluation): Pillow's bilinear resample of a stored box of the source, the flip, the OH x OW window, `(p / 255 - mean) / std`.
//   cls_input_kernel   per (sample, 16 output rows, 64 output columns), ONE launch: the tile's 64 column and 16 row entries (Pillow's bounds
//                      and 22-bit coefficients, float64, every operation rounded once) computed by 80 lanes into LDS -- a tile needs
//                      80 of its sample's OH + OW entries, so the tables of seg_augment.hip's first launch fit the prologue -- then the
//                      horizontally resampled source rows of the band as 8-bit pixels in LDS, the vertical pass from there, the division.
// Only the output window is computed; neither the resized image nor the intermediate of Pillow's two passes exists in memory.
// include/sc2_bottleneck.h states the contract; tests/ref_cls_input.py restates it.
// Plain kernel: every index checked against the stored box before use, no atomics, no workgroup waits for another.
// Shared through input_common.h with seg_augment.hip: pil_coeffs, the two passes of a pixel (pil_hpass, pil_vpass) and the tile; with
// det_input.hip as well: the pixel load and the entry's checks (InputNorm).  Its own: the identity entry of an axis of equal lengths.
#include "input_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CI_DESC = SC2_CLS_INPUT_DESC_INTS;         // int32 words of a descriptor row
constexpr int CI_ENTRY = 2 + PIL_TAPS;                   // int32 words of a table entry: first, count, 9 coefficients
constexpr int CI_MAX_SIDE = SC2_SEG_AUGMENT_MAX_SIDE;

struct Desc {
    int off, h, w, fh, fw, row0, col0, nh, nw, flip, top, left;
};

__device__ __forceinline__ Desc ci_desc(const int32_t *table, int i) {
    const int32_t *d = table + (size_t)i * CI_DESC;
    Desc s;
    s.off = d[0]; s.h = d[1]; s.w = d[2]; s.fh = d[3]; s.fw = d[4]; s.row0 = d[5]; s.col0 = d[6]; s.nh = d[7]; s.nw = d[8];
    s.flip = d[9]; s.top = d[10]; s.left = d[11];
    return s;
}

__device__ __forceinline__ bool ci_side(int v) { return v >= 1 && v <= CI_MAX_SIDE; }

// What the descriptor row alone decides.  0: go on to the taps; SC2_CLS_INPUT_BAD: a field no launch may follow (the wrapper refuses
// those before the launch; the kernel makes sure on its own that no such row moves an address); SC2_CLS_INPUT_RATIO: an axis shrinks
// by more than 4.  Every comparison is on values already known to lie in 0 .. CI_MAX_SIDE or done in 64 bits: nothing overflows.
__device__ __forceinline__ int ci_fields(const Desc &s, long long nbytes, int OH, int OW) {
    if (!(ci_side(s.h) && ci_side(s.w) && ci_side(s.fh) && ci_side(s.fw) && ci_side(s.nh) && ci_side(s.nw))) return SC2_CLS_INPUT_BAD;
    const bool box = s.row0 >= 0 && s.col0 >= 0 && s.row0 <= CI_MAX_SIDE && s.col0 <= CI_MAX_SIDE && s.row0 + s.h <= s.fh && s.col0 + s.w <= s.fw;
    const bool window = s.top >= 0 && s.left >= 0 && s.top <= CI_MAX_SIDE && s.left <= CI_MAX_SIDE && s.top + OH <= s.nh && s.left + OW <= s.nw;
    const bool bytes = s.off >= 0 && (long long)s.off + 3LL * s.h * s.w <= nbytes;
    if (!(box && window && bytes && (s.flip == 0 || s.flip == 1))) return SC2_CLS_INPUT_BAD;
    if (s.fh > 4 * s.nh || s.fw > 4 * s.nw) return SC2_CLS_INPUT_RATIO;
    return 0;
}

// The entry of resized index xx of an axis n_in -> n_out.  An axis of equal lengths is the identity pass -- the one coefficient 2^22,
// which gives Pillow's skipped pass byte for byte and reads no neighbour.
__device__ __forceinline__ void ci_entry(int n_in, int n_out, int xx, int32_t *e) {
    if (n_in != n_out) {
        pil_coeffs(n_in, n_out, xx, e);
        return;
    }
    e[0] = xx;
    e[1] = 1;
    e[2] = 1 << PIL_BITS;
#pragma unroll
    for (int t = 1; t < PIL_TAPS; ++t) e[2 + t] = 0;
}

struct Args {
    const uint8_t *buf;
    const int32_t *desc;
    float *images;
    int32_t *status;
    long long nbytes;
    InputNorm norm;
    int OH, OW;
};

__global__ __launch_bounds__(PIL_THREADS) void cls_input_kernel(const Args a) {
    __shared__ uint32_t hbuf[PIL_ROWS * PIL_TW];          // [source row][tile column]: the horizontal pass's 8-bit output, R | G << 8 | B << 16
    __shared__ int32_t ctab[PIL_TW * CI_ENTRY];           // the tile's column entries, in full-image coordinates
    __shared__ int32_t rtab[PIL_TH * CI_ENTRY];           // ... and its row entries
    __shared__ int32_t span[4];                           // the WINDOW's first and last source column and row (last: one past)
    const int i = blockIdx.z;
    const Desc s = ci_desc(a.desc, i);
    const bool reports = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0;
    const int fields = ci_fields(s, a.nbytes, a.OH, a.OW);
    if (fields != 0) {                                    // (uniform: the whole workgroup leaves, before any barrier)
        if (reports) a.status[i] = fields;
        return;
    }
    const int y0 = blockIdx.y * PIL_TH, x0 = blockIdx.x * PIL_TW;
    const int yv = min(y0 + PIL_TH, a.OH), xv = min(x0 + PIL_TW, a.OW);      // the tile's rows [y0, yv) and columns [x0, xv)
    const int tid = threadIdx.x;
    if (tid < PIL_TW) {
        int32_t e[CI_ENTRY];
        if (x0 + tid < xv) {
            const int c = s.left + x0 + tid;              // position in the flipped, resized image
            ci_entry(s.fw, s.nw, s.flip ? s.nw - 1 - c : c, e);
        } else {
#pragma unroll
            for (int k = 0; k < CI_ENTRY; ++k) e[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < CI_ENTRY; ++k) ctab[tid * CI_ENTRY + k] = e[k];
    } else if (tid < PIL_TW + PIL_TH) {
        const int r = tid - PIL_TW;
        int32_t e[CI_ENTRY];
        if (y0 + r < yv) {
            ci_entry(s.fh, s.nh, s.top + y0 + r, e);
        } else {
#pragma unroll
            for (int k = 0; k < CI_ENTRY; ++k) e[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < CI_ENTRY; ++k) rtab[r * CI_ENTRY + k] = e[k];
    } else if (tid < PIL_TW + PIL_TH + 4) {
        // The bounds do not decrease with the resized index, so the window's taps lie between `first` of its lowest index and
        // `first + count` of its highest: every workgroup of the sample reaches the same verdict from these four entries.
        const int q = tid - PIL_TW - PIL_TH;              // 0: first column, 1: past the last column, 2: first row, 3: past the last row
        const int lo = q < 2 ? (s.flip ? s.nw - s.left - a.OW : s.left) : s.top;
        const int hi = lo + (q < 2 ? a.OW : a.OH) - 1;
        int32_t e[CI_ENTRY];
        ci_entry(q < 2 ? s.fw : s.fh, q < 2 ? s.nw : s.nh, (q & 1) ? hi : lo, e);
        span[q] = (q & 1) ? e[0] + e[1] : e[0];
    }
    __syncthreads();
    const bool taps = span[0] >= s.col0 && span[1] <= s.col0 + s.w && span[2] >= s.row0 && span[3] <= s.row0 + s.h;
    if (reports) a.status[i] = taps ? 0 : SC2_CLS_INPUT_TAP;
    if (!taps) return;                                    // (uniform)
    const int lx = tid & (PIL_TW - 1), ly = tid / PIL_TW; // a wave owns a row, its lanes the columns
    const int x = x0 + lx;
    // the band's source rows run from its first row's bounds to its last row's (full-image coordinates)
    const int r_first = rtab[0];
    const int32_t *el = rtab + (yv - 1 - y0) * CI_ENTRY;
    const int r_count = min(el[0] + el[1] - r_first, PIL_ROWS);
    if (x < xv) {
        const int32_t *e = ctab + lx * CI_ENTRY;
        const int first = e[0] - s.col0, count = e[1];    // stored-box coordinates from here on
        int k[PIL_TAPS];
#pragma unroll
        for (int t = 0; t < PIL_TAPS; ++t) k[t] = e[2 + t];
        const uint8_t *img = a.buf + s.off;
        const size_t img_bytes = (size_t)s.h * s.w * 3;
        for (int r = ly; r < r_count; r += PIL_THREADS / PIL_TW) {
            const int sr = min(max(r_first + r - s.row0, 0), s.h - 1);
            hbuf[r * PIL_TW + lx] = pil_hpass(img, img_bytes, s.w, sr, first, count, k);
        }
    }
    __syncthreads();
    if (x >= xv) return;
    const size_t plane = (size_t)a.OH * a.OW;
    float *out = a.images + (size_t)i * 3 * plane;
    for (int y = y0 + ly; y < yv; y += PIL_THREADS / PIL_TW) {
        const int32_t *e = rtab + (y - y0) * CI_ENTRY;
        float v0, v1, v2;
        pil_vpass<PIL_ROWS, PIL_TW>(hbuf, lx, e, e[0] - r_first, a.norm.mean, a.norm.std, v0, v1, v2);
        const size_t o = (size_t)y * a.OW + x;
        out[o] = v0;
        out[plane + o] = v1;
        out[2 * plane + o] = v2;
    }
}

bool ci_sizes_ok(int n, int oh, int ow) {
    return n >= 1 && n <= SC2_CLS_INPUT_MAX_BATCH && oh >= 1 && ow >= 1 && oh <= CI_MAX_SIDE && ow <= CI_MAX_SIDE;
}

}  // namespace

extern "C" long long sc2_cls_input_workspace(int n, int oh, int ow) {
    return ci_sizes_ok(n, oh, ow) ? 0 : -1;      // the tables live in LDS: no workspace for any batch the entry takes
}

extern "C" int sc2_cls_input(const uint8_t *buf, long long nbytes, const int32_t *desc, int n, int oh, int ow, const float *mean,
                             const float *std, float *images, int32_t *status, void *stream) {
    SC2_REQUIRE(ci_sizes_ok(n, oh, ow), SC2_ERR_UNSUPPORTED, "cls_input: %d samples of %dx%d (1..%d samples, sides 1..%d)", n, oh, ow,
                SC2_CLS_INPUT_MAX_BATCH, CI_MAX_SIDE);
    const uintptr_t words = reinterpret_cast<uintptr_t>(desc) | reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(status);
    Args a;
    const int rc = a.norm.take("cls_input", nbytes, buf && desc && mean && std && images && status, (words & 3u) == 0, mean, std);
    if (rc != SC2_OK) return rc;
    a.buf = buf; a.desc = desc; a.images = images; a.status = status; a.nbytes = nbytes;
    a.OH = oh; a.OW = ow;
    const dim3 grid((unsigned)((ow + PIL_TW - 1) / PIL_TW), (unsigned)((oh + PIL_TH - 1) / PIL_TH), (unsigned)n);
    hipLaunchKernelGGL(cls_input_kernel, grid, dim3(PIL_THREADS), 0, static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
