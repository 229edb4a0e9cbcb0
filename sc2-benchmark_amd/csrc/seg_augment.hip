// The PASCAL VOC augmentation chain of a batch, from the source bytes to the finished training tensors (script/task/custom/transform.py
// of the reference: CustomRandomResize -> [flip] -> [pad + crop] -> ToTensor -> Normalize, then the collator's padded batch):
//   seg_augment_tables_kernel   per sample, the window's rows and columns: Pillow's bilinear bounds and 22-bit fixed-point coefficients
//                               (float64, every operation rounded once) and the nearest resize's source indices (a running float64 sum)
//   seg_augment_tile_kernel     per (sample, 16 output rows, 64 output columns): the horizontally resampled source rows the band needs
//                               as 8-bit pixels (one word each) in LDS, the vertical pass from there, `(p / 255 - mean) / std`, the mask gather
// Only the output window is computed; neither the resized image nor the intermediate of Pillow's two passes exists in memory.
// include/sc2_bottleneck.h states the contract; tests/ref_pil_resize.py restates the two resizes.
// Plain kernels: every index checked against its array before use, no atomics, no workgroup waits for another.
// Shared through input_common.h with cls_input.hip: pil_coeffs, the two passes of a pixel (pil_hpass, pil_vpass) and the tile; with
// det_input.hip as well: the pixel load and the entry's checks (InputNorm).  Their own: every axis goes through pil_coeffs, and an
// entry's last word is the nearest resize's index.
#include "input_common.h"

#pragma clang fp contract(off)   // int() truncates and the sums are ordered: a fused multiply-add in `center` moves xmin for some sizes

namespace {

constexpr int SA_DESC = SC2_SEG_AUGMENT_DESC_INTS;       // int32 words of a descriptor row
constexpr int SA_ENTRY = SC2_SEG_AUGMENT_ENTRY_INTS;     // int32 words of a table entry: first, count, 9 coefficients, nearest index
constexpr int SA_MAX_SIDE = SC2_SEG_AUGMENT_MAX_SIDE;

struct Desc {
    int img, mask, h, w, nh, nw, flip, top, left, eh, ew;
};

__device__ __forceinline__ Desc sa_desc(const int32_t *table, int i) {
    const int32_t *d = table + (size_t)i * SA_DESC;
    Desc s;
    s.img = d[0]; s.mask = d[1]; s.h = d[2]; s.w = d[3]; s.nh = d[4]; s.nw = d[5];
    s.flip = d[6]; s.top = d[7]; s.left = d[8]; s.eh = d[9]; s.ew = d[10];
    return s;
}

// 0: the kernels take the sample; SC2_SEG_AUGMENT_RATIO: a pass shrinks by more than 4; SC2_SEG_AUGMENT_BAD: a field no launch may
// follow (the wrapper refuses those before the launch; the kernels make sure on their own that no such row moves an address)
__device__ __forceinline__ int sa_status(const Desc &s, long long nbytes, int OH, int OW) {
    const bool sides = s.h >= 1 && s.w >= 1 && s.nh >= 1 && s.nw >= 1 && s.h <= SA_MAX_SIDE && s.w <= SA_MAX_SIDE && s.nh <= SA_MAX_SIDE &&
                       s.nw <= SA_MAX_SIDE;
    if (!sides) return SC2_SEG_AUGMENT_BAD;
    const long long px = (long long)s.h * s.w;
    const bool ok = s.img >= 0 && s.mask >= 0 && s.img + 3 * px <= nbytes && s.mask + px <= nbytes && s.top >= 0 && s.left >= 0 &&
                    s.top <= SA_MAX_SIDE && s.left <= SA_MAX_SIDE && s.eh >= 0 && s.ew >= 0 && s.eh <= OH && s.ew <= OW &&
                    (s.flip == 0 || s.flip == 1);
    if (!ok) return SC2_SEG_AUGMENT_BAD;
    if (s.h > 4 * s.nh || s.w > 4 * s.nw) return SC2_SEG_AUGMENT_RATIO;
    return 0;
}

// The table of sample i: OW column entries, then OH row entries.
__device__ __forceinline__ int32_t *sa_table(void *ws, int i, int OH, int OW) {
    return static_cast<int32_t *>(ws) + (size_t)i * (OH + OW) * SA_ENTRY;
}

struct TableArgs {
    const int32_t *desc;
    void *ws;
    int32_t *status;
    long long nbytes;
    int OH, OW, blocks;      // blocks: workgroups along x that compute coefficients; one more walks the nearest sums
};

__global__ __launch_bounds__(PIL_THREADS) void seg_augment_tables_kernel(const TableArgs a) {
    const int i = blockIdx.z, axis = blockIdx.y;      // axis 0: columns, 1: rows
    const Desc s = sa_desc(a.desc, i);
    const int st = sa_status(s, a.nbytes, a.OH, a.OW);
    if (blockIdx.x == 0 && axis == 0 && threadIdx.x == 0) a.status[i] = st;
    if (st != 0) return;
    int32_t *tab = sa_table(a.ws, i, a.OH, a.OW) + (axis == 0 ? 0 : (size_t)a.OW * SA_ENTRY);
    const int len = axis == 0 ? a.OW : a.OH;
    const int n_in = axis == 0 ? s.w : s.h, n_out = axis == 0 ? s.nw : s.nh;
    const int origin = axis == 0 ? s.left : s.top, ext = axis == 0 ? s.ew : s.eh;
    const bool flip = axis == 0 && s.flip != 0;
    if ((int)blockIdx.x < a.blocks) {
        const int o = blockIdx.x * PIL_THREADS + threadIdx.x;
        if (o >= len) return;
        const int r = origin + o;                    // position in the padded, flipped, resized image
        int32_t e[SA_ENTRY];
        if (o < ext && r < n_out) {
            pil_coeffs(n_in, n_out, flip ? n_out - 1 - r : r, e);
        } else {
#pragma unroll
            for (int k = 0; k < SA_ENTRY; ++k) e[k] = 0;
        }
        int32_t *dst = tab + (size_t)o * SA_ENTRY;
#pragma unroll
        for (int k = 0; k < SA_ENTRY - 1; ++k) dst[k] = e[k];
        if (!(o < ext && r < n_out)) dst[SA_ENTRY - 1] = 0;
        return;
    }
    // ImagingScaleAffine's index table: a running sum, so entry j depends on the j additions in front of it -- one lane walks it
    if (threadIdx.x != 0) return;
    const double step = (double)n_in / (double)n_out;
    double xo = step * 0.5;
    int last = origin + ext;                         // resized positions [origin, last) are in the window
    if (last > n_out) last = n_out;
    const int lo = flip ? n_out - last : origin, hi = flip ? n_out - origin : last;      // the same range as resized indices
    for (int j = 0; j < hi; ++j) {
        if (j >= lo) {
            int src = (int)xo;
            if (src > n_in - 1) src = n_in - 1;
            const int o = (flip ? n_out - 1 - j : j) - origin;
            if (o >= 0 && o < len) tab[(size_t)o * SA_ENTRY + SA_ENTRY - 1] = src;
        }
        xo += step;
    }
}

struct TileArgs {
    const uint8_t *buf;
    const int32_t *desc;
    const void *ws;
    float *images;
    long long *targets;
    long long nbytes;
    InputNorm norm;
    int OH, OW;
};

__global__ __launch_bounds__(PIL_THREADS) void seg_augment_tile_kernel(const TileArgs a) {
    __shared__ uint32_t hbuf[PIL_ROWS * PIL_TW];      // [source row][tile column]: the horizontal pass's 8-bit output, R | G << 8 | B << 16
    const int i = blockIdx.z;
    const Desc s = sa_desc(a.desc, i);
    if (sa_status(s, a.nbytes, a.OH, a.OW) != 0) return;      // (wave-uniform: the whole workgroup leaves)
    const int y0 = blockIdx.y * PIL_TH, x0 = blockIdx.x * PIL_TW;
    const int32_t *cols = static_cast<const int32_t *>(a.ws) + (size_t)i * (a.OH + a.OW) * SA_ENTRY;
    const int32_t *rows = cols + (size_t)a.OW * SA_ENTRY;
    // the part of the tile that shows resized pixels: rows [y0, yv), columns [x0, xv)
    const int yv = min(min(y0 + PIL_TH, s.eh), s.nh - s.top), xv = min(min(x0 + PIL_TW, s.ew), s.nw - s.left);
    const int lx = threadIdx.x & (PIL_TW - 1), ly = threadIdx.x / PIL_TW;      // a wave owns a row, its lanes the columns
    const int x = x0 + lx;
    int r_first = 0, r_count = 0;
    if (yv > y0 && xv > x0) {
        // the bounds do not decrease with the output index, so the band's source rows run from its first row's to its last row's
        const int32_t *ef = rows + (size_t)y0 * SA_ENTRY, *el = rows + (size_t)(yv - 1) * SA_ENTRY;
        r_first = ef[0];
        r_count = min(el[0] + el[1] - r_first, PIL_ROWS);
        if (x < xv) {
            const int32_t *e = cols + (size_t)x * SA_ENTRY;
            const int first = e[0], count = e[1];
            int k[PIL_TAPS];
#pragma unroll
            for (int t = 0; t < PIL_TAPS; ++t) k[t] = e[2 + t];
            const uint8_t *img = a.buf + s.img;
            const size_t img_bytes = (size_t)s.h * s.w * 3;
            for (int r = ly; r < r_count; r += PIL_THREADS / PIL_TW) {
                const int sr = min(max(r_first + r, 0), s.h - 1);
                hbuf[r * PIL_TW + lx] = pil_hpass(img, img_bytes, s.w, sr, first, count, k);
            }
        }
    }
    __syncthreads();
    if (x >= a.OW) return;
    const size_t plane = (size_t)a.OH * a.OW;
    float *out = a.images + (size_t)i * 3 * plane;
    long long *tgt = a.targets + (size_t)i * plane;
    const uint8_t *mask = a.buf + s.mask;
    const int mcol = x < xv ? min(max(cols[(size_t)x * SA_ENTRY + SA_ENTRY - 1], 0), s.w - 1) : 0;
    for (int y = y0 + ly; y < min(y0 + PIL_TH, a.OH); y += PIL_THREADS / PIL_TW) {
        float v0, v1, v2;
        long long label = 255;
        if (y >= s.eh || x >= s.ew) {                 // outside the sample's extent: the collator's fill
            v0 = v1 = v2 = 0.0f;
        } else if (y >= yv || x >= xv) {              // pad_if_smaller's area: a zero pixel, normalised
            v0 = __fdiv_rn(0.0f - a.norm.mean[0], a.norm.std[0]);
            v1 = __fdiv_rn(0.0f - a.norm.mean[1], a.norm.std[1]);
            v2 = __fdiv_rn(0.0f - a.norm.mean[2], a.norm.std[2]);
        } else {
            const int32_t *e = rows + (size_t)y * SA_ENTRY;
            pil_vpass<PIL_ROWS, PIL_TW>(hbuf, lx, e, e[0] - r_first, a.norm.mean, a.norm.std, v0, v1, v2);
            const int mrow = min(max(e[SA_ENTRY - 1], 0), s.h - 1);
            label = (long long)mask[(size_t)mrow * s.w + mcol];
        }
        const size_t o = (size_t)y * a.OW + x;
        out[o] = v0;
        out[plane + o] = v1;
        out[2 * plane + o] = v2;
        tgt[o] = label;
    }
}

bool sa_sizes_ok(int n, int oh, int ow) {
    return n >= 1 && n <= SC2_SEG_AUGMENT_MAX_BATCH && oh >= 1 && ow >= 1 && oh <= SA_MAX_SIDE && ow <= SA_MAX_SIDE;
}

}  // namespace

extern "C" long long sc2_seg_augment_workspace(int n, int oh, int ow) {
    if (!sa_sizes_ok(n, oh, ow)) return 0;
    return (long long)n * (oh + ow) * SA_ENTRY * (long long)sizeof(int32_t);
}

extern "C" int sc2_seg_augment(const uint8_t *buf, long long nbytes, const int32_t *desc, int n, int oh, int ow, const float *mean,
                               const float *std, float *images, long long *targets, void *ws, int32_t *status, void *stream) {
    SC2_REQUIRE(sa_sizes_ok(n, oh, ow), SC2_ERR_UNSUPPORTED, "seg_augment: %d samples of %dx%d (1..%d samples, sides 1..%d)", n, oh, ow,
                SC2_SEG_AUGMENT_MAX_BATCH, SA_MAX_SIDE);
    const uintptr_t words = reinterpret_cast<uintptr_t>(desc) | reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(ws) |
                            reinterpret_cast<uintptr_t>(status);
    TileArgs a;
    const int rc = a.norm.take("seg_augment", nbytes, buf && desc && mean && std && images && targets && ws && status,
                               (words & 3u) == 0 && (reinterpret_cast<uintptr_t>(targets) & 7u) == 0, mean, std);
    if (rc != SC2_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TableArgs t;
    t.desc = desc; t.ws = ws; t.status = status; t.nbytes = nbytes; t.OH = oh; t.OW = ow;
    t.blocks = ((oh > ow ? oh : ow) + PIL_THREADS - 1) / PIL_THREADS;
    hipLaunchKernelGGL(seg_augment_tables_kernel, dim3((unsigned)t.blocks + 1, 2, (unsigned)n), dim3(PIL_THREADS), 0, s, t);
    SC2_CHECK_LAUNCH();
    a.buf = buf; a.desc = desc; a.ws = ws; a.images = images; a.targets = targets; a.nbytes = nbytes;
    a.OH = oh; a.OW = ow;
    const dim3 grid((unsigned)((ow + PIL_TW - 1) / PIL_TW), (unsigned)((oh + PIL_TH - 1) / PIL_TH), (unsigned)n);
    hipLaunchKernelGGL(seg_augment_tile_kernel, grid, dim3(PIL_THREADS), 0, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
