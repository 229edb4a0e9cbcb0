// Codec feature-compression baseline (sc2bench's PILTensorModule with format='JPEG'): a feature map [B,C,H,W] goes through the 8-bit
// baseline JPEG process three channels at a time, one workgroup per (sample, channel group) image, everything on chip
// (sc2_jpeg_tensor_codec).  include/sc2_bottleneck.h states the contract; tests/ref_jpeg.py restates it as a sequential integer
// program.  Baseline JPEG is integer arithmetic from the 8-bit samples on, so the bytes, their count and the reconstruction are exact.
// Plain kernel: every index checked against its array before use, LDS atomics only (an integer OR of disjoint bits: the order of
// arrival cannot show), no workgroup waits for another.
#include "jpeg_common.h"

#pragma clang fp contract(off)   // `((v - low) / high) * 255` and `(p / 255) * high + low`: every step rounded once

namespace {

constexpr int JT = 256;                       // lanes of a workgroup
constexpr int JSIDE = SC2_JPEG_MAX_SIDE;      // 64: at most 8 x 8 luma blocks, 4 x 4 blocks per chroma plane
constexpr int JBLOCKS = 96;                   // 64 + 16 + 16
constexpr int JWORDS = JBLOCKS * 64;          // the int32 work area: DCT rows / columns, then the scan's bits, then the IDCT
constexpr int CB_AT = JSIDE * JSIDE, CR_AT = CB_AT + 32 * 32, CPITCH = 32;     // the decoded planes inside `pix`
static_assert(JBLOCKS * JBLOCK_BITS <= JWORDS * 32, "the longest scan fits the work area");

struct JpegArgs {
    const float *x;
    float *recon;
    int32_t *sizes;
    float *extrema;
    int32_t *status;
    uint8_t *bytes;
    long long slot;
    int C, H, W, quality, per_sample;
};

// h2v2 upsampling of one chroma sample position: the triangle filter where the plane has more than two columns (the row beyond an
// edge of the real plane equals the edge row), plain repetition otherwise.
__device__ __forceinline__ int chroma_at(const uint8_t *p, int y, int x, int ch, int cw) {
    const int cy = y >> 1, cx = x >> 1;
    if (cw <= 2) return p[cy * CPITCH + cx];
    const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    return chroma_taps(p + cy * CPITCH, p + fy * CPITCH, cx, cx == 0, cx == cw - 1, x & 1);
}

__global__ __launch_bounds__(JT) void jpeg_tensor_codec_kernel(const JpegArgs a) {
    __shared__ int ws[JWORDS];                         // 24 KB
    __shared__ short coef[JWORDS];                     // 12 KB: quantised coefficients, natural order, block after block
    __shared__ uint8_t pix[3 * JSIDE * JSIDE];         // 12 KB: the 8-bit input planes; later the decoded Y, Cb, Cr planes
    __shared__ JpegTables tab;
    __shared__ uint16_t qt[2][64];
    __shared__ int scan[JT];
    __shared__ float red_lo[JT / 64], red_hi[JT / 64];
    __shared__ int red_bad[JT / 64];

    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    const int sample = img / a.per_sample, g = img - sample * a.per_sample;
    const int H = a.H, W = a.W, HW = H * W;
    const int n3 = a.C / 3;
    const bool rgb = g < n3;
    const int nch = rgb ? 3 : 1;
    const int c0 = rgb ? 3 * g : 3 * n3 + (g - n3);
    const long long first = ((long long)sample * a.C + c0) * HW;
    const float *src = a.x + first;
    const int n = nch * HW;

    jpeg_copy_tables(&tab, tid, JT);

    // ---- the group's extrema
    float lo = __builtin_inff(), hi = -__builtin_inff();
    int bad = 0;
    for (int i = tid; i < n; i += JT) {
        const float v = src[i];
        bad |= !(v - v == 0.0f);      // NaN or an infinity
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const float olo = __shfl_xor(lo, m), ohi = __shfl_xor(hi, m);
        bad |= __shfl_xor(bad, m);
        lo = olo < lo ? olo : lo;
        hi = ohi > hi ? ohi : hi;
    }
    if ((tid & 63) == 0) {
        red_lo[tid >> 6] = lo;
        red_hi[tid >> 6] = hi;
        red_bad[tid >> 6] = bad;
    }
    __syncthreads();
    for (int w = 0; w < JT / 64; ++w) {
        lo = red_lo[w] < lo ? red_lo[w] : lo;
        hi = red_hi[w] > hi ? red_hi[w] : hi;
        bad |= red_bad[w];
    }
    const float low = lo, high = hi;
    const int st = bad ? SC2_JPEG_NOT_FINITE : (low < 0.0f ? SC2_JPEG_NEGATIVE_MIN : 0) | (!(high > 0.0f) ? SC2_JPEG_ZERO_MAX : 0);
    if (tid == 0) {
        a.extrema[2 * (long long)img] = low;
        a.extrema[2 * (long long)img + 1] = high;
        a.status[img] = st;
        if (st) a.sizes[img] = 0;
    }
    if (st) return;      // (the same for every lane)

    if (tid < 128) {     // the two tables at this quality
        const int q = a.quality;
        const int s = q < 50 ? 5000 / q : 200 - 2 * q;
        const int v = (tab.base_q[tid >> 6][tid & 63] * s + 50) / 100;
        qt[tid >> 6][tid & 63] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }

    // ---- 8-bit samples
    for (int i = tid; i < n; i += JT) {
        const int c = i / HW, r = i - c * HW;
        const int y = r / W, x = r - y * W;
        const float f = ((src[i] - low) / high) * 255.0f;
        pix[c * JSIDE * JSIDE + y * JSIDE + x] = (uint8_t)(int)f;
    }
    __syncthreads();

    // ---- geometry: luma / grey blocks, MCUs (= chroma blocks), the real chroma plane
    const int wb = (W + 7) >> 3, hb = (H + 7) >> 3, mx = (W + 15) >> 4, my = (H + 15) >> 4;
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const int nY = wb * hb, nC = mx * my;
    const int nblk = rgb ? nY + 2 * nC : nY;

    // ---- level-shifted samples of every block: luma / grey edge-replicated, chroma through the 2 x 2 box filter
    for (int e = tid; e < nblk * 64; e += JT) {
        const int blk = e >> 6, r = (e >> 3) & 7, c = e & 7;
        int v;
        if (blk < nY) {
            const int by = blk / wb, bx = blk - by * wb;
            const int at = min(8 * by + r, H - 1) * JSIDE + min(8 * bx + c, W - 1);
            v = rgb ? (19595 * pix[at] + 38470 * pix[JSIDE * JSIDE + at] + 7471 * pix[2 * JSIDE * JSIDE + at] + 32768) >> 16 : pix[at];
        } else {
            const int comp = (blk - nY) >= nC;
            const int cblk = blk - nY - comp * nC;
            const int cby = cblk / mx, cbx = cblk - cby * mx;
            const int cy = min(8 * cby + r, ch - 1), cx = 8 * cbx + c;
            const int y0 = 2 * cy, y1 = min(2 * cy + 1, H - 1), x0 = min(2 * cx, W - 1), x1 = min(2 * cx + 1, W - 1);
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int at = ((k >> 1) ? y1 : y0) * JSIDE + ((k & 1) ? x1 : x0);
                const int R = pix[at], G = pix[JSIDE * JSIDE + at], Bv = pix[2 * JSIDE * JSIDE + at];
                sum += comp ? (32768 * R - 27439 * G - 5329 * Bv + (128 << 16) + 32767) >> 16
                            : (-11059 * R - 21709 * G + 32768 * Bv + (128 << 16) + 32767) >> 16;
            }
            v = (sum + 1 + (cx & 1)) >> 2;
        }
        ws[e] = v - 128;
    }
    __syncthreads();

    // ---- forward DCT: rows, then columns + quantisation
    for (int t = tid; t < nblk * 8; t += JT) {
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = ws[t * 8 + i];
        fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[t * 8 + i] = d[i];
    }
    __syncthreads();
    for (int t = tid; t < nblk * 8; t += JT) {
        const int blk = t >> 3, c = t & 7;
        const uint16_t *q = qt[rgb && blk >= nY];
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = ws[blk * 64 + 8 * i + c];
        fdct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int div = 8 * q[8 * i + c];
            const int mag = ((d[i] < 0 ? -d[i] : d[i]) + (div >> 1)) / div;
            coef[blk * 64 + 8 * i + c] = (short)(d[i] < 0 ? -mag : mag);
        }
    }
    __syncthreads();

    // ---- the scan: one lane per block in scan order.  Lengths first, a prefix sum for the bit offsets, then the bits.
    const int n_scan = rgb ? 6 * nC : nY;
    const short *blk_coef = nullptr;
    int diff = 0, table = 0;
    if (tid < n_scan) {
        if (rgb) {
            const int m = tid / 6, k = tid - 6 * m;
            if (k < 4) {
                // DC of luma block k of MCU m; a block beyond the grid carries the DC of the block before it in the MCU (block 0 is real)
                auto y_dc = [&](int mm, int kk, bool &real) {
                    const int m_y = mm / mx, m_x = mm - m_y * mx;
                    real = true;
                    for (;; --kk) {
                        const int by = 2 * m_y + (kk >> 1), bx = 2 * m_x + (kk & 1);
                        if ((by < hb && bx < wb) || kk == 0) return (by * wb + bx) * 64;
                        real = false;
                    }
                };
                bool real, other;
                const int at = y_dc(m, k, real);
                const int pred = k > 0 ? coef[y_dc(m, k - 1, other)] : (m > 0 ? coef[y_dc(m - 1, 3, other)] : 0);
                diff = coef[at] - pred;
                blk_coef = real ? coef + at : nullptr;
            } else {
                const int at = (nY + (k - 4) * nC + m) * 64;
                diff = coef[at] - (m > 0 ? coef[at - 64] : 0);
                blk_coef = coef + at;
                table = 1;
            }
        } else {
            diff = coef[tid * 64] - (tid > 0 ? coef[(tid - 1) * 64] : 0);
            blk_coef = coef + tid * 64;
        }
    }
    int my_bits = 0;
    if (tid < n_scan) {
        CountBits cnt = {0};
        code_block(cnt, blk_coef, diff, tab.dc[table], tab.ac[table], tab.zigzag);
        my_bits = cnt.n;
    }
    int total_bits;
    const int bit_at = block_scan<JT>(my_bits, scan, tid, total_bits);
    const int n_bytes = (total_bits + 7) >> 3;
    uint32_t *bits = reinterpret_cast<uint32_t *>(ws);
    for (int i = tid; i < min((n_bytes + 3) >> 2, JWORDS); i += JT) bits[i] = 0u;
    __syncthreads();
    if (tid < n_scan) {
        EmitBits<JWORDS> em = {bits, 0ull, bit_at >> 5, bit_at & 31};
        code_block(em, blk_coef, diff, tab.dc[table], tab.ac[table], tab.zigzag);
        em.finish();
    }
    if (tid == JT - 1 && (total_bits & 7)) {     // the last byte is filled up with 1 bits (they lie inside one word)
        const int pad = 8 - (total_bits & 7);
        const int word = total_bits >> 5;
        if (word < JWORDS) atomicOr(&bits[word], ((1u << pad) - 1u) << (32 - (total_bits & 31) - pad));
    }
    __syncthreads();

    // ---- a zero byte follows every 0xFF: count them per lane's run of bytes, prefix sum, place
    const int per_lane = (n_bytes + JT - 1) / JT;
    const int b0 = min(tid * per_lane, n_bytes), b1 = min(b0 + per_lane, n_bytes);
    int ff = 0;
    for (int b = b0; b < b1; ++b) ff += ((bits[b >> 2] >> (24 - 8 * (b & 3))) & 0xFFu) == 0xFFu;
    int total_ff;
    const int ff_before = block_scan<JT>(ff, scan, tid, total_ff);
    if (tid == 0) a.sizes[img] = (rgb ? SC2_JPEG_HEADER_RGB : SC2_JPEG_HEADER_GREY) + n_bytes + total_ff + 2;     // header, segment, EOI
    if (a.bytes) {
        uint8_t *out = a.bytes + (long long)img * a.slot;
        long long o = b0 + ff_before;
        for (int b = b0; b < b1; ++b) {
            const uint32_t v = (bits[b >> 2] >> (24 - 8 * (b & 3))) & 0xFFu;
            if (o < a.slot) out[o] = (uint8_t)v;
            ++o;
            if (v == 0xFFu) {
                if (o < a.slot) out[o] = 0;
                ++o;
            }
        }
    }
    __syncthreads();     // the work area changes hands again

    // ---- decode from the coefficients: dequantise, inverse DCT columns, then rows into the 8-bit planes
    for (int t = tid; t < nblk * 8; t += JT) {
        const int blk = t >> 3, c = t & 7;
        const uint16_t *q = qt[rgb && blk >= nY];
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = coef[blk * 64 + 8 * i + c] * q[8 * i + c];
        idct8<11>(v);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[blk * 64 + 8 * i + c] = v[i];
    }
    __syncthreads();
    for (int t = tid; t < nblk * 8; t += JT) {
        const int blk = t >> 3, r = t & 7;
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ws[t * 8 + i];
        idct8<18>(v);
        int at;
        if (blk < nY) {
            const int by = blk / wb, bx = blk - by * wb;
            at = (8 * by + r) * JSIDE + 8 * bx;
        } else {
            const int comp = (blk - nY) >= nC;
            const int cblk = blk - nY - comp * nC;
            const int cby = cblk / mx, cbx = cblk - cby * mx;
            at = (comp ? CR_AT : CB_AT) + (8 * cby + r) * CPITCH + 8 * cbx;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) pix[at + i] = (uint8_t)clamp255(v[i] + 128);
    }
    __syncthreads();

    // ---- pixels: chroma up, colour conversion, and back to the group's range
    float *dst = a.recon + first;
    for (int i = tid; i < HW; i += JT) {
        const int y = i / W, x = i - y * W;
        const int Y = pix[y * JSIDE + x];
        if (!rgb) {
            dst[i] = ((float)Y / 255.0f) * high + low;
            continue;
        }
        const int cb = chroma_at(pix + CB_AT, y, x, ch, cw) - 128, cr = chroma_at(pix + CR_AT, y, x, ch, cw) - 128;
        const int R = clamp255(Y + ((91881 * cr + 32768) >> 16));
        const int G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        const int Bv = clamp255(Y + ((116130 * cb + 32768) >> 16));
        dst[i] = ((float)R / 255.0f) * high + low;
        dst[HW + i] = ((float)G / 255.0f) * high + low;
        dst[2 * HW + i] = ((float)Bv / 255.0f) * high + low;
    }
}

long long jpeg_scan_blocks(int mode, int H, int W) {
    return mode == SC2_JPEG_RGB ? 6ll * ((H + 15) / 16) * ((W + 15) / 16) : (long long)((H + 7) / 8) * ((W + 7) / 8);
}

}  // namespace

extern "C" long long sc2_jpeg_max_bytes(int mode, int H, int W) {
    if ((mode != SC2_JPEG_GREY && mode != SC2_JPEG_RGB) || H < 1 || W < 1 || H > SC2_JPEG_MAX_SIDE || W > SC2_JPEG_MAX_SIDE) return -1;
    return 2 * ((jpeg_scan_blocks(mode, H, W) * JBLOCK_BITS + 7) / 8);
}

extern "C" int sc2_jpeg_tensor_codec(const float *x, int B, int C, int H, int W, int quality, float *recon, int32_t *sizes, float *extrema,
                                     int32_t *status, uint8_t *bytes, long long slot_bytes, void *stream) {
    SC2_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, SC2_ERR_INVALID_ARG, "jpeg_tensor_codec: bad dims B=%d C=%d %dx%d", B, C, H, W);
    SC2_REQUIRE(H <= SC2_JPEG_MAX_SIDE && W <= SC2_JPEG_MAX_SIDE, SC2_ERR_UNSUPPORTED, "jpeg_tensor_codec: %dx%d (at most %d per side)", H, W,
                SC2_JPEG_MAX_SIDE);
    SC2_REQUIRE(quality >= 1 && quality <= 100, SC2_ERR_INVALID_ARG, "jpeg_tensor_codec: quality %d (1..100)", quality);
    SC2_REQUIRE(x && recon && sizes && extrema && status, SC2_ERR_INVALID_ARG, "jpeg_tensor_codec: null pointer");
    SC2_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(recon) | reinterpret_cast<uintptr_t>(sizes) |
                  reinterpret_cast<uintptr_t>(extrema) | reinterpret_cast<uintptr_t>(status)) & 3u) == 0,
                SC2_ERR_INVALID_ARG, "jpeg_tensor_codec: misaligned pointer");
    const int per_sample = C / 3 + C % 3;
    const long long n_img = (long long)B * per_sample;
    SC2_REQUIRE(n_img <= 0x7FFFFFFFll, SC2_ERR_UNSUPPORTED, "jpeg_tensor_codec: %lld images in one call", n_img);
    if (bytes) {
        const long long need = sc2_jpeg_max_bytes(C >= 3 ? SC2_JPEG_RGB : SC2_JPEG_GREY, H, W);
        SC2_REQUIRE(slot_bytes >= need, SC2_ERR_INVALID_ARG, "jpeg_tensor_codec: byte slots of %lld (at least %lld)", slot_bytes, need);
    }
    JpegArgs a;
    a.x = x;
    a.recon = recon;
    a.sizes = sizes;
    a.extrema = extrema;
    a.status = status;
    a.bytes = bytes;
    a.slot = bytes ? slot_bytes : 0;
    a.C = C; a.H = H; a.W = W; a.quality = quality; a.per_sample = per_sample;
    hipLaunchKernelGGL(jpeg_tensor_codec_kernel, dim3((unsigned)n_img), dim3(JT), 0, static_cast<hipStream_t>(stream), a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
