// Codec feature-compression baseline (sc2bench's PILTensorModule with format='JPEG'): a feature map [B,C,H,W] goes through the 8-bit
// baseline JPEG process three channels at a time, one workgroup per (sample, channel group) image, everything on chip
// (sc2_jpeg_tensor_codec).  include/sc2_bottleneck.h states the contract; tests/ref_jpeg.py restates it as a sequential integer
// program.  Baseline JPEG is integer arithmetic from the 8-bit samples on, so the bytes, their count and the reconstruction are exact.
// Plain kernel: every index checked against its array before use, LDS atomics only (an integer OR of disjoint bits: the order of
// arrival cannot show), no workgroup waits for another.
#include "sc2_common.h"

#pragma clang fp contract(off)   // `((v - low) / high) * 255` and `(p / 255) * high + low`: every step rounded once

namespace {

constexpr int JT = 256;                       // lanes of a workgroup
constexpr int JSIDE = SC2_JPEG_MAX_SIDE;      // 64: at most 8 x 8 luma blocks, 4 x 4 blocks per chroma plane
constexpr int JBLOCKS = 96;                   // 64 + 16 + 16
constexpr int JWORDS = JBLOCKS * 64;          // the int32 work area: DCT rows / columns, then the scan's bits, then the IDCT
constexpr int JBLOCK_BITS = 22 + 63 * 26;     // DC: a code of at most 11 bits + 11; AC: 63 x (16 + 10)
constexpr int CB_AT = JSIDE * JSIDE, CR_AT = CB_AT + 32 * 32, CPITCH = 32;     // the decoded planes inside `pix`
static_assert(JBLOCKS * JBLOCK_BITS <= JWORDS * 32, "the longest scan fits the work area");

constexpr int K_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                              35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K quantisation tables, natural order
constexpr int K_LUM_Q[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr int K_CHR_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K Huffman tables: codes per length 1..16, then the symbols in code order
constexpr int K_DC_LUM_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr int K_DC_CHR_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr int K_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr int K_AC_LUM_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr int K_AC_LUM_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr int K_AC_CHR_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr int K_AC_CHR_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// What a workgroup copies into LDS when it starts: per symbol (code length << 16) | code, 0 for a symbol the table does not hold;
// the two quantisation bases; the zigzag order.
struct JpegTables {
    uint32_t ac[2][256];
    uint32_t dc[2][16];
    uint8_t base_q[2][64];
    uint8_t zigzag[64];
};

constexpr void jpeg_fill_codes(uint32_t *out, const int *bits, const int *vals) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}

constexpr JpegTables jpeg_make_tables() {
    JpegTables t = {};
    jpeg_fill_codes(t.ac[0], K_AC_LUM_BITS, K_AC_LUM_VALS);
    jpeg_fill_codes(t.ac[1], K_AC_CHR_BITS, K_AC_CHR_VALS);
    jpeg_fill_codes(t.dc[0], K_DC_LUM_BITS, K_DC_VALS);
    jpeg_fill_codes(t.dc[1], K_DC_CHR_BITS, K_DC_VALS);
    for (int i = 0; i < 64; ++i) {
        t.base_q[0][i] = (uint8_t)K_LUM_Q[i];
        t.base_q[1][i] = (uint8_t)K_CHR_Q[i];
        t.zigzag[i] = (uint8_t)K_ZIGZAG[i];
    }
    return t;
}

__device__ const JpegTables k_jpeg_tables = jpeg_make_tables();

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

__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// One pass of the forward "islow" DCT over eight values (the constants are FIX(x) = round(x * 2^13)).  FIRST: the row pass, outputs
// scaled by 4; otherwise the column pass, which takes that scale out again.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int N = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    const int e1 = (t12 + t13) * 4433;
    d[2] = descale(e1 + t13 * 6270, N);
    d[6] = descale(e1 - t12 * 15137, N);
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = -(t4 + t7) * 7373, z2 = -(t5 + t6) * 20995, z3 = -(t4 + t6) * 16069 + z5, z4 = -(t5 + t7) * 3196 + z5;
    d[7] = descale(t4 * 2446 + z1 + z3, N);
    d[5] = descale(t5 * 16819 + z2 + z4, N);
    d[3] = descale(t6 * 25172 + z2 + z3, N);
    d[1] = descale(t7 * 12299 + z1 + z4, N);
}

// One pass of the inverse: N = 11 for the columns, 18 for the rows.
template <int N>
__device__ __forceinline__ void idct8(int (&v)[8]) {
    const int e1 = (v[2] + v[6]) * 4433;
    const int e2 = e1 - v[6] * 15137, e3 = e1 + v[2] * 6270;
    const int e0 = (v[0] + v[4]) * 8192, e4 = (v[0] - v[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e4 + e2, t12 = e4 - e2;
    int t0 = v[7], t1 = v[5], t2 = v[3], t3 = v[1];
    const int z5 = (t0 + t2 + t1 + t3) * 9633;
    const int z1 = -(t0 + t3) * 7373, z2 = -(t1 + t2) * 20995, z3 = -(t0 + t2) * 16069 + z5, z4 = -(t1 + t3) * 3196 + z5;
    t0 = t0 * 2446 + z1 + z3;
    t1 = t1 * 16819 + z2 + z4;
    t2 = t2 * 25172 + z2 + z3;
    t3 = t3 * 12299 + z1 + z4;
    v[0] = descale(t10 + t3, N); v[7] = descale(t10 - t3, N);
    v[1] = descale(t11 + t2, N); v[6] = descale(t11 - t2, N);
    v[2] = descale(t12 + t1, N); v[5] = descale(t12 - t1, N);
    v[3] = descale(t13 + t0, N); v[4] = descale(t13 - t0, N);
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

struct CountBits {
    int n;
    __device__ __forceinline__ void put(uint32_t, int len) { n += len; }
};

// Appends bits, most significant first, at a bit offset of the word array: whole words are OR-ed in as they fill up.  The first and
// the last word of a block are shared with its neighbours, hence the atomic; the bits of two blocks never overlap.
struct EmitBits {
    uint32_t *buf;
    unsigned long long acc;
    int word, n;
    __device__ __forceinline__ void put(uint32_t v, int len) {
        acc = (acc << len) | v;
        n += len;
        if (n >= 32) {
            n -= 32;
            if (word < JWORDS) atomicOr(&buf[word], (uint32_t)(acc >> n));
            ++word;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0 && word < JWORDS) atomicOr(&buf[word], (uint32_t)(acc << (32 - n)));
    }
};

__device__ __forceinline__ int magnitude_bits(int v) {
    const int a = v < 0 ? -v : v;
    const int n = 32 - __clz(a);      // (__clz(0) = 32)
    return n < 15 ? n : 15;           // a baseline coefficient has at most 11: the table index stays inside its array whatever comes
}

template <typename Sink>
__device__ __forceinline__ void put_value(Sink &s, uint32_t entry, int v, int n) {
    s.put(entry & 0xFFFFu, (int)(entry >> 16));
    if (n) s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
}

// One block of the scan: the DC difference, then the AC coefficients in zigzag order as (run, size) symbols.  c == nullptr: a dummy
// block (no AC).
template <typename Sink>
__device__ __forceinline__ void code_block(Sink &s, const short *c, int diff, const uint32_t *dc, const uint32_t *ac, const uint8_t *zigzag) {
    const int nd = magnitude_bits(diff);
    put_value(s, dc[nd], diff, nd);
    int run = 0;
    if (c) {
        for (int k = 1; k < 64; ++k) {
            const int v = c[zigzag[k]];
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                s.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
                run -= 16;
            }
            const int n = magnitude_bits(v);
            put_value(s, ac[(run << 4) + n], v, n);
            run = 0;
        }
    } else {
        run = 63;
    }
    if (run) s.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

// exclusive prefix sum over the workgroup; `total` = the sum
__device__ __forceinline__ int block_scan(int v, int *sh, int tid, int &total) {
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < JT; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    total = sh[JT - 1];
    const int r = sh[tid] - v;
    __syncthreads();
    return r;
}

// h2v2 upsampling of one chroma sample position: the triangle filter where the plane has more than two columns (the row beyond an
// edge of the real plane equals the edge row), plain repetition otherwise.
__device__ __forceinline__ int chroma_at(const uint8_t *p, int y, int x, int ch, int cw) {
    const int cy = y >> 1, cx = x >> 1;
    if (cw <= 2) return p[cy * CPITCH + cx];
    const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
    const uint8_t *nr = p + cy * CPITCH, *fr = p + fy * CPITCH;
    const int s = 3 * nr[cx] + fr[cx];
    if (x & 1) {
        if (cx == cw - 1) return (4 * s + 7) >> 4;
        return (3 * s + 3 * nr[cx + 1] + fr[cx + 1] + 7) >> 4;
    }
    if (cx == 0) return (4 * s + 8) >> 4;
    return (3 * s + 3 * nr[cx - 1] + fr[cx - 1] + 8) >> 4;
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

    {   // tables: a straight copy, lane by lane
        const uint32_t *from = reinterpret_cast<const uint32_t *>(&k_jpeg_tables);
        uint32_t *to = reinterpret_cast<uint32_t *>(&tab);
        for (int i = tid; i < (int)(sizeof(JpegTables) / 4); i += JT) to[i] = from[i];
    }

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
    const int bit_at = block_scan(my_bits, scan, tid, total_bits);
    const int n_bytes = (total_bits + 7) >> 3;
    uint32_t *bits = reinterpret_cast<uint32_t *>(ws);
    for (int i = tid; i < min((n_bytes + 3) >> 2, JWORDS); i += JT) bits[i] = 0u;
    __syncthreads();
    if (tid < n_scan) {
        EmitBits em = {bits, 0ull, bit_at >> 5, bit_at & 31};
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
    const int ff_before = block_scan(ff, scan, tid, total_ff);
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
