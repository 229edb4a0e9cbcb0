// What the two baseline-JPEG kernels share (csrc/jpeg.hip: a whole image of at most 64 x 64 on chip; csrc/jpeg_image.hip: images cut
// into strips and chunks): the Annex K tables, the slow-integer DCT pair, the coder of one scan block, the workgroup prefix sum and the
// taps of the triangle upsampler.  include/sc2_bottleneck.h (sc2_jpeg_tensor_codec) states the arithmetic.
#pragma once
#include "sc2_common.h"

namespace {

constexpr int JBLOCK_BITS = 22 + 63 * 26;     // DC: a code of at most 11 bits + 11; AC: 63 x (16 + 10)

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

// the tables into LDS: a straight copy, lane by lane
__device__ __forceinline__ void jpeg_copy_tables(JpegTables *tab, int tid, int lanes) {
    const uint32_t *from = reinterpret_cast<const uint32_t *>(&k_jpeg_tables);
    uint32_t *to = reinterpret_cast<uint32_t *>(tab);
    for (int i = tid; i < (int)(sizeof(JpegTables) / 4); i += lanes) to[i] = from[i];
}

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

// Appends bits, most significant first, at a bit offset of an array of WORDS words: whole words are OR-ed in as they fill up.  The
// first and the last word of a block are shared with its neighbours, hence the atomic; the bits of two blocks never overlap.
template <int WORDS>
struct EmitBits {
    uint32_t *buf;
    unsigned long long acc;
    int word, n;
    __device__ __forceinline__ void put(uint32_t v, int len) {
        acc = (acc << len) | v;
        n += len;
        if (n >= 32) {
            n -= 32;
            if (word < WORDS) atomicOr(&buf[word], (uint32_t)(acc >> n));
            ++word;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0 && word < WORDS) atomicOr(&buf[word], (uint32_t)(acc << (32 - n)));
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

// exclusive prefix sum over a workgroup of LANES lanes; `total` = the sum
template <int LANES>
__device__ __forceinline__ int block_scan(int v, int *sh, int tid, int &total) {
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < LANES; off <<= 1) {
        const int t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    total = sh[LANES - 1];
    const int r = sh[tid] - v;
    __syncthreads();
    return r;
}

// The horizontal taps of the h2v2 triangle upsampler on s = 3 near + far: `nr` / `fr` are the near and the far chroma row, cx the
// sample's column in them; `first` / `last`: cx is the first / the last column of the real chroma plane; odd: the output column is odd.
__device__ __forceinline__ int chroma_taps(const uint8_t *nr, const uint8_t *fr, int cx, bool first, bool last, bool odd) {
    const int s = 3 * nr[cx] + fr[cx];
    if (odd) {
        if (last) return (4 * s + 7) >> 4;
        return (3 * s + 3 * nr[cx + 1] + fr[cx + 1] + 7) >> 4;
    }
    if (first) return (4 * s + 8) >> 4;
    return (3 * s + 3 * nr[cx - 1] + fr[cx - 1] + 8) >> 4;
}

}  // namespace
