// Codec input-compression baseline (sc2bench's PILImageModule with format='JPEG'): 8-bit images [B,C,H,W] of up to
// SC2_JPEG_IMAGE_MAX_SIDE per side through the baseline JPEG process of csrc/jpeg.hip, byte for byte (sc2_jpeg_image_codec;
// include/sc2_bottleneck.h states the contract, tests/ref_jpeg.py restates the arithmetic).  An image of that size does not fit on chip,
// so the work is cut into three launches on one stream, and the launch boundaries are the only dependencies between them:
//   transform: one workgroup per (image, MCU row, chunk of 128 columns): pixels -> quantised coefficients, int16, in scan order, in the
//              caller's workspace (a dummy Y block as what the scan codes for it: the DC of the block before it in the MCU, no AC);
//   entropy  : one workgroup per image walks the scan in chunks of SC2_JPEG_IMAGE_CHUNK_BLOCKS blocks, carrying the bits of the last,
//              partial byte and the count of bytes written; a block's DC predecessor is a stored coefficient (chunk or workspace);
//   decode   : one workgroup per (image, MCU row, chunk of 128 columns): coefficients -> pixels; the chroma blocks one MCU around the
//              strip are decoded along with it for the triangle upsampler's context rows and columns.
// Plain kernels: every index checked against its array before use, LDS atomics only (an integer OR of disjoint bits), no workgroup
// waits for another, nothing is read from the workspace or an output before these launches wrote it.
#include "jpeg_common.h"

namespace {

constexpr int IT = 256;                                   // lanes of a transform / decode workgroup
constexpr int ET = SC2_JPEG_IMAGE_CHUNK_BLOCKS;           // lanes of an entropy workgroup: one per scan block of a chunk
constexpr int STRIP_W = 128;                              // pixel columns of a workgroup: 8 MCUs, or 16 grey blocks
constexpr int STRIP_MCUS = STRIP_W / 16, STRIP_GREY = STRIP_W / 8;
constexpr int TBLOCKS = 6 * STRIP_MCUS;                   // 48 blocks per transform workgroup
constexpr int WS_PITCH = 72;                              // words per block of the DCT work area: 64 + 8, so that the column pass
                                                          // (lanes = 8 columns x 4 blocks per bank group) meets every bank once
constexpr int TILE_PITCH = STRIP_W + 4, TILE_PLANE = 16 * TILE_PITCH;     // the 8-bit input tile, rows one bank apart
constexpr int CCOLS = STRIP_MCUS + 2, CBLOCKS = 3 * CCOLS;                // decode: chroma blocks of one component around a strip
constexpr int DBLOCKS = 4 * STRIP_MCUS + 2 * CBLOCKS;                     // 32 Y + 60 chroma
constexpr int CPLANE_PITCH = 8 * CCOLS + 4, CPLANE = 24 * CPLANE_PITCH;
constexpr int COEF_PITCH = 33;                            // words per block of a chunk's coefficients in LDS (32 + 1: lanes = blocks)
constexpr int EWORDS = (ET * JBLOCK_BITS + 7 + 31) / 32 + 1;              // a chunk's bits behind up to 7 carried ones
static_assert(6ll * (SC2_JPEG_IMAGE_MAX_SIDE / 16) * (SC2_JPEG_IMAGE_MAX_SIDE / 16) * JBLOCK_BITS < 0x7FFFFFFFll, "bit and byte offsets fit int32");
static_assert(ET >= 64 && (ET & (ET - 1)) == 0, "the prefix sum runs over a power of two of lanes");

struct ImageArgs {
    const uint8_t *x;
    long long sb, sc, sh, sw;
    uint8_t *recon;
    int32_t *sizes;
    uint8_t *bytes;
    long long slot;
    short *coef;                 // [B][n_scan][64], natural order inside a block
    int C, H, W, quality;
    int rows, chunks, n_scan;    // strips per image, column chunks per strip, scan blocks per image
};

struct Geometry {
    int wb, hb, mx, my, ch, cw;
    __device__ __forceinline__ Geometry(int H, int W)
        : wb((W + 7) >> 3), hb((H + 7) >> 3), mx((W + 15) >> 4), my((H + 15) >> 4), ch((H + 1) >> 1), cw((W + 1) >> 1) {}
};

// an Annex K table entry `base` scaled to `quality`, clamped to 1..255 (baseline)
__device__ __forceinline__ uint16_t jpeg_quant_entry(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base * s + 50) / 100;
    return (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
}

// quantised coefficient of a column-pass output d with table entry q
__device__ __forceinline__ int jpeg_quantise(int d, int q) {
    const int div = 8 * q;
    const int mag = ((d < 0 ? -d : d) + (div >> 1)) / div;
    return d < 0 ? -mag : mag;
}

// colour conversion, 16-bit fixed point
__device__ __forceinline__ int jpeg_luma(int R, int G, int B) { return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16; }
__device__ __forceinline__ int jpeg_cb(int R, int G, int B) { return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int jpeg_cr(int R, int G, int B) { return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ void jpeg_ycc_to_rgb(int Y, int cb, int cr, int &R, int &G, int &B) {      // cb, cr minus 128
    R = clamp255(Y + ((91881 * cr + 32768) >> 16));
    G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    B = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

__device__ __forceinline__ void strip_of(const ImageArgs &a, int &img, int &row, int &chunk) {
    const int bid = blockIdx.x;
    chunk = bid % a.chunks;
    const int t = bid / a.chunks;
    row = t % a.rows;
    img = t / a.rows;
}

// ------------------------------------------------------------------------------------------------------------------ transform
__global__ __launch_bounds__(IT) void jpeg_image_transform_kernel(const ImageArgs a) {
    __shared__ int ws[TBLOCKS * WS_PITCH];           // 13.5 KB: level-shifted samples, DCT rows, then the quantised coefficients
    __shared__ uint8_t tile[3 * TILE_PLANE];         // 6.2 KB: the strip's pixels, replicated beyond the image's edges
    __shared__ uint16_t qt[2][64];

    const int tid = threadIdx.x;
    int img, row, chunk;
    strip_of(a, img, row, chunk);
    const int H = a.H, W = a.W;
    const bool rgb = a.C == 3;
    const Geometry g(H, W);
    const int unit0 = chunk * (rgb ? STRIP_MCUS : STRIP_GREY);                                  // first MCU / grey block of the chunk
    const int units = min(rgb ? STRIP_MCUS : STRIP_GREY, (rgb ? g.mx : g.wb) - unit0);
    const int nblk = rgb ? 6 * units : units;
    const int rows_t = rgb ? 16 : 8;
    const int y_org = rows_t * row, x_org = STRIP_W * chunk;

    if (tid < 128) qt[tid >> 6][tid & 63] = jpeg_quant_entry(k_jpeg_tables.base_q[tid >> 6][tid & 63], a.quality);

    {   // the tile: consecutive lanes along the input's unit stride (planes, or interleaved channels)
        const uint8_t *src = a.x + (long long)img * a.sb;
        const int n = (rgb ? 3 : 1) * rows_t * STRIP_W;
        const bool interleaved = rgb && a.sc == 1;
        for (int i = tid; i < n; i += IT) {
            int c, r, xx;
            if (interleaved) {
                c = i % 3;
                xx = (i / 3) & (STRIP_W - 1);
                r = i / (3 * STRIP_W);
            } else {
                xx = i & (STRIP_W - 1);
                r = (i / STRIP_W) % rows_t;
                c = i / (STRIP_W * rows_t);
            }
            const int y = min(y_org + r, H - 1), x = min(x_org + xx, W - 1);
            tile[c * TILE_PLANE + r * TILE_PITCH + xx] = src[c * a.sc + y * a.sh + x * a.sw];
        }
    }
    __syncthreads();

    // ---- level-shifted samples of every block: luma / grey edge-replicated (the tile is), chroma through the 2 x 2 box filter
    for (int e = tid; e < nblk * 64; e += IT) {
        const int blk = e >> 6, r = (e >> 3) & 7, c = e & 7;
        int v;
        if (!rgb) {
            v = tile[r * TILE_PITCH + 8 * blk + c];
        } else {
            const int j = blk / 6, k = blk - 6 * j;
            if (k < 4) {
                const int at = (8 * (k >> 1) + r) * TILE_PITCH + 16 * j + 8 * (k & 1) + c;
                v = jpeg_luma(tile[at], tile[TILE_PLANE + at], tile[2 * TILE_PLANE + at]);
            } else {
                // chroma row min(8 row + r, ch - 1) lies in this strip: its two pixel rows are tile rows 2 (cy - 8 row) and the next
                const int cy = min(8 * row + r, g.ch - 1) - 8 * row;
                int sum = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int at = (2 * cy + (q >> 1)) * TILE_PITCH + 16 * j + 2 * c + (q & 1);
                    const int R = tile[at], G = tile[TILE_PLANE + at], Bv = tile[2 * TILE_PLANE + at];
                    sum += k == 5 ? jpeg_cr(R, G, Bv) : jpeg_cb(R, G, Bv);
                }
                v = (sum + 1 + (c & 1)) >> 2;      // (the chroma column 8 (unit0 + j) + c has c's parity)
            }
        }
        ws[blk * WS_PITCH + 8 * r + c] = v - 128;
    }
    __syncthreads();

    // ---- forward DCT: rows, then columns + quantisation, in place
    for (int t = tid; t < nblk * 8; t += IT) {
        int *p = ws + (t >> 3) * WS_PITCH + 8 * (t & 7);
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = p[i];
        fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = d[i];
    }
    __syncthreads();
    for (int t = tid; t < nblk * 8; t += IT) {
        const int blk = t >> 3, c = t & 7;
        const uint16_t *q = qt[rgb && (blk % 6) >= 4];
        int *p = ws + blk * WS_PITCH + c;
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = p[8 * i];
        fdct8<false>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[8 * i] = jpeg_quantise(d[i], q[8 * i + c]);
    }
    __syncthreads();

    // ---- to the workspace: the chunk's blocks are consecutive in scan order; two coefficients per word
    const long long s0 = rgb ? 6ll * ((long long)row * g.mx + unit0) : (long long)row * g.wb + unit0;
    uint32_t *dst = reinterpret_cast<uint32_t *>(a.coef + ((long long)img * a.n_scan + s0) * 64);
    for (int w = tid; w < nblk * 32; w += IT) {
        const int blk = w >> 5, i = 2 * (w & 31);
        int from = blk;
        bool real = true;
        if (rgb) {
            const int j = blk / 6;
            int k = blk - 6 * j;
            if (k < 4) {
                // a Y block beyond the block grid carries the DC of the block before it in the MCU (block 0 is real) and no AC
                for (;; --k) {
                    const int by = 2 * row + (k >> 1), bx = 2 * (unit0 + j) + (k & 1);
                    if ((by < g.hb && bx < g.wb) || k == 0) break;
                    real = false;
                }
                from = 6 * j + k;
            }
        }
        const int *p = ws + from * WS_PITCH;
        const int lo = real ? p[i] : (i == 0 ? p[0] : 0), hi = real ? p[i + 1] : 0;
        dst[w] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
    }
}

// ------------------------------------------------------------------------------------------------------------------ entropy
// code_block of jpeg_common.h on a block held in ZIGZAG order with the bit mask of its non-zero coefficients: the same symbols, but
// only the non-zero coefficients are visited (a run is the gap between two set bits), which is most of a lane's time in this kernel.
template <typename Sink>
__device__ __forceinline__ void code_block_sparse(Sink &s, const short *zz, unsigned long long nonzero, int diff, const uint32_t *dc,
                                                  const uint32_t *ac) {
    const int nd = magnitude_bits(diff);
    put_value(s, dc[nd], diff, nd);
    int before = 0;
    for (unsigned long long m = nonzero & ~1ull; m; m &= m - 1) {
        const int k = __ffsll((long long)m) - 1;
        int run = k - before - 1;
        before = k;
        while (run > 15) {
            s.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
            run -= 16;
        }
        const int v = zz[k];
        const int n = magnitude_bits(v);
        put_value(s, ac[(run << 4) + n], v, n);
    }
    if (before != 63) s.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

__global__ __launch_bounds__(ET) void jpeg_image_entropy_kernel(const ImageArgs a) {
    __shared__ uint32_t bits[EWORDS];                // 26 KB: the chunk's bits, behind the carried bits of the byte before them
    __shared__ uint32_t coefw[ET * COEF_PITCH];      // 16.5 KB: the chunk's coefficients in zigzag order, one block per lane
    __shared__ JpegTables tab;
    __shared__ uint8_t unzig[64];                    // position in the zigzag sequence of a coefficient in natural order
    __shared__ int scan[ET];

    const int tid = threadIdx.x;
    const int img = blockIdx.x;
    const bool rgb = a.C == 3;
    const int n_scan = a.n_scan;
    const short *src = a.coef + (long long)img * n_scan * 64;
    uint8_t *out = a.bytes ? a.bytes + (long long)img * a.slot : nullptr;
    jpeg_copy_tables(&tab, tid, ET);
    if (tid < 64) unzig[k_jpeg_tables.zigzag[tid]] = (uint8_t)tid;
    __syncthreads();

    int carry_n = 0;             // bits of the last, partial byte of the chunks so far ...
    uint32_t carry = 0;          // ... as that byte's value (the bits on top)
    int out_pos = 0;             // bytes of the segment written so far, stuffing included

    for (int c0 = 0; c0 < n_scan; c0 += ET) {
        const int n = min(ET, n_scan - c0);
        const bool last = c0 + ET >= n_scan;
        const uint32_t *from = reinterpret_cast<const uint32_t *>(src + (long long)c0 * 64);
        short *staged = reinterpret_cast<short *>(coefw);
        for (int w = tid; w < n * 32; w += ET) {     // consecutive lanes read consecutive words; each coefficient goes to its zigzag place
            const uint32_t pair = from[w];
            short *blk = staged + (w >> 5) * (2 * COEF_PITCH);
            blk[unzig[2 * (w & 31)]] = (short)(pair & 0xFFFFu);
            blk[unzig[2 * (w & 31) + 1]] = (short)(pair >> 16);
        }
        __syncthreads();

        // one lane per block: lengths first, a prefix sum for the bit offsets, then the bits
        const short *c = staged + tid * (2 * COEF_PITCH);
        int diff = 0, table = 0, my_bits = 0;
        unsigned long long nonzero = 0;
        if (tid < n) {
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const uint32_t pair = coefw[tid * COEF_PITCH + j];
                nonzero |= (unsigned long long)((pair & 0xFFFFu) != 0) << (2 * j) | (unsigned long long)((pair >> 16) != 0) << (2 * j + 1);
            }
            const int s = c0 + tid;
            int before = s - 1;                   // the block before it of its component, in scan order
            if (rgb) {
                const int k = s % 6;
                table = k >= 4;
                before = k == 0 ? s - 3 : (k < 4 ? s - 1 : s - 6);
            }
            // (its DC: in the chunk's staged blocks, or -- for the chunk's first blocks -- in the workspace)
            diff = c[0] - (before >= c0 ? staged[(before - c0) * (2 * COEF_PITCH)] : (before >= 0 ? src[(long long)before * 64] : 0));
            CountBits cnt = {0};
            code_block_sparse(cnt, c, nonzero, diff, tab.dc[table], tab.ac[table]);
            my_bits = cnt.n;
        }
        int total_bits;
        const int bit_at = carry_n + block_scan<ET>(my_bits, scan, tid, total_bits);
        const int all_bits = carry_n + total_bits;
        const int n_words = min(((all_bits + 31) >> 5) + 1, EWORDS);
        for (int i = tid; i < n_words; i += ET) bits[i] = i == 0 ? carry << 24 : 0u;
        __syncthreads();
        if (tid < n) {
            EmitBits<EWORDS> em = {bits, 0ull, bit_at >> 5, bit_at & 31};
            code_block_sparse(em, c, nonzero, diff, tab.dc[table], tab.ac[table]);
            em.finish();
        }
        if (last && tid == ET - 1 && (all_bits & 7)) {     // the segment's last byte is filled up with 1 bits (they lie inside one word)
            const int pad = 8 - (all_bits & 7);
            const int word = all_bits >> 5;
            if (word < EWORDS) atomicOr(&bits[word], ((1u << pad) - 1u) << (32 - (all_bits & 31) - pad));
        }
        __syncthreads();

        // ---- the chunk's whole bytes; a zero byte follows every 0xFF: count them per lane's run of bytes, prefix sum, place
        const int n_bytes = last ? (all_bits + 7) >> 3 : all_bits >> 3;
        const int per_lane = (n_bytes + ET - 1) / ET;
        const int b0 = min(tid * per_lane, n_bytes), b1 = min(b0 + per_lane, n_bytes);
        int ff = 0;
        for (int b = b0; b < b1; ++b) ff += ((bits[b >> 2] >> (24 - 8 * (b & 3))) & 0xFFu) == 0xFFu;
        int total_ff;
        const int ff_before = block_scan<ET>(ff, scan, tid, total_ff);
        if (out) {
            long long o = (long long)out_pos + b0 + ff_before;
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
        // the carry of the next chunk: the bits behind the last whole byte (the words up to there were cleared above)
        carry_n = last ? 0 : all_bits & 7;
        carry = (n_bytes >> 2) < EWORDS ? (bits[n_bytes >> 2] >> (24 - 8 * (n_bytes & 3))) & 0xFFu : 0u;
        out_pos += n_bytes + total_ff;
        __syncthreads();         // the two work areas change hands
    }
    if (tid == 0) a.sizes[img] = (rgb ? SC2_JPEG_HEADER_RGB : SC2_JPEG_HEADER_GREY) + out_pos + 2;     // header, segment, EOI
}

// ------------------------------------------------------------------------------------------------------------------ decode
__global__ __launch_bounds__(IT) void jpeg_image_decode_kernel(const ImageArgs a) {
    __shared__ int ws[DBLOCKS * WS_PITCH];           // 26 KB: dequantised coefficients, IDCT columns
    __shared__ uint8_t ypl[16 * STRIP_W];            // the strip's decoded luma (grey: 8 rows of it)
    __shared__ uint8_t cpl[2 * CPLANE];              // Cb, Cr: three MCU rows x ten MCU columns around the strip, 24 x 80 samples each
    __shared__ int blk_s[DBLOCKS];                   // scan index of every block slot, -1: not needed / outside the image
    __shared__ uint16_t qt[2][64];

    const int tid = threadIdx.x;
    int img, row, chunk;
    strip_of(a, img, row, chunk);
    const int H = a.H, W = a.W;
    const bool rgb = a.C == 3;
    const Geometry g(H, W);
    const int unit0 = chunk * (rgb ? STRIP_MCUS : STRIP_GREY);
    const int nb = rgb ? DBLOCKS : STRIP_GREY;
    const int rows_t = rgb ? 16 : 8;
    const int y_org = rows_t * row, x_org = STRIP_W * chunk;
    const short *src = a.coef + (long long)img * a.n_scan * 64;

    if (tid < 128) qt[tid >> 6][tid & 63] = jpeg_quant_entry(k_jpeg_tables.base_q[tid >> 6][tid & 63], a.quality);
    if (tid < nb) {
        int s = -1;
        if (!rgb) {
            if (unit0 + tid < g.wb) s = row * g.wb + unit0 + tid;
        } else if (tid < 4 * STRIP_MCUS) {
            const int j = tid >> 2, k = tid & 3, m_x = unit0 + j;
            if (m_x < g.mx && 2 * row + (k >> 1) < g.hb && 2 * m_x + (k & 1) < g.wb) s = 6 * (row * g.mx + m_x) + k;
        } else {
            const int u = tid - 4 * STRIP_MCUS;
            const int comp = u / CBLOCKS, v = u - comp * CBLOCKS;
            const int m_y = row - 1 + v / CCOLS, m_x = unit0 - 1 + v % CCOLS;
            if (m_y >= 0 && m_y < g.my && m_x >= 0 && m_x < g.mx) s = 6 * (m_y * g.mx + m_x) + 4 + comp;
        }
        blk_s[tid] = s;
    }
    __syncthreads();

    // ---- dequantise, inverse DCT columns, then rows into the 8-bit planes
    for (int e = tid; e < nb * 64; e += IT) {
        const int blk = e >> 6, i = e & 63;
        const int s = blk_s[blk];
        if (s < 0) continue;
        ws[blk * WS_PITCH + i] = src[(long long)s * 64 + i] * qt[rgb && blk >= 4 * STRIP_MCUS][i];
    }
    __syncthreads();
    for (int t = tid; t < nb * 8; t += IT) {
        const int blk = t >> 3, c = t & 7;
        if (blk_s[blk] < 0) continue;
        int *p = ws + blk * WS_PITCH + c;
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[8 * i];
        idct8<11>(v);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[8 * i] = v[i];
    }
    __syncthreads();
    for (int t = tid; t < nb * 8; t += IT) {
        const int blk = t >> 3, r = t & 7;
        if (blk_s[blk] < 0) continue;
        const int *p = ws + blk * WS_PITCH + 8 * r;
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i];
        idct8<18>(v);
        uint8_t *to;
        if (!rgb) {
            to = ypl + r * STRIP_W + 8 * blk;
        } else if (blk < 4 * STRIP_MCUS) {
            const int j = blk >> 2, k = blk & 3;
            to = ypl + (8 * (k >> 1) + r) * STRIP_W + 16 * j + 8 * (k & 1);
        } else {
            const int u = blk - 4 * STRIP_MCUS;
            const int comp = u / CBLOCKS, w = u - comp * CBLOCKS;
            to = cpl + comp * CPLANE + (8 * (w / CCOLS) + r) * CPLANE_PITCH + 8 * (w % CCOLS);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) to[i] = (uint8_t)clamp255(v[i] + 128);
    }
    __syncthreads();

    // ---- pixels: chroma up, colour conversion.  Chroma sample (cy, cx) of the image sits at (cy - 8 row + 8, cx - 8 unit0 + 8) of `cpl`.
    uint8_t *dst = a.recon + (long long)img * a.C * H * W;
    const long long HW = (long long)H * W;
    for (int i = tid; i < rows_t * STRIP_W; i += IT) {
        const int ly = i / STRIP_W, lx = i & (STRIP_W - 1);
        const int y = y_org + ly, x = x_org + lx;
        if (y >= H || x >= W) continue;
        const int Y = ypl[i];
        const long long at = (long long)y * W + x;
        if (!rgb) {
            dst[at] = (uint8_t)Y;
            continue;
        }
        const int cy = y >> 1, cx = x >> 1;
        const int ny = cy - 8 * row + 8, lcx = cx - 8 * unit0 + 8;
        int cb, cr;
        if (g.cw <= 2) {       // one or two chroma columns: every sample repeated 2 x 2
            cb = cpl[ny * CPLANE_PITCH + lcx];
            cr = cpl[CPLANE + ny * CPLANE_PITCH + lcx];
        } else {               // the triangle filter; the row beyond an edge of the real plane equals the edge row
            const int fy = ((y & 1) ? min(cy + 1, g.ch - 1) : max(cy - 1, 0)) - 8 * row + 8;
            const uint8_t *nr = cpl + ny * CPLANE_PITCH, *fr = cpl + fy * CPLANE_PITCH;
            cb = chroma_taps(nr, fr, lcx, cx == 0, cx == g.cw - 1, x & 1);
            cr = chroma_taps(nr + CPLANE, fr + CPLANE, lcx, cx == 0, cx == g.cw - 1, x & 1);
        }
        int R, G, Bv;
        jpeg_ycc_to_rgb(Y, cb - 128, cr - 128, R, G, Bv);
        dst[at] = (uint8_t)R;
        dst[HW + at] = (uint8_t)G;
        dst[2 * HW + at] = (uint8_t)Bv;
    }
}

bool image_dims_ok(int C, int H, int W) {
    return (C == 1 || C == 3) && H >= 1 && W >= 1 && H <= SC2_JPEG_IMAGE_MAX_SIDE && W <= SC2_JPEG_IMAGE_MAX_SIDE;
}

long long image_scan_blocks(int C, int H, int W) {
    return C == 3 ? 6ll * ((H + 15) / 16) * ((W + 15) / 16) : (long long)((H + 7) / 8) * ((W + 7) / 8);
}

}  // namespace

extern "C" long long sc2_jpeg_image_max_bytes(int C, int H, int W) {
    if (!image_dims_ok(C, H, W)) return -1;
    return 2 * ((image_scan_blocks(C, H, W) * JBLOCK_BITS + 7) / 8);
}

extern "C" long long sc2_jpeg_image_workspace_bytes(int B, int C, int H, int W) {
    if (B < 1 || !image_dims_ok(C, H, W)) return -1;
    return (long long)B * image_scan_blocks(C, H, W) * 64 * (long long)sizeof(short);
}

extern "C" int sc2_jpeg_image_codec(const uint8_t *x, long long sb, long long sc, long long sh, long long sw, int B, int C, int H, int W,
                                    int quality, uint8_t *recon, int32_t *sizes, uint8_t *bytes, long long slot_bytes, void *workspace,
                                    long long workspace_bytes, void *stream) {
    SC2_REQUIRE(C == 1 || C == 3, SC2_ERR_UNSUPPORTED, "jpeg_image_codec: %d channels (1: grey, 3: RGB)", C);
    SC2_REQUIRE(H >= 1 && W >= 1 && H <= SC2_JPEG_IMAGE_MAX_SIDE && W <= SC2_JPEG_IMAGE_MAX_SIDE, SC2_ERR_UNSUPPORTED,
                "jpeg_image_codec: %dx%d (sides 1..%d)", H, W, SC2_JPEG_IMAGE_MAX_SIDE);
    SC2_REQUIRE(quality >= 1 && quality <= 100, SC2_ERR_UNSUPPORTED, "jpeg_image_codec: quality %d (1..100)", quality);
    SC2_REQUIRE(B > 0, SC2_ERR_INVALID_ARG, "jpeg_image_codec: bad batch size %d", B);
    SC2_REQUIRE(x && recon && sizes && workspace, SC2_ERR_INVALID_ARG, "jpeg_image_codec: null pointer");
    SC2_REQUIRE(sb >= 0 && sc >= 0 && sh >= 0 && sw >= 0, SC2_ERR_INVALID_ARG, "jpeg_image_codec: negative stride");
    SC2_REQUIRE(((reinterpret_cast<uintptr_t>(sizes) | reinterpret_cast<uintptr_t>(workspace)) & 3u) == 0, SC2_ERR_INVALID_ARG,
                "jpeg_image_codec: misaligned pointer");
    const long long need_ws = sc2_jpeg_image_workspace_bytes(B, C, H, W);
    SC2_REQUIRE(workspace_bytes >= need_ws, SC2_ERR_INVALID_ARG, "jpeg_image_codec: workspace of %lld bytes (at least %lld)", workspace_bytes, need_ws);
    if (bytes) {
        const long long need = sc2_jpeg_image_max_bytes(C, H, W);
        SC2_REQUIRE(slot_bytes >= need, SC2_ERR_INVALID_ARG, "jpeg_image_codec: byte slots of %lld (at least %lld)", slot_bytes, need);
    }
    ImageArgs a;
    a.x = x;
    a.sb = sb; a.sc = sc; a.sh = sh; a.sw = sw;
    a.recon = recon;
    a.sizes = sizes;
    a.bytes = bytes;
    a.slot = bytes ? slot_bytes : 0;
    a.coef = static_cast<short *>(workspace);
    a.C = C; a.H = H; a.W = W; a.quality = quality;
    a.rows = C == 3 ? (H + 15) / 16 : (H + 7) / 8;
    a.chunks = (W + STRIP_W - 1) / STRIP_W;
    a.n_scan = (int)image_scan_blocks(C, H, W);
    const long long strips = (long long)B * a.rows * a.chunks;
    SC2_REQUIRE(strips <= 0x7FFFFFFFll, SC2_ERR_UNSUPPORTED, "jpeg_image_codec: %lld strips in one call", strips);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(jpeg_image_transform_kernel, dim3((unsigned)strips), dim3(IT), 0, s, a);
    SC2_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_image_entropy_kernel, dim3((unsigned)B), dim3(ET), 0, s, a);
    SC2_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_image_decode_kernel, dim3((unsigned)strips), dim3(IT), 0, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
