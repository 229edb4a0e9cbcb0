// Serial context-model scan of the joint autoregressive hierarchical prior (CompressAI's
// `JointAutoregressiveHierarchicalPriors._compress_ar` / `_decompress_ar`, the `mbt2018` zoo model) for gfx950.
//
// Each latent pixel depends on the y_hat of the pixels before it in raster order, so the scan is H x W dependent steps.
// The parallel axis is the batch: ONE WORKGROUP OWNS ONE IMAGE for the whole range of pixels it is given and walks them in
// order, synchronising only within itself -- no grid-wide barrier and no in-kernel wait on other workgroups.  A step is four
// GEMVs (context taps 12M -> 2M, the context half of entropy_parameters' first layer, its second and third layers), the
// Gaussian index search, and either the quantisation of y (encoder) or M serial rANS decodes (decoder), then the write of
// y_hat into the padded map the next steps gather from.  Encoder and decoder run the same step code; they differ only in
// where the symbol comes from.
//
// Determinism and batch invariance: every output of every GEMV is the same fixed sum -- kSplit contiguous k ranges, each
// accumulated in k order with fmaf, added in range order, then the bias / precomputed term -- whatever B is and wherever the
// image sits in the batch.  The hyper-params half of layer 1 (W1[:, :2M] . params + b1) is one GEMM over all pixels before the
// scan (p1), added here after the context half, in both directions.
//
// Decoder: CompressAI's RansDecoder.decode_stream semantics (64-bit state, 32-bit words, 16-bit precision, 4-bit bypass
// escapes), the search over the CDF row as an upper bound (identical in result to upstream's linear find_if over a strictly
// increasing row).  The Gaussian table's rows are packed into LDS as u16 (the closing 65536 is implied by the row's end).
// A table too long for LDS beside the step's vectors (a scale table reaching into the thousands) is searched in device memory.
// State and read position are loaded from / stored to device memory at the ends of the pixel range: a scan may be split.
// No word outside a stream's bytes is ever read (zeros are supplied past its end and the stream is flagged).
//
// Two weight forms, one step: sc2_ar_scan reads the four matrices as bf16, sc2_ar_scan_f32 as f32 (same k-major shapes, same zero
// padding).  The kernel is a template on the weight type; only the load of a weight pair differs, so the f32 form is as
// deterministic and batch invariant, and its encoder and decoder run the same step code too.
#include <math.h>

#include "gfx950_prims.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSplit = 4;          // fixed k ranges per GEMV output
constexpr int kTaps = 12;          // 5x5 mask type A: two full rows above and two pixels to the left
constexpr int kPrecision = 16;
constexpr int kBypassPrecision = 4;
constexpr int kMaxBypassVal = (1 << kBypassPrecision) - 1;
constexpr unsigned long long kRansL = 1ull << 31;
constexpr int kStatusIndex = 4;    // a CDF-row index outside the table (the resumable decoder's explicit indexes)
constexpr int kStatusCorrupt = 8;  // as rans.hip
constexpr int kStatusTail = 16;
constexpr int kMaxEscapeNibbles = 8;
constexpr int kMaxWidth = 1280;

struct ArDec {
    unsigned long long x;
    int pos;             // next word to read
    int n_words;
    int corrupt;
    const uint32_t *w;
};

__device__ __forceinline__ void ar_dec_renorm(ArDec &d) {
    if (d.x < kRansL) {
        const uint32_t v = d.pos < d.n_words ? d.w[d.pos] : 0u;
        d.x = (d.x << 32) | v;
        d.pos += 1;
    }
}

__device__ __forceinline__ unsigned ar_dec_get_bits(ArDec &d) {
    const unsigned val = (unsigned)(d.x & kMaxBypassVal);
    d.x >>= kBypassPrecision;
    ar_dec_renorm(d);
    return val;
}

// The stream of image / stream `s`: its words, clamped to its row.
__device__ __forceinline__ void ar_dec_bind(ArDec &d, const uint8_t *buf, long long stride, const int32_t *io_offset,
                                            const int32_t *io_nbytes, int s) {
    const long long off = io_offset[s];
    long long nb = io_nbytes[s];
    int bad = 0;
    if (off < 0 || (off & 3) || off > stride) { nb = 0; bad = 1; }
    if (nb < 0) { nb = 0; bad = 1; }
    if (!bad && off + nb > stride) { nb = stride - off; bad = 1; }
    d.w = reinterpret_cast<const uint32_t *>(buf + (long long)s * stride + (bad && off > stride ? 0 : off));
    d.n_words = (int)(nb / 4);
    d.corrupt = bad ? kStatusCorrupt : 0;
}

__device__ __forceinline__ void ar_dec_start(ArDec &d) {
    const uint32_t w0 = d.n_words > 0 ? d.w[0] : 0u, w1 = d.n_words > 1 ? d.w[1] : 0u;
    d.x = (unsigned long long)w0 | ((unsigned long long)w1 << 32);
    d.pos = 2;
}

// One symbol with CDF row `idx`; `entry(j)` is the row's j-th cumulative frequency (j < size - 1; entry size - 1 = 65536).
template <class Entry>
__device__ __forceinline__ int ar_dec_symbol(ArDec &d, int size, int offset, Entry &&entry) {
    const int max_value = size - 2;
    const unsigned cum_freq = (unsigned)(d.x & 0xFFFFu);
    int lo = 0, hi = size;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const unsigned v = mid >= size - 1 ? 65536u : entry(mid);
        if (v > cum_freq) hi = mid; else lo = mid + 1;
    }
    int sidx = lo - 1;
    if (sidx < 0) { sidx = 0; d.corrupt |= kStatusCorrupt; }   // entry(0) != 0: not a table the encoder could have used
    const unsigned start = entry(sidx);
    const unsigned end = sidx + 1 >= size - 1 ? 65536u : entry(sidx + 1);
    const unsigned freq = end - start;
    d.x = (unsigned long long)freq * (d.x >> kPrecision) + cum_freq - start;
    ar_dec_renorm(d);
    int value = sidx;
    if (value == max_value) {
        const int n_bypass = (int)ar_dec_get_bits(d);
        if (n_bypass > kMaxEscapeNibbles) {
            d.corrupt |= kStatusCorrupt;
        } else {
            unsigned raw = 0;
            for (int j = 0; j < n_bypass; ++j) raw |= ar_dec_get_bits(d) << (j * kBypassPrecision);
            const int raw_val = (int)raw;
            value = (int)(raw >> 1);
            if (raw_val & 1) value = -value - 1;
            else value += max_value;
        }
    }
    return value + offset;
}

__device__ __forceinline__ int ar_dec_status(const ArDec &d, bool last) {
    int st = d.corrupt | (d.pos > d.n_words ? kStatusCorrupt : 0);
    if (last && (d.x != kRansL || d.pos != d.n_words)) st |= kStatusTail;
    return st;
}

using namespace sc2prim;   // gfx950_prims.h: bf_lo / bf_hi

// The two weight forms.  A lane loads the weights of two adjacent outputs as ONE value: a 4-byte pair of bf16 (Wt = uint16_t) or
// an 8-byte pair of f32 (Wt = float; N is even, so every row starts on an 8-byte boundary of an 8-byte aligned matrix).
template <class Wt> struct ArPair;
template <> struct ArPair<uint16_t> {
    using type = uint32_t;
    static __device__ __forceinline__ float lo(uint32_t w) { return bf_lo(w); }
    static __device__ __forceinline__ float hi(uint32_t w) { return bf_hi(w); }
};
template <> struct ArPair<float> {
    using type = float2;
    static __device__ __forceinline__ float lo(const float2 &w) { return w.x; }
    static __device__ __forceinline__ float hi(const float2 &w) { return w.y; }
};

// out[n] = act(sum_k in[k] W[k][n] (+ bias[n]) (+ add[n])), N even, W k-major bf16 or f32 with row length N.  `in` and `out` in
// LDS, `part` = kSplit * N floats of LDS.  Ends with a barrier: `out` is visible to the whole workgroup.
template <class Wt>
__device__ void ar_gemv(const float *in, int K, const Wt *__restrict__ W, int N, const float *__restrict__ bias,
                        const float *__restrict__ add, bool leaky, float *out, float *part) {
    using Pair = ArPair<Wt>;
    using pair_t = typename Pair::type;
    const int P = N >> 1;
    const int kc = (K + kSplit - 1) / kSplit;
    const pair_t *W2 = reinterpret_cast<const pair_t *>(W);
    for (int u = threadIdx.x; u < P * kSplit; u += kThreads) {
        const int s = u / P, p = u - s * P;
        const int k0 = s * kc, k1 = min(K, k0 + kc);
        float a0 = 0.f, a1 = 0.f;
        const pair_t *wp = W2 + (long long)k0 * P + p;
        int k = k0;
        if (sizeof(Wt) == 4) {
            // f32 weights: the eight 8-byte loads of a block are issued before its first fmaf (left to itself the compiler waited
            // for every load of the encoder's loop before issuing the next: one load in flight, 5 x the step time).  Same sums, same order.
            for (; k + 8 <= k1; k += 8) {
                pair_t w[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = wp[(long long)j * P];
                wp += 8LL * P;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float xv = in[k + j];
                    a0 = fmaf(xv, Pair::lo(w[j]), a0);
                    a1 = fmaf(xv, Pair::hi(w[j]), a1);
                }
            }
        }
#pragma unroll 8
        for (; k < k1; ++k) {
            const pair_t w = *wp;
            wp += P;
            const float xv = in[k];
            a0 = fmaf(xv, Pair::lo(w), a0);
            a1 = fmaf(xv, Pair::hi(w), a1);
        }
        part[s * N + 2 * p] = a0;
        part[s * N + 2 * p + 1] = a1;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += kThreads) {
        float v = part[n];
#pragma unroll
        for (int s = 1; s < kSplit; ++s) v += part[s * N + n];
        if (bias) v += bias[n];
        if (add) v += add[n];
        if (leaky) v = v < 0.f ? 0.01f * v : v;
        out[n] = v;
    }
    __syncthreads();
}

struct LdsLayout {
    int xin, ctx, h1, h2, gp, part, idx, sym, tab, rows, cdf, total_words;
};

__host__ __device__ inline LdsLayout ar_lds_layout(int M, int C1p, int C2p, int n_table, int n_cdfs, long long cdf_entries,
                                                   int decode) {
    LdsLayout L;
    int o = 0;
    const int C0 = 2 * M;
    int wmax = C0 > C1p ? C0 : C1p;
    wmax = wmax > C2p ? wmax : C2p;
    L.xin = o; o += kTaps * M;
    L.ctx = o; o += C0;
    L.h1 = o; o += C1p;
    L.h2 = o; o += C2p;
    L.gp = o; o += C0;
    L.part = o; o += kSplit * wmax;
    L.idx = o; o += M;
    L.sym = o; o += M;
    L.tab = o; o += n_table;
    L.rows = o; o += decode ? 3 * n_cdfs : 0;                    // row start, size, offset
    L.cdf = o; o += decode ? (int)((cdf_entries + 1) / 2) : 0;   // u16 entries
    L.total_words = o;
    return L;
}

// CDF_LDS: the decoder's CDF rows are packed into LDS (otherwise each search reads a.cdfs in device memory).
// Wt: the type of the four weight matrices, uint16_t (bf16 bits) or float; everything but the weight load is the same code.
template <bool DECODE, bool CDF_LDS, class Wt = uint16_t>
__global__ __launch_bounds__(kThreads) void ar_scan_kernel(const sc2_ar_scan_args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x;
    const int M = a.M, C0 = 2 * M, H = a.H, W = a.W;
    const LdsLayout L = ar_lds_layout(M, a.C1p, a.C2p, a.n_table, a.n_cdfs, 0, 0);
    float *xin = lds + L.xin, *ctx = lds + L.ctx, *h1 = lds + L.h1, *h2 = lds + L.h2, *gp = lds + L.gp, *part = lds + L.part;
    int *s_idx = reinterpret_cast<int *>(lds + L.idx);
    int *s_sym = reinterpret_cast<int *>(lds + L.sym);
    float *tab = lds + L.tab;
    int *rows = reinterpret_cast<int *>(lds + L.tab + a.n_table);
    uint16_t *cdf16 = reinterpret_cast<uint16_t *>(rows + 3 * a.n_cdfs);
    for (int t = threadIdx.x; t < a.n_table; t += kThreads) tab[t] = a.scale_table[t];
    if (DECODE) {
        if (threadIdx.x == 0) {
            int o = 0;
            for (int r = 0; r < a.n_cdfs; ++r) {
                rows[r] = o;
                rows[a.n_cdfs + r] = a.cdf_sizes[r];
                rows[2 * a.n_cdfs + r] = a.offsets[r];
                o += a.cdf_sizes[r] - 1;
            }
        }
        __syncthreads();
        if (CDF_LDS) {
            for (int r = 0; r < a.n_cdfs; ++r) {
                const int n = a.cdf_sizes[r] - 1, o = rows[r];
                for (int j = threadIdx.x; j < n; j += kThreads) cdf16[o + j] = (uint16_t)a.cdfs[(long long)r * a.cdf_stride + j];
            }
        }
    }
    ArDec d;
    if (DECODE && threadIdx.x == 0) {
        ar_dec_bind(d, a.buf, a.stride, a.io_offset, a.io_nbytes, b);
        if (a.pix0 == 0) {
            ar_dec_start(d);
        } else {
            d.x = a.st_x[b];
            d.pos = a.st_pos[b];
            d.corrupt |= a.status[b] & kStatusCorrupt;
        }
    }
    __syncthreads();

    const int PW = W + 4;
    float *yp = a.y_hat_pad + (long long)b * (H + 2) * PW * M;
    const Wt *wc = static_cast<const Wt *>(a.wc);
    const Wt *w1 = static_cast<const Wt *>(a.w1);
    const Wt *w2 = static_cast<const Wt *>(a.w2);
    const Wt *w3 = static_cast<const Wt *>(a.w3);
    const float *bc = static_cast<const float *>(a.bc), *b2 = static_cast<const float *>(a.b2),
                *b3 = static_cast<const float *>(a.b3), *p1 = static_cast<const float *>(a.p1);
    uint16_t *yo = static_cast<uint16_t *>(a.y_hat_nhwc);
    for (int p = a.pix0; p < a.pix1; ++p) {
        const int h = p / W, w = p - h * W;
        // gather the 12 causal taps (padded coordinates: row h + 2 + dy, column w + 2 + dx)
        for (int i = threadIdx.x; i < kTaps * M; i += kThreads) {
            const int t = i / M, c = i - t * M;
            const int dy = t < 5 ? -2 : (t < 10 ? -1 : 0);
            const int dx = t < 5 ? t - 2 : (t < 10 ? t - 7 : t - 12);
            xin[i] = yp[((long long)(h + 2 + dy) * PW + (w + 2 + dx)) * M + c];
        }
        __syncthreads();
        ar_gemv(xin, kTaps * M, wc, C0, bc, nullptr, false, ctx, part);
        ar_gemv(ctx, C0, w1, a.C1p, nullptr, p1 + ((long long)b * H * W + p) * a.C1p, true, h1, part);
        ar_gemv(h1, a.C1p, w2, a.C2p, b2, nullptr, true, h2, part);
        ar_gemv(h2, a.C2p, w3, C0, b3, nullptr, false, gp, part);
        const long long sbase = ((long long)b * H * W + p) * M;
        if (a.gaussian_params)
            for (int c = threadIdx.x; c < C0; c += kThreads) a.gaussian_params[2 * sbase + c] = gp[c];
        for (int c = threadIdx.x; c < M; c += kThreads) {
            const float s = fmaxf(gp[c], a.scale_bound);
            int idx = a.n_table - 1;
            for (int t = 0; t + 1 < a.n_table; ++t) idx -= (s <= tab[t]) ? 1 : 0;
            s_idx[c] = idx;
            if (!DECODE) {
                const float yv = a.y[(((long long)b * M + c) * H + h) * W + w];
                const int q = (int)rintf(yv - gp[M + c]);
                s_sym[c] = q;
                a.symbols[sbase + c] = q;
                a.indexes[sbase + c] = idx;
            }
        }
        __syncthreads();
        if (DECODE && threadIdx.x == 0) {
            for (int c = 0; c < M; ++c) {
                const int idx = s_idx[c];
                if (CDF_LDS) {
                    const uint16_t *row = cdf16 + rows[idx];
                    s_sym[c] = ar_dec_symbol(d, rows[a.n_cdfs + idx], rows[2 * a.n_cdfs + idx],
                                             [&](int j) { return (unsigned)row[j]; });
                } else {
                    const int32_t *row = a.cdfs + (long long)idx * a.cdf_stride;
                    s_sym[c] = ar_dec_symbol(d, rows[a.n_cdfs + idx], rows[2 * a.n_cdfs + idx],
                                             [&](int j) { return (unsigned)row[j]; });
                }
            }
        }
        __syncthreads();
        float *centre = yp + ((long long)(h + 2) * PW + (w + 2)) * M;
        for (int c = threadIdx.x; c < M; c += kThreads) {
            const float v = (float)s_sym[c] + gp[M + c];
            centre[c] = v;
            if (yo) yo[sbase + c] = f32_to_bf16_bits(v);
            if (DECODE) {
                if (a.symbols) a.symbols[sbase + c] = s_sym[c];
                if (a.indexes) a.indexes[sbase + c] = s_idx[c];
            }
        }
        __threadfence_block();
        __syncthreads();
    }
    if (DECODE && threadIdx.x == 0) {
        a.st_x[b] = d.x;
        a.st_pos[b] = d.pos;
        a.status[b] = ar_dec_status(d, a.pix1 == H * W);
    }
}

__global__ __launch_bounds__(64) void rans_decode_resume_kernel(const uint8_t *buf, long long stride, const int32_t *io_offset,
                                                                const int32_t *io_nbytes, const int32_t *indexes, int n_streams,
                                                                long long n_sym, const int32_t *cdfs, int n_cdfs,
                                                                int cdf_stride, const int32_t *cdf_sizes,
                                                                const int32_t *offsets, int first, int last,
                                                                unsigned long long *st_x, int32_t *st_pos, int32_t *status,
                                                                int32_t *symbols_out) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_streams) return;
    ArDec d;
    ar_dec_bind(d, buf, stride, io_offset, io_nbytes, s);
    if (first) {
        ar_dec_start(d);
    } else {
        d.x = st_x[s];
        d.pos = st_pos[s];
        d.corrupt |= status[s] & (kStatusCorrupt | kStatusIndex);   // what an earlier call flagged stays flagged
    }
    for (long long i = 0; i < n_sym; ++i) {
        int idx = indexes[(long long)s * n_sym + i];
        if (idx < 0 || idx >= n_cdfs) { d.corrupt |= kStatusIndex; idx = 0; }
        const int32_t *row = cdfs + (long long)idx * cdf_stride;
        symbols_out[(long long)s * n_sym + i] = ar_dec_symbol(d, cdf_sizes[idx], offsets[idx],
                                                              [&](int j) { return (unsigned)row[j]; });
    }
    st_x[s] = d.x;
    st_pos[s] = d.pos;
    status[s] = ar_dec_status(d, last != 0);
}

template <class Wt>
int ar_scan_launch(const sc2_ar_scan_args *args, void *stream) {
    SC2_REQUIRE(args, SC2_ERR_INVALID_ARG, "ar_scan: null arguments");
    const sc2_ar_scan_args &a = *args;
    SC2_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && a.M > 0 && a.M <= 512, SC2_ERR_INVALID_ARG, "ar_scan: bad dims");
    SC2_REQUIRE(a.C1p > 0 && a.C2p > 0 && a.C1p % 8 == 0 && a.C2p % 8 == 0 && a.C1p <= kMaxWidth && a.C2p <= kMaxWidth &&
                    2 * a.M <= kMaxWidth,
                SC2_ERR_UNSUPPORTED, "ar_scan: widths C1p=%d C2p=%d M=%d (multiples of 8, at most %d)", a.C1p, a.C2p, a.M,
                kMaxWidth);
    SC2_REQUIRE(a.pix0 >= 0 && a.pix0 <= a.pix1 && (long long)a.pix1 <= (long long)a.H * a.W, SC2_ERR_INVALID_ARG,
                "ar_scan: pixel range [%d, %d) outside %d x %d", a.pix0, a.pix1, a.H, a.W);
    SC2_REQUIRE(a.wc && a.bc && a.w1 && a.p1 && a.w2 && a.b2 && a.w3 && a.b3 && a.scale_table && a.y_hat_pad,
                SC2_ERR_INVALID_ARG, "ar_scan: null weight / map argument");
    // the f32 form loads a pair of adjacent weights as one 8-byte value (sc2_ar_scan's checks are what they were)
    SC2_REQUIRE(sizeof(Wt) != 4 || ((uintptr_t)a.wc | (uintptr_t)a.w1 | (uintptr_t)a.w2 | (uintptr_t)a.w3) % 8 == 0,
                SC2_ERR_INVALID_ARG, "ar_scan: the f32 weight matrices must be 8-byte aligned");
    SC2_REQUIRE(a.n_table >= 1 && a.n_table <= 256 && a.scale_bound > 0.f, SC2_ERR_INVALID_ARG, "ar_scan: scale table");
    long long entries = 0;
    if (a.decode) {
        SC2_REQUIRE(a.buf && a.io_offset && a.io_nbytes && a.cdfs && a.cdf_sizes && a.offsets && a.st_x && a.st_pos && a.status,
                    SC2_ERR_INVALID_ARG, "ar_scan: decoding needs the streams, tables and state");
        SC2_REQUIRE(a.n_cdfs == a.n_table, SC2_ERR_INVALID_ARG, "ar_scan: %d CDF rows for a scale table of %d", a.n_cdfs,
                    a.n_table);
        entries = a.cdf_entries;   // the CDF sizes live on the device
        SC2_REQUIRE(entries > 0, SC2_ERR_INVALID_ARG, "ar_scan: decoding needs cdf_entries");
    } else {
        SC2_REQUIRE(a.y && a.symbols && a.indexes, SC2_ERR_INVALID_ARG, "ar_scan: encoding needs y, symbols and indexes");
    }
    if (a.pix0 == a.pix1 && !a.decode) return SC2_OK;
    constexpr size_t kLdsBytes = 160 * 1024;
    LdsLayout L = ar_lds_layout(a.M, a.C1p, a.C2p, a.n_table, a.n_cdfs, entries, a.decode);
    const bool cdf_lds = !a.decode || (size_t)L.total_words * 4 <= kLdsBytes;
    if (!cdf_lds) L = ar_lds_layout(a.M, a.C1p, a.C2p, a.n_table, a.n_cdfs, 0, 1);   // the rows' start / size / offset only
    const size_t lds = (size_t)L.total_words * 4;
    SC2_REQUIRE(lds <= kLdsBytes, SC2_ERR_UNSUPPORTED, "ar_scan: %zu bytes of LDS needed (160 KiB available)", lds);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (a.decode && cdf_lds) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ar_scan_kernel<true, true, Wt>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((ar_scan_kernel<true, true, Wt>), dim3(a.B), dim3(kThreads), lds, st, a);
    } else if (a.decode) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ar_scan_kernel<true, false, Wt>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((ar_scan_kernel<true, false, Wt>), dim3(a.B), dim3(kThreads), lds, st, a);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ar_scan_kernel<false, false, Wt>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((ar_scan_kernel<false, false, Wt>), dim3(a.B), dim3(kThreads), lds, st, a);
    }
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

}  // namespace

extern "C" int sc2_ar_scan(const sc2_ar_scan_args *args, void *stream) { return ar_scan_launch<uint16_t>(args, stream); }

extern "C" int sc2_ar_scan_f32(const sc2_ar_scan_args *args, void *stream) { return ar_scan_launch<float>(args, stream); }

extern "C" int sc2_rans_decode_resume(const uint8_t *buf, int64_t stride, const int32_t *io_offset, const int32_t *io_nbytes,
                                      const int32_t *indexes, int n_streams, int64_t n_sym, const int32_t *cdfs, int n_cdfs,
                                      int cdf_stride, const int32_t *cdf_sizes, const int32_t *offsets, int first, int last,
                                      uint64_t *st_x, int32_t *st_pos, int32_t *status, int32_t *symbols_out, void *stream) {
    SC2_REQUIRE(buf && io_offset && io_nbytes && cdfs && cdf_sizes && offsets && st_x && st_pos && status,
                SC2_ERR_INVALID_ARG, "rans_decode_resume: null argument");
    SC2_REQUIRE(n_streams > 0 && n_sym >= 0 && n_cdfs > 0 && cdf_stride > 0 && stride > 0, SC2_ERR_INVALID_ARG,
                "rans_decode_resume: bad dims");
    SC2_REQUIRE(n_sym == 0 || (indexes && symbols_out), SC2_ERR_INVALID_ARG, "rans_decode_resume: indexes / output missing");
    hipLaunchKernelGGL(rans_decode_resume_kernel, dim3((n_streams + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       buf, (long long)stride, io_offset, io_nbytes, indexes, n_streams, (long long)n_sym, cdfs, n_cdfs,
                       cdf_stride, cdf_sizes, offsets, first, last, reinterpret_cast<unsigned long long *>(st_x), st_pos,
                       status, symbols_out);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
