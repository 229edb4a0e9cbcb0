// CR+BQ baseline (channel reduction + bottleneck quantization): the 8-bit affine quantizer of the reference's
// `SimpleQuantizer` / `SimpleDequantizer` (sc2bench/transforms/misc.py:181-231, which call torchdistill's
// tensor_util.quantize_tensor / dequantize_tensor) and the two pooling layers of `larger_resnet_bottleneck`
// (sc2bench/models/layer.py:108-153) that the fused conv kernels do not cover.
// Plain grid-size kernels: no workgroup waits for another, no atomics, 64-bit element counts.  Every result is defined to the bit
// (tests/ref_bq.py is the written-down contract): min / max are exact whatever the order, every other step is one IEEE operation.
#include "sc2_common.h"

#pragma clang fp contract(off)   // `zp + x / scale`, `scale * (q - zp)`: each step rounded once (the affine maps ask for fmaf by name)

namespace {

constexpr int BQ_THREADS = 256;
constexpr int BQ_MAX_BLOCKS = 1024;           // partial pairs per segment (launch 2 re-reduces them in every workgroup)
constexpr long long BQ_ELEMS_PER_BLOCK = 4096;   // 16 elements per thread before a segment gets a second workgroup

inline int bq_blocks_per_seg(long long n_per_seg) {
    const long long nb = (n_per_seg + BQ_ELEMS_PER_BLOCK - 1) / BQ_ELEMS_PER_BLOCK;
    return (int)(nb < 1 ? 1 : nb > BQ_MAX_BLOCKS ? BQ_MAX_BLOCKS : nb);
}

// torch.min / torch.max semantics: a NaN anywhere makes both results NaN.  fminf / fmaxf skip NaNs, the flag carries them.
struct MinMax {
    float mn, mx;
    bool nan;
};
__device__ __forceinline__ void mm_init(MinMax &r) { r.mn = __builtin_inff(); r.mx = -__builtin_inff(); r.nan = false; }
__device__ __forceinline__ void mm_take(MinMax &r, float v) {
    r.nan = r.nan || v != v;
    r.mn = fminf(r.mn, v);
    r.mx = fmaxf(r.mx, v);
}

// wave reduction, then LDS across the four waves; every thread returns the workgroup's result
__device__ __forceinline__ MinMax mm_block_reduce(MinMax r, float (*lds)[3]) {
    int nan = r.nan ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        r.mn = fminf(r.mn, __shfl_xor(r.mn, off, 64));
        r.mx = fmaxf(r.mx, __shfl_xor(r.mx, off, 64));
        nan |= __shfl_xor(nan, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        lds[wave][0] = r.mn;
        lds[wave][1] = r.mx;
        lds[wave][2] = nan ? 1.0f : 0.0f;
    }
    __syncthreads();
    MinMax o;
    mm_init(o);
#pragma unroll
    for (int w = 0; w < BQ_THREADS / 64; ++w) {
        o.mn = fminf(o.mn, lds[w][0]);
        o.mx = fmaxf(o.mx, lds[w][1]);
        o.nan = o.nan || lds[w][2] != 0.0f;
    }
    __syncthreads();   // (lds may be written again by the caller's next reduction)
    return o;
}

// Launch 1: workgroup (seg, b) walks its share of segment `seg` -- 16-byte loads where the segment starts on a 16-byte boundary
// (VEC), the n % 4 trailing elements by the first threads of workgroup 0 -- and writes one (min, max) pair; NaN as the pair.
template <bool VEC>
__global__ __launch_bounds__(BQ_THREADS) void bq_minmax_kernel(const float *__restrict__ x, float *__restrict__ partial,
                                                               long long n_per_seg, int nb) {
    __shared__ float lds[BQ_THREADS / 64][3];
    const long long seg = blockIdx.x / nb;
    const int b = (int)(blockIdx.x - seg * nb);
    const float *xs = x + seg * n_per_seg;
    MinMax r;
    mm_init(r);
    if (VEC) {
        const long long n4 = n_per_seg >> 2;
        const float4 *x4 = reinterpret_cast<const float4 *>(xs);
        for (long long i = (long long)b * BQ_THREADS + threadIdx.x; i < n4; i += (long long)nb * BQ_THREADS) {
            const float4 v = x4[i];
            mm_take(r, v.x); mm_take(r, v.y); mm_take(r, v.z); mm_take(r, v.w);
        }
        const long long tail = (n4 << 2) + threadIdx.x;
        if (b == 0 && tail < n_per_seg) mm_take(r, xs[tail]);
    } else {
        for (long long i = (long long)b * BQ_THREADS + threadIdx.x; i < n_per_seg; i += (long long)nb * BQ_THREADS) mm_take(r, xs[i]);
    }
    r = mm_block_reduce(r, lds);
    if (threadIdx.x == 0) {
        const float qnan = __builtin_nanf("");
        partial[2 * (long long)blockIdx.x] = r.nan ? qnan : r.mn;
        partial[2 * (long long)blockIdx.x + 1] = r.nan ? qnan : r.mx;
    }
}

struct BqParams {
    float scale;
    int zp, status;
};

// tensor_util.quantize_tensor's scalar arithmetic, f32, one rounding per step
__device__ __forceinline__ BqParams bq_params(float mn, float mx) {
    BqParams p;
    p.scale = (mx - mn) / 255.0f;
    const float izp = 0.0f - mn / p.scale;
    p.status = izp != izp ? 1 : 0;        // int(nan): the reference raises ValueError here
    const float zpf = izp < 0.0f ? 0.0f : izp > 255.0f ? 255.0f : izp;
    p.zp = p.status ? 0 : (int)zpf;       // truncation toward zero
    return p;
}

__device__ __forceinline__ uint32_t bq_code(float x, float scale, float zpf) {
    float q = zpf + x / scale;
    q = q < 0.0f ? 0.0f : q > 255.0f ? 255.0f : q;   // clamp_: a NaN stays a NaN
    q = rintf(q);                                    // half to even
    return q == q ? (uint32_t)(int)q : 0u;           // (NaN -> u8 is undefined in the reference too: 0 here)
}

// Launch 2: every workgroup reduces its segment's nb pairs again (same exact result everywhere), derives scale and zero point and
// quantizes the share of the segment it read in launch 1.  Workgroup 0 of a segment writes the three scalars.
template <bool VEC>
__global__ __launch_bounds__(BQ_THREADS) void bq_quantize_kernel(const float *__restrict__ x, const float *__restrict__ partial,
                                                                 uint8_t *__restrict__ q, float *__restrict__ scale,
                                                                 int32_t *__restrict__ zero_point, int32_t *__restrict__ status,
                                                                 long long n_per_seg, int nb) {
    __shared__ float lds[BQ_THREADS / 64][3];
    const long long seg = blockIdx.x / nb;
    const int b = (int)(blockIdx.x - seg * nb);
    MinMax r;
    mm_init(r);
    for (int i = threadIdx.x; i < nb; i += BQ_THREADS) {
        mm_take(r, partial[2 * (seg * nb + i)]);
        mm_take(r, partial[2 * (seg * nb + i) + 1]);
    }
    r = mm_block_reduce(r, lds);
    const float qnan = __builtin_nanf("");
    const BqParams p = bq_params(r.nan ? qnan : r.mn, r.nan ? qnan : r.mx);
    if (b == 0 && threadIdx.x == 0) {
        scale[seg] = p.scale;
        zero_point[seg] = p.zp;
        status[seg] = p.status;
    }
    const float zpf = (float)p.zp;
    const float *xs = x + seg * n_per_seg;
    uint8_t *qs = q + seg * n_per_seg;
    if (VEC) {
        const long long n4 = n_per_seg >> 2;
        const float4 *x4 = reinterpret_cast<const float4 *>(xs);
        uint32_t *q4 = reinterpret_cast<uint32_t *>(qs);
        for (long long i = (long long)b * BQ_THREADS + threadIdx.x; i < n4; i += (long long)nb * BQ_THREADS) {
            const float4 v = x4[i];
            q4[i] = p.status ? 0u
                             : bq_code(v.x, p.scale, zpf) | (bq_code(v.y, p.scale, zpf) << 8) | (bq_code(v.z, p.scale, zpf) << 16) |
                                   (bq_code(v.w, p.scale, zpf) << 24);
        }
        const long long tail = (n4 << 2) + threadIdx.x;
        if (b == 0 && tail < n_per_seg) qs[tail] = p.status ? (uint8_t)0 : (uint8_t)bq_code(xs[tail], p.scale, zpf);
    } else {
        for (long long i = (long long)b * BQ_THREADS + threadIdx.x; i < n_per_seg; i += (long long)nb * BQ_THREADS)
            qs[i] = p.status ? (uint8_t)0 : (uint8_t)bq_code(xs[i], p.scale, zpf);
    }
}

// tensor_util.dequantize_tensor: scale * (q.float() - zero_point), segment by segment.  One thread = 4 codes (VEC) or 1.
template <bool VEC>
__global__ __launch_bounds__(BQ_THREADS) void bq_dequantize_f32_kernel(const uint8_t *__restrict__ q, const float *__restrict__ scale,
                                                                       const int32_t *__restrict__ zero_point, float *__restrict__ y,
                                                                       long long n_per_seg, long long total) {
    const long long t = (long long)blockIdx.x * BQ_THREADS + threadIdx.x;
    if (VEC) {
        const long long i = t << 2;
        if (i + 4 <= total) {
            const long long seg = i / n_per_seg;     // (n_per_seg % 4 == 0 or one segment: the four codes share it)
            const float s = scale[seg], z = (float)zero_point[seg];
            const uint32_t c = reinterpret_cast<const uint32_t *>(q)[t];
            reinterpret_cast<float4 *>(y)[t] = make_float4(s * ((float)(c & 255u) - z), s * ((float)((c >> 8) & 255u) - z),
                                                           s * ((float)((c >> 16) & 255u) - z), s * ((float)(c >> 24) - z));
        } else {
            for (long long j = i; j < total; ++j) {  // the n % 4 trailing codes of a single segment
                const long long seg = j / n_per_seg;
                y[j] = scale[seg] * ((float)q[j] - (float)zero_point[seg]);
            }
        }
    } else if (t < total) {
        const long long seg = t / n_per_seg;
        y[t] = scale[seg] * ((float)q[t] - (float)zero_point[seg]);
    }
}

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.0f ? 0.0f : v; }

// u8 NCHW codes -> dequantized bf16 NHWC map, channels zero-padded to Cpad, with the decoder's leading BatchNorm2d (eval: a
// per-channel affine) + ReLU folded in: relu(fmaf(a_c, scale * (q - zp), b_c)) in f32, rounded to bf16 once.  One thread = one
// pixel x 8 channels; lanes run along pixels, so each channel plane is read in contiguous bytes (nchw_f32_to_nhwc_bf16's shape).
__global__ __launch_bounds__(BQ_THREADS) void bq_dequantize_nhwc_kernel(const uint8_t *__restrict__ q, const float *__restrict__ scale,
                                                                        const int32_t *__restrict__ zero_point, int per_sample,
                                                                        const float *__restrict__ a, const float *__restrict__ b, int relu,
                                                                        uint16_t *__restrict__ y, int C, int HW, int Cpad,
                                                                        long long total_pix) {
    const long long gp = (long long)blockIdx.x * BQ_THREADS + threadIdx.x;
    if (gp >= total_pix) return;
    const int c0 = blockIdx.y * 8;
    const long long n = gp / HW;
    const int pix = (int)(gp - n * HW);
    const long long seg = per_sample ? n : 0;
    const float s = scale[seg], z = (float)zero_point[seg];
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        float r = 0.0f;              // padding channels: exact zeros
        if (c < C) {
            r = s * ((float)q[(n * C + c) * HW + pix] - z);
            if (a) r = fmaf(a[c], r, b[c]);
            if (relu) r = relu_keep_nan(r);
        }
        v[j] = r;
    }
    uint4 o;
    o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]);
    o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
    *reinterpret_cast<uint4 *>(y + gp * Cpad + c0) = o;
}

// MaxPool2d + BatchNorm2d (eval) + ReLU on a bf16 NHWC map: maxpool_nhwc_kernel's window walk (layout.hip: torch's update rule from
// -inf in row-major order, NaN propagates), then relu(fmaf(a_c, m, b_c)) in f32, rounded to bf16 once.  The affine comes AFTER the
// max: a negative norm scale must not turn the max into a min.
__global__ __launch_bounds__(256) void maxpool_affine_relu_nhwc_kernel(const uint16_t *__restrict__ x, uint16_t *__restrict__ y,
                                                                       const float *__restrict__ a, const float *__restrict__ b, int H, int W,
                                                                       int C8, int OH, int OW, int KH, int KW, int SH, int SW, int PH, int PW,
                                                                       long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c8 = (int)(t % C8);
    long long px = t / C8;
    const int ow = (int)(px % OW);
    px /= OW;
    const int oh = (int)(px % OH);
    const long long n = px / OH;
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -__builtin_inff();
    const uint4 *xi = reinterpret_cast<const uint4 *>(x) + n * H * W * C8 + c8;
    for (int kh = 0; kh < KH; ++kh) {
        const int ih = oh * SH - PH + kh;
        if ((unsigned)ih >= (unsigned)H) continue;
        for (int kw = 0; kw < KW; ++kw) {
            const int iw = ow * SW - PW + kw;
            if ((unsigned)iw >= (unsigned)W) continue;
            const uint4 v = xi[((long long)ih * W + iw) * C8];
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float lo = __builtin_bit_cast(float, w4[k] << 16), hi = __builtin_bit_cast(float, w4[k] & 0xFFFF0000u);
                if (lo > m[2 * k] || lo != lo) m[2 * k] = lo;
                if (hi > m[2 * k + 1] || hi != hi) m[2 * k + 1] = hi;
            }
        }
    }
    const float4 a0 = reinterpret_cast<const float4 *>(a)[2 * c8], a1 = reinterpret_cast<const float4 *>(a)[2 * c8 + 1];
    const float4 b0 = reinterpret_cast<const float4 *>(b)[2 * c8], b1 = reinterpret_cast<const float4 *>(b)[2 * c8 + 1];
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = relu_keep_nan(fmaf(av[e], m[e], bv[e]));
    uint4 o;
    o.x = pack_bf16x2(m[0], m[1]); o.y = pack_bf16x2(m[2], m[3]);
    o.z = pack_bf16x2(m[4], m[5]); o.w = pack_bf16x2(m[6], m[7]);
    reinterpret_cast<uint4 *>(y)[t] = o;
}

// AvgPool2d(kernel K, stride S, no padding) on a bf16 NHWC map: f32 sum over the window in row-major order, times 1 / (K * K),
// rounded to bf16 once.  One thread = one output pixel x 8 channels.
__global__ __launch_bounds__(256) void avgpool2d_nhwc_kernel(const uint16_t *__restrict__ x, uint16_t *__restrict__ y, int H, int W, int C8,
                                                             int OH, int OW, int K, int S, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c8 = (int)(t % C8);
    long long px = t / C8;
    const int ow = (int)(px % OW);
    px /= OW;
    const int oh = (int)(px % OH);
    const long long n = px / OH;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const uint4 *xi = reinterpret_cast<const uint4 *>(x) + n * H * W * C8 + c8;
    for (int kh = 0; kh < K; ++kh)
        for (int kw = 0; kw < K; ++kw) {
            const uint4 v = xi[((long long)(oh * S + kh) * W + (ow * S + kw)) * C8];
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc[2 * k] += __builtin_bit_cast(float, w4[k] << 16);
                acc[2 * k + 1] += __builtin_bit_cast(float, w4[k] & 0xFFFF0000u);
            }
        }
    const float inv = 1.0f / (float)(K * K);
    uint4 o;
    o.x = pack_bf16x2(acc[0] * inv, acc[1] * inv); o.y = pack_bf16x2(acc[2] * inv, acc[3] * inv);
    o.z = pack_bf16x2(acc[4] * inv, acc[5] * inv); o.w = pack_bf16x2(acc[6] * inv, acc[7] * inv);
    reinterpret_cast<uint4 *>(y)[t] = o;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" long long sc2_bq_partial_len(long long n_seg, long long n_per_seg) {
    if (n_seg <= 0 || n_per_seg <= 0) return 0;
    return 2 * n_seg * bq_blocks_per_seg(n_per_seg);
}

extern "C" int sc2_bq_quantize(const float *x, uint8_t *q, float *scale, int32_t *zero_point, int32_t *status, float *partial,
                               long long n_seg, long long n_per_seg, void *stream) {
    SC2_REQUIRE(x && q && scale && zero_point && status && partial, SC2_ERR_INVALID_ARG, "bq_quantize: null argument");
    SC2_REQUIRE(n_seg > 0 && n_per_seg > 0 && n_per_seg <= 0x7FFFFFFFFFFFFFFFLL / n_seg, SC2_ERR_INVALID_ARG,
                "bq_quantize: bad sizes n_seg=%lld n_per_seg=%lld", n_seg, n_per_seg);
    const int nb = bq_blocks_per_seg(n_per_seg);
    SC2_REQUIRE(n_seg * nb < 0x7FFFFFFFLL, SC2_ERR_UNSUPPORTED, "bq_quantize: too many segments (%lld x %d workgroups)", n_seg, nb);
    const unsigned grid = (unsigned)(n_seg * nb);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // 16-byte loads / 4-byte code stores need every segment to start on such a boundary
    const bool vec = aligned16(x) && aligned4(q) && (n_seg == 1 || n_per_seg % 4 == 0);
    if (vec) {
        hipLaunchKernelGGL(bq_minmax_kernel<true>, dim3(grid), dim3(BQ_THREADS), 0, s, x, partial, n_per_seg, nb);
        SC2_CHECK_LAUNCH();
        hipLaunchKernelGGL(bq_quantize_kernel<true>, dim3(grid), dim3(BQ_THREADS), 0, s, x, partial, q, scale, zero_point, status,
                           n_per_seg, nb);
    } else {
        hipLaunchKernelGGL(bq_minmax_kernel<false>, dim3(grid), dim3(BQ_THREADS), 0, s, x, partial, n_per_seg, nb);
        SC2_CHECK_LAUNCH();
        hipLaunchKernelGGL(bq_quantize_kernel<false>, dim3(grid), dim3(BQ_THREADS), 0, s, x, partial, q, scale, zero_point, status,
                           n_per_seg, nb);
    }
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_bq_dequantize(const uint8_t *q, const float *scale, const int32_t *zero_point, float *y, long long n_seg,
                                 long long n_per_seg, void *stream) {
    SC2_REQUIRE(q && scale && zero_point && y, SC2_ERR_INVALID_ARG, "bq_dequantize: null argument");
    SC2_REQUIRE(n_seg > 0 && n_per_seg > 0 && n_per_seg <= 0x7FFFFFFFFFFFFFFFLL / n_seg, SC2_ERR_INVALID_ARG,
                "bq_dequantize: bad sizes n_seg=%lld n_per_seg=%lld", n_seg, n_per_seg);
    const long long total = n_seg * n_per_seg;
    const bool vec = aligned4(q) && aligned16(y) && (n_seg == 1 || n_per_seg % 4 == 0);
    const long long threads = vec ? (total + 3) / 4 : total;
    const long long blocks = (threads + BQ_THREADS - 1) / BQ_THREADS;
    SC2_REQUIRE(blocks < 0x7FFFFFFFLL, SC2_ERR_UNSUPPORTED, "bq_dequantize: problem too large");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(bq_dequantize_f32_kernel<true>, dim3((unsigned)blocks), dim3(BQ_THREADS), 0, s, q, scale, zero_point, y,
                           n_per_seg, total);
    else
        hipLaunchKernelGGL(bq_dequantize_f32_kernel<false>, dim3((unsigned)blocks), dim3(BQ_THREADS), 0, s, q, scale, zero_point, y,
                           n_per_seg, total);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_bq_dequantize_nhwc(const uint8_t *q, const float *scale, const int32_t *zero_point, int per_sample, const float *a,
                                      const float *b, int relu, void *y, int N, int C, int H, int W, int Cpad, void *stream) {
    SC2_REQUIRE(q && scale && zero_point && y && (!a == !b), SC2_ERR_INVALID_ARG, "bq_dequantize_nhwc: null argument (a and b come together)");
    SC2_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && Cpad >= C && Cpad % 8 == 0 && Cpad / 8 <= 65535 && (long long)H * W < 0x7FFFFFFFLL,
                SC2_ERR_INVALID_ARG, "bq_dequantize_nhwc: bad dims N=%d C=%d H=%d W=%d Cpad=%d", N, C, H, W, Cpad);
    const long long total = (long long)N * H * W;
    const long long blocks = (total + BQ_THREADS - 1) / BQ_THREADS;
    SC2_REQUIRE(blocks < 0x7FFFFFFFLL, SC2_ERR_UNSUPPORTED, "bq_dequantize_nhwc: problem too large");
    hipLaunchKernelGGL(bq_dequantize_nhwc_kernel, dim3((unsigned)blocks, Cpad / 8), dim3(BQ_THREADS), 0, static_cast<hipStream_t>(stream), q,
                       scale, zero_point, per_sample ? 1 : 0, a, b, relu ? 1 : 0, static_cast<uint16_t *>(y), C, H * W, Cpad, total);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_maxpool_affine_relu_nhwc(const void *x, void *y, const float *a, const float *b, int N, int H, int W, int C, int KH, int KW,
                                            int stride_h, int stride_w, int pad_h, int pad_w, void *stream) {
    SC2_REQUIRE(x && y && a && b, SC2_ERR_INVALID_ARG, "maxpool_affine_relu_nhwc: null argument");
    SC2_REQUIRE(aligned16(a) && aligned16(b), SC2_ERR_INVALID_ARG, "maxpool_affine_relu_nhwc: a and b must be 16-byte aligned");
    SC2_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, SC2_ERR_INVALID_ARG,
                "maxpool_affine_relu_nhwc: bad dims N=%d H=%d W=%d C=%d (C %% 8 == 0)", N, H, W, C);
    SC2_REQUIRE(KH > 0 && KW > 0 && stride_h > 0 && stride_w > 0 && pad_h >= 0 && pad_w >= 0 && 2 * pad_h <= KH && 2 * pad_w <= KW,
                SC2_ERR_INVALID_ARG, "maxpool_affine_relu_nhwc: bad window (padding at most half the kernel, as nn.MaxPool2d requires)");
    const int OH = (H + 2 * pad_h - KH) / stride_h + 1, OW = (W + 2 * pad_w - KW) / stride_w + 1;
    SC2_REQUIRE(OH > 0 && OW > 0, SC2_ERR_INVALID_ARG, "maxpool_affine_relu_nhwc: window larger than the padded map");
    const long long total = (long long)N * OH * OW * (C / 8);
    SC2_REQUIRE((total + 255) / 256 < 0x7FFFFFFFLL, SC2_ERR_UNSUPPORTED, "maxpool_affine_relu_nhwc: problem too large");
    hipLaunchKernelGGL(maxpool_affine_relu_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), static_cast<uint16_t *>(y), a, b, H, W, C / 8, OH, OW, KH, KW, stride_h, stride_w,
                       pad_h, pad_w, total);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_avgpool2d_nhwc(const void *x, void *y, int N, int H, int W, int C, int kernel, int stride, void *stream) {
    SC2_REQUIRE(x && y, SC2_ERR_INVALID_ARG, "avgpool2d_nhwc: null argument");
    SC2_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, SC2_ERR_INVALID_ARG, "avgpool2d_nhwc: bad dims N=%d H=%d W=%d C=%d (C %% 8 == 0)",
                N, H, W, C);
    SC2_REQUIRE(kernel > 0 && kernel <= 64 && stride > 0 && kernel <= H && kernel <= W, SC2_ERR_INVALID_ARG,
                "avgpool2d_nhwc: bad window kernel=%d stride=%d on a %dx%d map", kernel, stride, H, W);
    const int OH = (H - kernel) / stride + 1, OW = (W - kernel) / stride + 1;
    const long long total = (long long)N * OH * OW * (C / 8);
    SC2_REQUIRE((total + 255) / 256 < 0x7FFFFFFFLL, SC2_ERR_UNSUPPORTED, "avgpool2d_nhwc: problem too large");
    hipLaunchKernelGGL(avgpool2d_nhwc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), static_cast<uint16_t *>(y), H, W, C / 8, OH, OW, kernel, stride, total);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
