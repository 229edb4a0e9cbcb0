// What the segmentation kernels share (seg.hip: labels + confusion counts; seg_loss.hip: the training loss): the integer axis map of
// the bilinear resize, the class loads and the ONE statement of the resized value -- include/sc2_bottleneck.h (sc2_seg_predict)
// states the formula, tests/ref_seg.py restates it in float64.
#pragma once
#include "sc2_common.h"

#pragma clang fp contract(off)   // `(1-ly)*((1-lx)*a + lx*b) + ly*(...)`: every step rounded once, the same for every class

namespace {

constexpr int SEG_MAX_DIM = 32768;           // (2 d + 1) * h - H stays inside 32 bits

// Source index pair and weight of output index d along one axis (align_corners=False), in integers: t = (2d+1)*in - out is the
// source coordinate times 2*out.  t <= 0 is the clamp at the first pixel.
__device__ __forceinline__ void seg_axis(int d, int in, int out, int &i0, int &i1, float &l) {
    const int t = (2 * d + 1) * in - out;
    if (t <= 0) {
        i0 = 0;
        l = 0.0f;
    } else {
        const unsigned den = 2u * (unsigned)out;
        const unsigned q = (unsigned)t / den;
        i0 = (int)q;
        l = (float)((unsigned)t - q * den) / (float)den;
    }
    i1 = min(i0 + 1, in - 1);
}

// seg_axis for d, d + 1, d + 2, ... without a division per step: t = q * den + r is kept in integers (t grows by 2 * in per step);
// q = 0 with r <= 0 is the clamp.  get() returns exactly what seg_axis(d) returns -- the same integers go into the same float division.
struct SegAxisWalk {
    int q, r, in, den;
    __device__ __forceinline__ SegAxisWalk(int d, int in_, int out) : in(in_), den(2 * out) {
        const int t = (2 * d + 1) * in_ - out;
        if (t <= 0) {
            q = 0;
            r = t;
        } else {
            q = (int)((unsigned)t / (unsigned)den);
            r = t - q * den;
        }
    }
    __device__ __forceinline__ void get(int &i0, int &i1, float &l) const {
        i0 = q;
        l = r > 0 ? (float)r / (float)den : 0.0f;
        i1 = min(q + 1, in - 1);
    }
    __device__ __forceinline__ void step() {
        r += 2 * in;
        while (r >= den) {
            r -= den;
            ++q;
        }
    }
};

// first output index whose seg_axis i0 is >= k (k <= 0: 0; k >= in: out): i0(d) is non-decreasing in d, and i0(d) >= k > 0 means
// (2d+1)*in - out >= 2*out*k
__host__ __device__ __forceinline__ int seg_axis_first(int k, int in, int out) {
    if (k <= 0) return 0;
    if (k >= in) return out;
    const long long num = (long long)(2 * k + 1) * out - in;      // 2d >= num / in
    if (num <= 0) return 0;
    const long long d = (num + 2ll * in - 1) / (2ll * in);
    return d < out ? (int)d : out;
}

template <bool BF16>
struct SegVec;
template <>
struct SegVec<false> {     // 4 f32 classes per 16-byte load
    static constexpr int V = 4;
    typedef float elem;
    __device__ static __forceinline__ void load(const void *base, long long at, float (&v)[4]) {
        const float4 q = *reinterpret_cast<const float4 *>(static_cast<const float *>(base) + at);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    __device__ static __forceinline__ float load1(const void *base, long long at) { return static_cast<const float *>(base)[at]; }
};
template <>
struct SegVec<true> {      // 8 bf16 classes per 16-byte load
    static constexpr int V = 8;
    typedef uint16_t elem;
    __device__ static __forceinline__ void load(const void *base, long long at, float (&v)[8]) {
        const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(base) + at);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __builtin_bit_cast(float, w[i] << 16);
            v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xFFFF0000u);
        }
    }
    __device__ static __forceinline__ float load1(const void *base, long long at) {
        return bf16_bits_to_f32(static_cast<const uint16_t *>(base)[at]);
    }
};

// the resized value of one class from its four source values
__device__ __forceinline__ float seg_value(float hy, float hx, float ly, float lx, float a, float b, float c, float d) {
    return hy * (hx * a + lx * b) + ly * (hx * c + lx * d);
}

// f(c, v[p,c]) for c = 0 .. C-1 in order, for the output pixel whose four source pixels start at p00, p01, p10, p11 (element offsets
// of class 0).  VEC: the classes of a pixel are consecutive in memory and readable in whole 16-byte pieces (the pad channels of the
// last piece never reach f).
template <bool BF16, bool VEC, typename F>
__device__ __forceinline__ void seg_for_each_class(const void *logits, int C, long long sC, long long p00, long long p01, long long p10,
                                                   long long p11, float hy, float hx, float ly, float lx, F &&f) {
    constexpr int V = SegVec<BF16>::V;
    if (VEC) {
        for (int c0 = 0; c0 < C; c0 += V) {
            float va[V], vb[V], vc[V], vd[V];
            SegVec<BF16>::load(logits, p00 + c0, va);
            SegVec<BF16>::load(logits, p01 + c0, vb);
            SegVec<BF16>::load(logits, p10 + c0, vc);
            SegVec<BF16>::load(logits, p11 + c0, vd);
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (c0 + v < C) f(c0 + v, seg_value(hy, hx, ly, lx, va[v], vb[v], vc[v], vd[v]));
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const long long o = c * sC;
            f(c, seg_value(hy, hx, ly, lx, SegVec<BF16>::load1(logits, p00 + o), SegVec<BF16>::load1(logits, p01 + o),
                           SegVec<BF16>::load1(logits, p10 + o), SegVec<BF16>::load1(logits, p11 + o)));
        }
    }
}

// 16-byte class loads: consecutive classes, every pixel's first class on a 16-byte boundary, and the whole last piece readable
inline bool seg_vec_ok(const void *logits, int is_bf16, int C, long long stride_n, long long stride_c, long long stride_h,
                       long long stride_w, int c_readable) {
    const int V = is_bf16 ? 8 : 4;
    return stride_c == 1 && c_readable >= (C + V - 1) / V * V && (reinterpret_cast<uintptr_t>(logits) & 15u) == 0 &&
           stride_n % V == 0 && stride_h % V == 0 && stride_w % V == 0;
}

}  // namespace
