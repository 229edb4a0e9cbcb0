// The frame that the f32 convolution (conv_f32.hip) and the split-bf16 convolution (conv_split.hip) share: the argument fields, the
// tap table entry, the per-lane output-row set-up, the epilogue, the descriptor checks and the chunk-width rule.  Only code that is
// THE SAME for both lives here: nothing in this file knows which of the two called it.  Their k loops, operand loads and weight
// rings differ in substance and stay in their files.
//
// The epilogue decides the bytes a user gets -- the reference's operation order (norm = beta + acc, IEEE division, one multiply:
// compressai.layers.GDN1.forward) and the symbol rounding rintf(acc - median) -- so the modes 'f32', 'bf16x3' and 'bf16x6' code
// the same stream from equal accumulators because they run this one copy of it.
//
// The squared-form GDN of the input codecs (compressai.layers.GDN: SC2_EPI_GDN2 / SC2_EPI_IGDN2, a 1x1 launch with a_op = SQUARE,
// ep_x = the GDN's input, ep_beta = the effective beta) is norm = acc + beta[c], r = sqrtf(norm), then y = ep_x * r (IGDN2) or
// y = ep_x * (1.0f / r) (GDN2): a correctly rounded square root, a correctly rounded division and one multiply -- never a
// reciprocal-square-root instruction or intrinsic, and no fast-math flag on the files that include this.  Why 1 / sqrt and not the
// reference's torch.rsqrt: the reference's rsqrt is not bit-defined.  On the CPU (torch 2.10, 4 M random values in (0, 100))
// torch.rsqrt(x) differs from 1 / torch.sqrt(x) on 0.57 % of the values, and agrees on short tensors, which take the vectoriser's
// tail path.  So there is no bit target; the device takes the form that is reproducible and within an ulp of either CPU path.
#pragma once

#include "sc2_common.h"

namespace {

struct PreciseArgs {
    const float *__restrict__ x;       // f32 NHWC [N, H, W, Cin] (Cin % 4 == 0)
    const float *__restrict__ ep_x;    // f32 NHWC [N, OH, OW, Cout] (GDN operand) or null
    const float *__restrict__ ep_beta; // f32 [Cout]: beta (GDN) / bias / medians (symbols) or null
    void *__restrict__ y;
    int N, H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w, OH, OW;
    int o_H, o_W, o_sh, o_sw, o_h0, o_w0;   // output scatter (o_H == 0: dense): pixel (oh, ow) -> (oh o_sh + o_h0, ow o_sw + o_w0) of [N, o_H, o_W, Cout]
    int a_op, epilogue, out_format;
    int n_steps;                       // k-steps of the caller's MFMA shape
    long long M;                       // N * OH * OW
    unsigned x_bytes;                  // size of x (< 2 GB: the activation loads go through a buffer descriptor)
    unsigned w_bytes;                  // size of the weight stream
    unsigned ring_off;                 // LDS offset of the weight ring (after the tap table, 1 KB aligned)
};

// Tap table entry of k quad e (k0 = 4 e, K = (kh, kw, ci) with ci fastest): {byte offset of the quad inside the window, kh | kw << 16}.
// pix_floats: floats from one pixel of x to the next (Cin for NHWC; 1 where a channel plane is addressed, whose quads start at ci = 0).
__device__ __forceinline__ int2 precise_tap_entry(const PreciseArgs &p, int e, int pix_floats) {
    const int k0 = e * 4;
    const int tap = k0 / p.Cin, ci = k0 - tap * p.Cin;
    int2 v;
    if (tap < p.KH * p.KW) {
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
        v.x = ((kh * p.W + kw) * pix_floats + ci) * 4;      // BYTE offset inside the window
        v.y = kh | (kw << 16);
    } else {            // K padding: never in bounds (its weights are zero too)
        v.x = 0;
        v.y = 0x7FFF | (0x7FFF << 16);
    }
    return v;
}

// The lane's A rows: pixel m_base + mt * 16 + r.  a_base: byte offset of the window's first pixel, ih0 / iw0: its position.
// img_rows: rows of W pixels from one image of x to the next (H; 3 H for three channel planes), pix_floats as above.
// (byte offsets modulo 2^32: a window that starts above / left of the image has a negative base, but base + tap offset of
//  every tap that is INSIDE the image is a plain offset below x_bytes < 2^31)
template <int MT>
__device__ __forceinline__ void precise_rows(const PreciseArgs &p, long long m_base, int r, int img_rows, int pix_floats,
                                             uint32_t (&a_base)[MT], int (&ih0)[MT], int (&iw0)[MT]) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const long long m = m_base + mt * 16 + r;
        if (m < p.M) {                             // (M < 2^31, checked by the host: 32-bit divisions)
            const uint32_t ohw_u = (uint32_t)(p.OH * p.OW), n = (uint32_t)m / ohw_u;
            const int rem = (int)((uint32_t)m - n * ohw_u);
            const int oh = (int)((uint32_t)rem / (uint32_t)p.OW), ow = rem - oh * p.OW;
            ih0[mt] = oh * p.stride - p.pad_h;
            iw0[mt] = ow * p.stride - p.pad_w;
            a_base[mt] = (uint32_t)(((((long long)n * img_rows + ih0[mt]) * (long long)p.W + iw0[mt]) * pix_floats) * 4);
        } else {
            ih0[mt] = iw0[mt] = -(1 << 20);       // every tap out of bounds: zeros
            a_base[mt] = 0;
        }
    }
}

// Epilogue.  The WEIGHTS are the first MFMA operand, so the result tile is [channel][pixel]: acc[mt][nt][i] = output
// (pixel m_base + mt * 16 + r, channel (chunk * NT + nt) * 16 + 4 q + i) -- a lane holds FOUR CONSECUTIVE CHANNELS of one
// pixel: one 16-byte access per tile for NHWC tensors (ep_x, y), and for NCHW outputs the 16 lanes of a quarter write 16
// consecutive pixels of a channel plane.  nrm: the fused GDN's gamma |acc| sums in the same layout (FUSED only).
// Output scatter (o_H != 0; f32 NHWC, plain / bias / activation epilogues only: the host refuses the rest, GDN2 / IGDN2 included): the pixel's row of
// y is that of its place in [N, o_H, o_W, Cout]; a pixel outside that tensor is dropped.
template <int MT, int NT, bool FUSED>
__device__ __forceinline__ void precise_epilogue(const PreciseArgs &p, const f32x4_t (&acc)[MT][NT],
                                                 const f32x4_t (&nrm)[FUSED ? MT : 1][FUSED ? NT : 1], long long m_base, int chunk,
                                                 int r, int q) {
    const long long ohw = (long long)p.OH * p.OW;
    const bool vec4 = (p.Cout & 3) == 0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const long long m = m_base + mt * 16 + r;
        if (m >= p.M) continue;
        const long long n_img = (uint32_t)m / (uint32_t)ohw;
        const long long pix = m - n_img * ohw;
        long long y_row = m;                       // pixel index of the NHWC output
        if constexpr (!FUSED) {
            if (p.o_H != 0) {
                const int oh = (int)((uint32_t)pix / (uint32_t)p.OW), ow = (int)pix - oh * p.OW;
                const int yh = oh * p.o_sh + p.o_h0, yw = ow * p.o_sw + p.o_w0;
                if (yh >= p.o_H || yw >= p.o_W) continue;
                y_row = (n_img * p.o_H + yh) * p.o_W + yw;
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int c0 = (chunk * NT + nt) * 16 + 4 * q;
            if (c0 >= p.Cout) continue;
            float v[4] = {acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]};
            float bc[4] = {0.f, 0.f, 0.f, 0.f};
            if (p.ep_beta) {
                if (vec4) {
                    const f32x4_t b = *reinterpret_cast<const f32x4_t *>(p.ep_beta + c0);
                    bc[0] = b.x; bc[1] = b.y; bc[2] = b.z; bc[3] = b.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) bc[i] = c0 + i < p.Cout ? p.ep_beta[c0 + i] : 0.f;
                }
            }
            if constexpr (FUSED) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float norm = nrm[mt][nt][i] + bc[i];
                    if (p.epilogue == SC2_EPI_FUSED_GDN) norm = 1.0f / norm;
                    v[i] = v[i] * norm;
                }
            } else if (p.epilogue == SC2_EPI_GDN || p.epilogue == SC2_EPI_IGDN || p.epilogue == SC2_EPI_GDN2 || p.epilogue == SC2_EPI_IGDN2) {
                const bool squared = p.epilogue == SC2_EPI_GDN2 || p.epilogue == SC2_EPI_IGDN2;
                const bool divide = p.epilogue == SC2_EPI_GDN || p.epilogue == SC2_EPI_GDN2;
                float xv[4];
                if (vec4) {
                    const f32x4_t t = *reinterpret_cast<const f32x4_t *>(p.ep_x + m * p.Cout + c0);
                    xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) xv[i] = c0 + i < p.Cout ? p.ep_x[m * p.Cout + c0 + i] : 0.f;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float norm = v[i] + bc[i];                 // conv2d(|x| or x^2, gamma, beta): the bias joins the finished sum
                    if (squared) norm = sqrtf(norm);           // correctly rounded (see the header comment: no rsqrt)
                    if (divide) norm = 1.0f / norm;            // IEEE division, then one multiply, as GDN1.forward
                    v[i] = xv[i] * norm;
                }
            } else if (p.epilogue == SC2_EPI_BIAS) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += bc[i];
            } else if (p.epilogue == SC2_EPI_BIAS_RELU || p.epilogue == SC2_EPI_BIAS_LEAKY_RELU) {
                // torch's CPU forms on the f32 value: relu v > 0 ? v : 0, leaky_relu v > 0 ? v : v * 0.01f (one f32 multiply)
                const bool leaky = p.epilogue == SC2_EPI_BIAS_LEAKY_RELU;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float t = p.ep_beta ? v[i] + bc[i] : v[i];
                    v[i] = t > 0.f ? t : (leaky ? t * 0.01f : 0.f);
                }
            }
            if (p.out_format == SC2_OUT_F32_NHWC) {
                float *dst = static_cast<float *>(p.y) + y_row * p.Cout + c0;
                if (vec4) {
                    *reinterpret_cast<f32x4_t *>(dst) = f32x4_t{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (c0 + i < p.Cout) dst[i] = v[i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (c0 + i >= p.Cout) continue;
                    const long long o = (n_img * p.Cout + c0 + i) * ohw + pix;
                    if (p.out_format == SC2_OUT_F32_NCHW) static_cast<float *>(p.y)[o] = v[i];
                    else static_cast<int32_t *>(p.y)[o] = (int32_t)rintf(v[i] - bc[i]);   // symbols: bc = the channel's median
                }
            }
        }
    }
}

// Output channels of one chunk (= of one wave): 32 / 48 / 96.
inline int precise_chunk_channels(int Cout) { return Cout <= 32 ? 32 : (Cout <= 48 ? 48 : 96); }

// The descriptor rules both entry points have; `who` names the entry point in the messages.  gamma: the fused GDN's packed gamma.
// (The callers check their own rules after these: a descriptor that breaks several rules at once is refused for the first one here.)
inline int precise_check_desc(const char *who, const sc2_conv_desc *d, const void *ep_x, const void *gamma, const void *ep_beta) {
    SC2_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cin % 4 == 0 && d->Cout > 0 && d->KH > 0 && d->KW > 0,
                SC2_ERR_INVALID_ARG, "%s: bad dims (Cin must be a multiple of 4)", who);
    SC2_REQUIRE(d->stride_h == d->stride_w && d->stride_h > 0, SC2_ERR_UNSUPPORTED, "%s: square stride only", who);
    SC2_REQUIRE(d->pad_h >= 0 && d->pad_w >= 0, SC2_ERR_INVALID_ARG, "%s: negative padding", who);
    const bool scatter = d->out_H != 0;
    if (scatter) {
        // transposed-convolution use, with the meaning sc2_conv2d_fwd gives the fields: OH / OW as given (rows past the padding
        // formula read implicit zeros: the bounded activation loads), each pixel's place in [N, out_H, out_W, Cout] from the strides
        // and offsets, pixels outside it dropped
        SC2_REQUIRE(d->out_H > 0 && d->out_W > 0 && d->OH > 0 && d->OW > 0 && d->out_stride_h > 0 && d->out_stride_w > 0 &&
                        d->out_off_h >= 0 && d->out_off_w >= 0,
                    SC2_ERR_INVALID_ARG, "%s: bad output scatter", who);
        // (32-bit row / column arithmetic in the kernels: oh * stride - pad, oh * out_stride + out_off)
        SC2_REQUIRE((long long)d->OH * d->stride_h < (1 << 30) && (long long)d->OW * d->stride_w < (1 << 30) &&
                        (long long)d->OH * d->out_stride_h + d->out_off_h < (1 << 30) && (long long)d->OW * d->out_stride_w + d->out_off_w < (1 << 30) &&
                        (long long)d->N * d->out_H * d->out_W * d->Cout < (1ll << 33),
                    SC2_ERR_UNSUPPORTED, "%s: scatter geometry too large for this kernel's index arithmetic", who);
        SC2_REQUIRE(d->out_format == SC2_OUT_F32_NHWC, SC2_ERR_UNSUPPORTED, "%s: output scatter writes f32 NHWC only (out_format %d)", who,
                    d->out_format);
        SC2_REQUIRE(d->epilogue == SC2_EPI_NONE || d->epilogue == SC2_EPI_BIAS || d->epilogue == SC2_EPI_BIAS_RELU ||
                        d->epilogue == SC2_EPI_BIAS_LEAKY_RELU,
                    SC2_ERR_UNSUPPORTED, "%s: output scatter takes the plain, bias and activation epilogues only (epilogue %d)", who, d->epilogue);
    } else {
        SC2_REQUIRE(d->OH == (d->H + 2 * d->pad_h - d->KH) / d->stride_h + 1 && d->OW == (d->W + 2 * d->pad_w - d->KW) / d->stride_w + 1 &&
                        d->OH > 0 && d->OW > 0,
                    SC2_ERR_INVALID_ARG, "%s: OH / OW do not match the geometry", who);
    }
    SC2_REQUIRE(d->a_op == SC2_AOP_NONE || d->a_op == SC2_AOP_ABS || d->a_op == SC2_AOP_SQUARE, SC2_ERR_INVALID_ARG, "%s: a_op", who);
    const bool fused = d->epilogue == SC2_EPI_FUSED_GDN || d->epilogue == SC2_EPI_FUSED_IGDN;
    const bool act = d->epilogue == SC2_EPI_BIAS_RELU || d->epilogue == SC2_EPI_BIAS_LEAKY_RELU;   // (ep_beta may be null: no bias)
    const bool gdn = d->epilogue == SC2_EPI_GDN || d->epilogue == SC2_EPI_IGDN || d->epilogue == SC2_EPI_GDN2 || d->epilogue == SC2_EPI_IGDN2;
    SC2_REQUIRE(d->epilogue == SC2_EPI_NONE || gdn || d->epilogue == SC2_EPI_BIAS || act || fused,
                SC2_ERR_UNSUPPORTED, "%s: epilogue %d", who, d->epilogue);
    SC2_REQUIRE(!act || d->out_format != SC2_OUT_I32_NCHW_SYM, SC2_ERR_INVALID_ARG,
                "%s: symbols come straight from the accumulators (epilogue NONE)", who);
    SC2_REQUIRE(!fused || (d->Cout <= 96 && gamma && ep_beta), SC2_ERR_UNSUPPORTED,
                "%s: the fused GDN needs every channel of a pixel in one chunk (Cout <= 96), gamma fragments and beta", who);
    // the fused norm GEMM walks the whole chunk width in k-steps of gamma fragments; gamma is packed as a 1x1 weight of K = Cout,
    // ceil(Cout / 16) tiles wide: a narrower Cout (49 .. 80, or <= 16) would read up to 12 KB past the tensor
    SC2_REQUIRE(!fused || (d->Cout + 15) / 16 * 16 == precise_chunk_channels(d->Cout), SC2_ERR_UNSUPPORTED,
                "%s: the fused GDN needs ceil(Cout / 16) * 16 == the chunk width (%d channels: chunk %d); run conv and GDN1 as two launches",
                who, d->Cout, precise_chunk_channels(d->Cout));
    SC2_REQUIRE(d->out_format == SC2_OUT_F32_NHWC || d->out_format == SC2_OUT_F32_NCHW || d->out_format == SC2_OUT_I32_NCHW_SYM,
                SC2_ERR_UNSUPPORTED, "%s: out_format %d", who, d->out_format);
    SC2_REQUIRE(!gdn || (ep_x && ep_beta), SC2_ERR_INVALID_ARG, "%s: GDN epilogue needs ep_x and ep_beta", who);
    SC2_REQUIRE((d->epilogue != SC2_EPI_BIAS && d->out_format != SC2_OUT_I32_NCHW_SYM) || ep_beta, SC2_ERR_INVALID_ARG,
                "%s: ep_beta (bias / medians) missing", who);
    SC2_REQUIRE(d->out_format != SC2_OUT_I32_NCHW_SYM || d->epilogue == SC2_EPI_NONE, SC2_ERR_INVALID_ARG,
                "%s: symbols come straight from the accumulators (epilogue NONE)", who);
    return SC2_OK;
}

// The fields of a checked descriptor that both kernels read (n_steps and the byte sizes are the caller's).
inline void precise_fill_args(PreciseArgs &a, const sc2_conv_desc *d, const float *x, const float *ep_x, const float *ep_beta, void *y) {
    a.x = x; a.ep_x = ep_x; a.ep_beta = ep_beta; a.y = y;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout; a.KH = d->KH; a.KW = d->KW;
    a.stride = d->stride_h; a.pad_h = d->pad_h; a.pad_w = d->pad_w; a.OH = d->OH; a.OW = d->OW;
    a.o_H = d->out_H; a.o_W = d->out_W; a.o_sh = d->out_stride_h; a.o_sw = d->out_stride_w; a.o_h0 = d->out_off_h; a.o_w0 = d->out_off_w;
    a.a_op = d->a_op; a.epilogue = d->epilogue; a.out_format = d->out_format;
    a.M = (long long)d->N * d->OH * d->OW;
}

// Raises kernel KERN's dynamic-LDS limit to `lds` bytes (> 64 KB needs it) unless it is there already: a per-device property of
// the function.  false: that much LDS is not available.
template <auto KERN>
inline bool precise_raise_lds_limit(size_t lds) {
    static size_t set_dev[SC2_MAX_DEVICES] = {};
    size_t &have = set_dev[sc2_device_slot()];
    if (have < lds) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        have = lds;
    }
    return true;
}

}  // namespace
