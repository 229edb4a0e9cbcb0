/*
 * sc2_bottleneck.h -- C-ABI of libsc2amd.so, the MI355X (gfx950) implementation of the
 * supervised-compression bottleneck hot path of sc2bench.
 *
 * The reference has no FFI of its own: the path sits behind Python nn.Modules
 * (sc2bench/models/layer.py) that call CompressAI (Python + two pybind11
 * extensions) and torch's conv kernels.  Each entry point below names the
 * reference interface it replaces (file:line under the sc2bench tree, or the
 * CompressAI symbol the reference calls at that line).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  All device
 *    work is enqueued on it; nothing synchronises, nothing allocates.
 *  - every buffer is caller-allocated device memory unless marked HOST.
 *  - return value: 0 = success, negative = error (SC2_ERR_*).  No exceptions cross
 *    the boundary.  sc2_last_error() returns a thread-local message.
 *  - stateless and re-entrant.
 */
#ifndef SC2_BOTTLENECK_H
#define SC2_BOTTLENECK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC2_OK 0
#define SC2_ERR_INVALID_ARG (-1)
#define SC2_ERR_UNSUPPORTED (-2)
#define SC2_ERR_DOMAIN (-3)      /* pmf has a negative / non-finite entry (std::domain_error upstream) */
#define SC2_ERR_ZERO_PMF (-4)    /* pmf sums to zero */
#define SC2_ERR_LAUNCH (-5)      /* hip launch error */
#define SC2_ERR_NO_DEVICE (-6)
#define SC2_ERR_INTERNAL (-7)

/* ABI version: bumped on any signature change. */
#define SC2_ABI_VERSION 51
int sc2_abi_version(void);

/* ------------------------------------------------------------------------------------------ */
/* Dispatch policy.  Which kernel serves a launch is a function of the call's arguments and of  */
/* THIS struct -- the library reads no environment variable (round 5; rounds 1 - 4 steered ~27    */
/* choices through getenv).  The defaults are the measured choices; every   */
/* field exists for an A/B measurement or a diagnostic, and `tools/env_policy.py` is the only     */
/* place that maps SC2_* environment variables onto it.  The policy is process-wide             */
/* configuration: set it before issuing launches (sc2_policy_set copies the struct; concurrent    */
/* launches from other threads see either the old or the new value of each field).  The entry     */
/* points themselves stay re-entrant: no call reads or writes anything else that outlives it,     */
/* except per-device resource caches (unit counters, function attributes).                        */
/* ------------------------------------------------------------------------------------------ */
typedef struct sc2_policy {
    int32_t struct_bytes;        /* sizeof(sc2_policy) of the caller's header (sc2_policy_default sets it; _set checks it) */
    /* sc2_conv2d_fwd */
    int32_t conv_patch3;         /* window staging of stride-1 slab-major layers: 0 off, 1 = 3x3 on the 128-wide tile (default), 256 = also the 256-wide tile, 2 = also the 2x2 decoder layers */
    int32_t conv_s2;             /* static 3x3 stride-2 tile: 0 off, 1 (default) 256-wide where it wins, 128 / 256 force */
    int32_t conv_persist;        /* persistent 8-wave decoder tile (conv_dec_persist): 0 off, 1, 2, 3 (default: one phase per slab) */
    int32_t conv_half;           /* 1: half-width static decoder tiles (A/B; default 0) */
    int32_t conv_big4;           /* 1: the 4-wave register-tile kernel for the 256-channel layers (A/B; default 0) */
    int32_t conv_no_big;         /* 1: never the 8-wave 256-row tile */
    int32_t conv_force_big;      /* 1: the 8-wave tile wherever Cout allows (tests) */
    int32_t conv_no_epx;         /* 1: no epilogue-operand prefetch instantiations */
    int32_t conv_debug;          /* development: bit 0 skips the store epilogue, bit 1 the K loop (results garbage) */
    int32_t conv_chunk;          /* conv_dec_persist: tiles per claim (0 = default 2) */
    /* window-plane kernels */
    int32_t w2_run;              /* conv2x2_win: tiles per workgroup run (0 = default: min(share, 2)) */
    int32_t win_half;            /* conv3x3_win: half tiles, two workgroups per CU (default 1) */
    int32_t win_dbg;             /* conv3x3_win 14 x 14: timing experiments (results garbage; -DSC2_EXPERIMENTS builds only; default 0) */
    int32_t win_stamps;          /* conv3x3_win: 1 = per-workgroup wall-clock summary on stderr (diagnostic) */
    int32_t p1_half;             /* conv1x1_win: 112-pixel tiles (default 0) */
    int32_t p1_nbuf;             /* conv1x1_win: LDS ring depth 2 / 4 (0 = by shape) */
    int32_t pair_alt;            /* conv1x1_pair: alternate the traversal direction between launches (default 1) */
    /* reference-precision encoder, decoder head, training */
    int32_t f32_persist0;        /* conv_f32: the persistent first stage (default 1) */
    int32_t dec_stagger;         /* conv2x2_gdn512: stagger workgroup starts (A/B; default 0) */
    int32_t wgrad_wgs;           /* conv_wgrad: target workgroup count (0 = default 1024) */
    /* range coder */
    int32_t rans_lds_pad_kb;     /* small coder launches ask for this much LDS so that nothing shares their CU (default 159; 0 off) */
    int32_t rans_pad_waves;      /* ... launches of up to this many serial waves (default 16) */
    int32_t rans_ragged2;        /* four-lanes-per-stream decoder for per-symbol CDF rows (default 1) */
    int32_t rans_ragged2_waves;  /* ... waves per workgroup sharing one table copy: 0 (default) = 1 below 1 024 streams per launch, 2 from there; 1, 2, 4, 8 force */
    int32_t rans_lut8;           /* 1: one-lookup bucketed decode tables for implicit CDF rows (default 0: measured 6 % SLOWER than the two-lookup decoder) */
    int32_t rans_dq_lds;         /* 1: the dequantising last pass of a decode launch through LDS for every channel count (default 0: <= 32 channels transpose in registers, no LDS: fits beside the persistent kernels) */
    int32_t wgrad_ct;            /* conv_wgrad: 0 (default) = 256-channel tiles for layers with more than 128 output channels, 64-channel tiles for 64 or fewer; 128 = always the 128 x 128 tile (A/B) */
    int32_t reserved[6];
} sc2_policy;
void sc2_policy_default(sc2_policy *p);
int sc2_policy_set(const sc2_policy *p);      /* SC2_ERR_INVALID_ARG if p is NULL or struct_bytes != sizeof(sc2_policy) */
void sc2_policy_get(sc2_policy *p);
const char *sc2_last_error(void);
/* number of visible HIP devices (0 on a CPU-only box); never throws. */
int sc2_device_count(void);

/* ------------------------------------------------------------------------------------------ */
/* Layout conversion                                                                          */
/* ------------------------------------------------------------------------------------------ */
/* x: f32 NCHW [N,C,H,W]  ->  y: bf16 NHWC [N,H,W,Cpad] (channels c>=C zero-filled).
 * Replaces the implicit layout of the tensor handed to nn.Conv2d at layer.py:475. */
int sc2_nchw_f32_to_nhwc_bf16(const float *x, void *y, int N, int C, int H, int W, int Cpad, void *stream);
/* x: bf16 NHWC [N,H,W,C] -> y: f32 NCHW [N,C,H,W] (what a reference caller sees). */
int sc2_nhwc_bf16_to_nchw_f32(const void *x, float *y, int N, int C, int H, int W, void *stream);
/* Workgroups along x of both conversions' grids for `pixels` = N H W (y = the channel groups): min(ceil(pixels / 256), 16 384), each
 * thread striding over the pixels; 0 for pixels <= 0.  What the launchers use, exported for the tests' restated launch arithmetic. */
long long sc2_layout_blocks(long long pixels);

/* AdaptiveAvgPool2d((1,1)) + flatten of a bf16 NHWC feature map [N, HW, C] (torchvision ResNet.avgpool,
 * sc2bench/models/backbone.py:250-252): mean over HW in f32 -> y_f32 [N, C] and / or y_bf16 [N, C] (either may be NULL). */
int sc2_avgpool_nhwc(const void *x, float *y_f32, void *y_bf16, int N, int HW, int C, void *stream);

/* nn.BatchNorm2d in TRAINING mode (batch statistics) on a bf16 NHWC map x [M = N H W][C], with the ReLU and the residual add of a
 * torchvision Bottleneck block folded in (stage 2 of the Entropic-Student recipe fine-tunes layer2 .. layer4 with their norm layers
 * training: configs/.../splitable_resnet50-fp-beta0.08_from_resnet50.yaml:231-295; sc2bench/models/backbone.py:235-254 runs the blocks).
 *   forward : y = relu?((x - mean) rstd gamma + beta (+ residual)); mean / biased variance over the M rows; running_mean / running_var
 *             (may both be NULL) take the momentum update with the UNBIASED variance, as torch; save_mean / save_rstd [C] for backward
 *             NaN propagates as in torch: the ReLU zeroes only where its operand is < 0 and the variance is clamped only where it is
 *             < 0, so one NaN in x makes that channel's save_mean, save_rstd, running statistics and every y of the channel NaN (never
 *             a channel of zeros), and the backward on them gives a NaN dx for the channel
 *   backward: dz = y ? dy * (y > 0) : dy (y = the forward's output when it applied the ReLU, else NULL); dgamma = sum dz xhat, dbeta =
 *             sum dz; dx = gamma rstd (dz - dbeta / M - xhat dgamma / M); dz (NULL, or bf16 like dx) = the residual operand's gradient
 *   gamma, beta, running_*, save_*, dgamma, dbeta : f32 [C];  ws : f32 scratch of sc2_bn_ws_floats(M, C) floats (per-workgroup partial
 *   sums + coefficient rows; either direction);  C % 8 == 0, C <= 2048 */
long long sc2_bn_ws_floats(long long M, int C);
int sc2_bn_train_fwd(const void *x, const void *residual, const float *gamma, const float *beta, float *running_mean, float *running_var,
                     float momentum, float eps, int relu, void *y, float *save_mean, float *save_rstd, float *ws, long long M, int C,
                     void *stream);
int sc2_bn_train_bwd(const void *dy, const void *x, const void *y, const float *gamma, const float *save_mean, const float *save_rstd,
                     void *dx, void *dz, float *dgamma, float *dbeta, float *ws, long long M, int C, void *stream);

/* nn.MaxPool2d (floor mode, no dilation) on a bf16 NHWC map: x [N,H,W,C] -> y [N,OH,OW,C], C % 8 == 0 (torchvision ResNet.maxpool
 * behind the stem, sc2bench/models/backbone.py:235-254 via torchvision's resnet forward; the teacher of the training step and the
 * input-compression classifier run it).  Bit-identical to torch's kernel: same update rule, NaN propagates. */
int sc2_maxpool_nhwc(const void *x, void *y, int N, int H, int W, int C, int KH, int KW, int stride_h, int stride_w, int pad_h, int pad_w,
                     void *stream);

/* Classifier on the pooled features: out[m][n] = sum_k a[m][k] w[n][k] + bias[n] (torchvision ResNet.fc behind the pool,
 * sc2bench/models/backbone.py:247-253).  K split over the four waves of a workgroup, operands straight from L2.
 *   a : bf16 [M,K] (sc2_avgpool_nhwc's y_bf16), K % 128 == 0;   w_frag : bf16 fragment blocks [Npad/16][K/32][64][8] of the
 *   [Npad,K] weight (rows >= N zero; hip.pack_weight_fragments);   bias : f32 [Npad];   out : f32 [M,Npad], Npad % 16 == 0. */
int sc2_fc_fwd(const void *a, const void *w_frag, const float *bias, float *out, int M, int K, int Npad, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Implicit-GEMM convolution on the matrix cores (bf16 in, f32 accumulate)                    */
/* Replaces nn.Conv2d(bias=False) at layer.py:475-476,479-480,482-483 (encoder) and            */
/* 485-486,489-490,492-493 (decoder); with a_op/epilogue set, CompressAI GDN1.forward at       */
/* layer.py:478,481,488,491 (norm = conv2d(|x|, gamma 1x1, beta); y = x/norm or x*norm).       */
/* ------------------------------------------------------------------------------------------ */
enum sc2_conv_aop { SC2_AOP_NONE = 0, SC2_AOP_ABS = 1,
                    SC2_AOP_SQUARE = 2 /* x^2: the operand of CompressAI GDN (squared form), compressai.layers.GDN.forward */ };
enum sc2_conv_epilogue {
    SC2_EPI_NONE = 0,
    SC2_EPI_GDN = 1,  /* y = ep_x / (ep_beta[c] + acc)   (GDN1, inverse=False) */
    SC2_EPI_IGDN = 2, /* y = ep_x * (ep_beta[c] + acc)   (GDN1, inverse=True)  */
    SC2_EPI_BIAS = 3, /* y = acc + ep_beta[c]            (conv + bias / folded BN) */
    SC2_EPI_BIAS_RELU = 4,     /* y = relu(acc + ep_beta[c]) */
    SC2_EPI_BIAS_ADD_RELU = 5, /* y = relu(acc + ep_beta[c] + ep_x) (residual add) */
    /* conv FOLLOWED BY GDN1 in one launch where one tile holds every channel of a pixel: Cout in {32,48,64,96}, or
     * Cout == 256 on the 256-wide big-tile path (sc2_conv_fused_gdn_supported tells):
     * x = acc; y = x / (ep_beta + gamma |x|)  resp.  x * (ep_beta + gamma |x|).  `ep_x` carries the packed bf16
     * gamma matrix instead of an activation, in the layout sc2_conv_fused_gdn_supported reports. */
    SC2_EPI_FUSED_GDN = 6,
    SC2_EPI_FUSED_IGDN = 7,
    SC2_EPI_BIAS_LEAKY_RELU = 8, /* y = leaky_relu(acc + ep_beta[c], 0.01) (nn.LeakyReLU() default slope; h_a / h_s) */
    /* CompressAI GDN (squared form; bmshj2018_factorized g_a / g_s, reached from sc2bench/models/registry.py:73-80): with
     * a_op = SC2_AOP_SQUARE and the 1x1 gamma GEMM, acc = gamma x^2 */
    SC2_EPI_GDN2 = 9,  /* y = ep_x * rsqrt(ep_beta[c] + acc)   (GDN, inverse=False) */
    SC2_EPI_IGDN2 = 10, /* y = ep_x * sqrt(ep_beta[c] + acc)    (GDN, inverse=True)  */
    /* (sc2_conv2d_f32_fwd / sc2_conv2d_split_fwd take GDN2 as y = ep_x * (1.0f / sqrtf(ep_beta[c] + acc)), both operations
     *  correctly rounded: see there) */
    /* sc2_gdn1_bwd_gemm only (round 5): the two GEMMs of the GDN1 backward with its element-wise halves in their epilogues.
     * n = ep_beta[c] + acc (acc = gamma |x|, a_op ABS), g = the gradient at the GDN's output, x = its input: */
    SC2_EPI_GDN1_BWD_PRE = 11,   /* ep_x = g, ep_x2 = x:  y2 = g / n (direct term),  y = -y2 * x / n  (d_norm) */
    SC2_EPI_IGDN1_BWD_PRE = 12,  /* ep_x = g, ep_x2 = x:  y2 = g * n,                y = g * x         (d_norm) */
    SC2_EPI_GDN1_BWD_POST = 13   /* acc = gamma^T d_norm, ep_x = direct term, ep_x2 = x:  y = ep_x + sign(x) * acc  (= dL/dx) */
};
enum sc2_conv_out { SC2_OUT_BF16_NHWC = 0, SC2_OUT_F32_NCHW = 1, SC2_OUT_F32_NHWC = 2,
                    /* int32 NCHW symbols round_half_even(acc - ep_beta[c]) (ep_beta = the entropy bottleneck's medians,
                     * epilogue NONE): the last encoder conv followed by EntropyModel.quantize(.., 'symbols') in one
                     * launch (layer.py:482-483 + :506), bit-identical to sc2_conv2d_fwd(F32_NCHW) + sc2_eb_symbols */
                    SC2_OUT_I32_NCHW_SYM = 3 };
/* Order of the K axis of the packed weights (and of the kernel's walk over the input):
 *   TAP_MAJOR  k = (kh*KW + kw)*Cin + ci                       (default)
 *   SLAB_MAJOR k = ((ci/32)*KH*KW + kh*KW + kw)*32 + ci%32     (Cin % 32 == 0): the taps of one 32-channel slab are
 *              consecutive, so the overlapping pixels they re-read stay in L1/L2 (measured 4x fewer fabric reads on
 *              the 2x2 decoder convs). */
enum sc2_conv_k_order { SC2_K_TAP_MAJOR = 0, SC2_K_SLAB_MAJOR = 1,
                        /* flag, OR-ed in: w_packed is [Kpad/32][Cout_pad][32] (the B tile of one 32-deep k-slab is
                         * contiguous) instead of [Cout_pad][Kpad] */
                        SC2_K_B_TILE_MAJOR = 2,
                        /* flag, with SLAB_MAJOR only: w_packed is MFMA-fragment-major [Kpad/32][Cout_pad/16][64][8], entry
                         * (kt, jt, lane = fq*16 + frow, e) = W[jt*16 + frow][kt*32 + fq*8 + e]; taken by the LDS-patch
                         * kernel of the 5x5 stride-2 geometry (sc2_conv_patch_supported) */
                        SC2_K_B_FRAG_MAJOR = 4 };

typedef struct sc2_conv_desc {
    int32_t N, H, W, Cin;          /* input  : bf16 NHWC [N,H,W,Cin], Cin % 8 == 0              */
    int32_t Cout;                  /* output channels, Cout % 8 == 0                             */
    int32_t KH, KW;                /* filter taps                                                */
    int32_t stride_h, stride_w;
    int32_t pad_h, pad_w;
    int32_t OH, OW;                /* output spatial size (caller computes, library validates)   */
    int32_t a_op;                  /* enum sc2_conv_aop: transform applied to the input on load  */
    int32_t epilogue;              /* enum sc2_conv_epilogue                                     */
    int32_t out_format;            /* enum sc2_conv_out                                          */
    int32_t Kpad;                  /* row pitch (elements) of the packed weights, % 64 == 0      */
    int32_t Cout_pad;              /* rows of the packed weight matrix (>= Cout, % 128 == 0 or
                                      == tile width; see sc2_conv_weight_rows.  The squared-form
                                      GDN (SC2_AOP_SQUARE with SC2_EPI_GDN2 / SC2_EPI_IGDN2) has
                                      128-row tiles only: with Cout <= 96 it takes gamma zero-padded
                                      to Cout_pad = 128 rows)                                     */
    /* Output scatter, for the data gradient of a strided conv (one launch per stride-parity class).  out_H == 0:
     * dense output [N,OH,OW,Cout].  Otherwise OH/OW are taken as given (rows past the symmetric-padding formula
     * see implicit zeros) and output pixel (oh, ow) is written to (oh*out_stride_h + out_off_h,
     * ow*out_stride_w + out_off_w) of an NHWC tensor [N,out_H,out_W,Cout]; pixels outside it are dropped. */
    int32_t out_H, out_W, out_stride_h, out_stride_w, out_off_h, out_off_w;
    int32_t k_order;               /* enum sc2_conv_k_order */
    /* filter dilation (0 or 1 = none), sc2_conv2d_fwd only: tap (kh, kw) reads input pixel (oh*stride_h - pad_h + kh*dil_h, ..);
     * OH = (H + 2 pad_h - dil_h (KH - 1) - 1) / stride_h + 1.  The atrous layers of the dense-prediction models
     * (sc2bench/models/segmentation/deeplabv3.py ASPP rates 12 / 24 / 36; torchvision's `replace_stride_with_dilation` layer3 /
     * layer4): Cout > 96, plain epilogues (NONE / BIAS / BIAS_RELU / BIAS_ADD_RELU / GDN / IGDN), dense output. */
    int32_t dil_h, dil_w;
} sc2_conv_desc;

/* Rows the packed weight buffer must have for a given Cout (zero rows beyond Cout). */
int sc2_conv_weight_rows(int Cout);
/* Row pitch (elements) the packed weight buffer must have for K = KH*KW*Cin. */
int sc2_conv_weight_pitch(int K);

/* w_packed: bf16 [Cout_pad][Kpad], element (co, (kh*KW+kw)*Cin + ci); zero padded.
 * ep_x   : bf16 NHWC [N,OH,OW,Cout] for GDN/IGDN/ADD epilogues (NULL otherwise)
 * ep_beta: f32 [Cout] for GDN/IGDN/BIAS epilogues (NULL otherwise)
 * y      : per out_format. */
/* Non-zero if SC2_EPI_FUSED_GDN / _IGDN is available for this geometry (all of `d` filled in as for sc2_conv2d_fwd):
 * 1 = `ep_x` carries gamma as packed rows [sc2_conv_weight_rows(Cout)][sc2_conv_weight_pitch(Cout)] (tiles of
 * 32..96 channels); 2 = `ep_x` carries gamma as MFMA-fragment blocks [Cout/16][Cout/32][64][8], entry (jt, ks,
 * lane = fq*16 + frow, e) = gamma[jt*16 + frow][ks*32 + fq*8 + e] (the 256-wide 8-wave tile). */
int sc2_conv_fused_gdn_supported(const sc2_conv_desc *d);
/* 1 if this geometry runs on the LDS-resident-patch kernel (5x5 stride 2 pad 2, Cin 96 -> Cout 48, OW <= 64, bf16 NHWC
 * output: the second encoder conv, layer.py:479-480), which takes SC2_K_SLAB_MAJOR | SC2_K_B_FRAG_MAJOR weights. */
int sc2_conv_patch_supported(const sc2_conv_desc *d);
int sc2_conv2d_fwd(const sc2_conv_desc *d, const void *x, const void *w_packed, void *y,
                   const void *ep_x, const float *ep_beta, void *stream);

/* The two channel-mixing GEMMs of the GDN1 / inverse-GDN1 BACKWARD (CompressAI GDN1 under autograd, reached by loss.backward() for
 * sc2bench/models/layer.py:478,481,488,491) with the element-wise halves of that backward fused into their epilogues
 * (SC2_EPI_GDN1_BWD_PRE / SC2_EPI_IGDN1_BWD_PRE / SC2_EPI_GDN1_BWD_POST): a 1x1 "conv" (d: KH = KW = 1, stride 1, no padding,
 * Cin == Cout == C in {96, 256, 512, ...: packed rows 96 or a multiple of 128}, bf16 NHWC output) that reads TWO per-element
 * operands and, for the PRE forms, writes TWO outputs.  Replaces, per GDN layer, the norm GEMM + sc2_gdn_bwd_pre and the
 * gamma^T GEMM + sc2_gdn_bwd_post (nine passes over [pixels x C] tensors instead of fifteen).
 *   x : bf16 [M, C] the GEMM's operand (PRE: the GDN input, a_op ABS; POST: d_norm);  w_packed : gamma resp. gamma^T, packed as for
 *   sc2_conv2d_fwd;  ep_x, ep_x2 : bf16 [M, C];  ep_beta : f32 [C] (PRE; ignored by POST);  y, y2 : bf16 [M, C] (y2: PRE only). */
int sc2_gdn1_bwd_gemm(const sc2_conv_desc *d, const void *x, const void *w_packed, void *y, void *y2, const void *ep_x,
                      const void *ep_x2, const float *ep_beta, void *stream);

/* GDN1 / inverse GDN1 over C = 96, 256 or 512 channels with the whole channel row of a pixel tile resident in LDS (gdn512_rows.hip: 128-pixel
 * tiles, C = 256 / 512; gdn96_strips.hip: 32-pixel strips per wave, C = 96) -- the training-time forms of the first encoder normalisation
 * and the decoder's two (sc2bench/models/layer.py:476-477, 486-491; forward in train mode keeps its input
 * for the backward, which loss.backward() of script/task/image_classification.py:79 reaches):
 *   sc2_gdn1_rows_fwd : y = x * (beta + gamma |x|)  (inverse != 0)  or  x / (...);  x, y bf16 [M, C]
 *   sc2_gdn1_rows_bwd : given x and the gradient gy of y, BOTH GEMMs of the backward and its element-wise halves in one launch:
 *                       d_norm (bf16 [M, C]: its column sums are d_beta, d_norm^T |x| is d_gamma) and dx (bf16 [M, C]).
 *                       Same quantities as SC2_EPI_(I)GDN1_BWD_PRE + SC2_EPI_GDN1_BWD_POST of sc2_gdn1_bwd_gemm, the direct term kept
 *                       in f32 in the accumulators instead of rounded to bf16 in between; sign(0) = 0 as torch.abs's gradient.
 *                       d_beta (f32 [C] or NULL): the column sums of d_norm -- accumulated inside the launch for C = 96 / 256 (from
 *                       the f32 values, before their rounding to bf16), by sc2_colsum_bf16 behind it for C = 512.
 *   gamma_frag / gamma_t_frag : the effective gamma [C, C] and its transpose as MFMA fragments, bf16 [C/16][C/32][64][8]: entry
 *                       (jt, ks, lane = fq*16 + frow, e) = W[jt*16 + frow][ks*32 + fq*8 + e];  beta f32 [C];  M * C * 2 < 2 GB. */
int sc2_gdn1_rows_supported(int C);
int sc2_gdn1_rows_fwd(const void *x, const void *gamma_frag, const float *beta, void *y, long long M, int C, int inverse,
                      void *stream);
int sc2_gdn1_rows_bwd(const void *x, const void *gy, const void *gamma_frag, const void *gamma_t_frag, const float *beta,
                      void *d_norm, void *dx, float *d_beta, long long M, int C, int inverse, void *stream);
/* their launch geometry: tiles of 128 pixels (C = 256 / 512) or strips of 32 pixels (C = 96) that M pixels make, and the persistent
 * workgroups that share them: min(tiles, CUs), or min(ceil(strips / 8), CUs) workgroups of eight one-strip waves; 0 for dims the
 * launchers refuse. */
long long sc2_gdn1_rows_units(long long M, int C);
long long sc2_gdn1_rows_workgroups(long long M, int C);
/* column sums of a bf16 [M, C] tensor in f32 (d_beta = sum over pixels of d_norm): out f32 [C], C % 8 == 0, C <= 2048. */
int sc2_colsum_bf16(const void *x, long long M, int C, float *out, void *stream);
/* its grid: min(ceil(M / (1024 / (C / 8))), 256) workgroups of 1 024 threads, four pixels per thread and iteration; 0 for dims the
 * launcher refuses. */
long long sc2_colsum_blocks(long long M, int C);

/* Two consecutive 1x1 layers of the ResNet tail across a block boundary in ONE launch (torchvision Bottleneck blocks b and
 * b + 1 of layer2, eval mode, BatchNorm folded; sc2bench/models/backbone.py:235-254 runs them one after the other):
 *     h = relu(W3 o + b3 + identity)      conv3 + bn3 + residual + ReLU of block b        (K1 -> C)
 *     u = relu(W1 h + b1)                 conv1 + bn1 + ReLU of block b + 1               (C -> N2)
 * h is written once (it is the next block's identity) and feeds the second GEMM from LDS instead of being read again.
 *   o : bf16 [M][K1];  identity, h : bf16 [M][C];  u : bf16 [M][N2];  w3_frag : bf16 fragment-major [C/16][K1/32][64][8];
 *   w1_frag : bf16 fragment-major [N2/16][C/32][64][8] (hip.pack_weight_fragments);  b3 : f32 [C];  b1 : f32 [N2].
 * Supported: K1 = 128, C = 512, N2 = 128 (the block boundaries inside layer2 of ResNet-50) or 256 (layer2.3 -> layer3.0).  Bit-identical to sc2_conv1x1_stream_fwd (residual, relu)
 * followed by the 1x1 kernel of the next block. */
int sc2_conv1x1_pair_supported(int K1, int C, int N2);
int sc2_conv1x1_pair_fwd(const void *o, const void *w3_frag, const float *b3, const void *identity, void *h,
                         const void *w1_frag, const float *b1, void *u, long long M, int K1, int C, int N2, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Reference-precision analysis transform: the same convolution / GDN1 with f32 OPERANDS on the   */
/* f32 matrix cores (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered f32 fma chain), for callers   */
/* that need the symbols -- hence the byte streams -- the reference's f32 CPU path produces        */
/* (nn.Conv2d + compressai GDN1 in f32, sc2bench/models/layer.py:475-483, quantised at :506).      */
/* 1/16 of the bf16 matrix rate; `FPBasedResNetBottleneck.set_encoder_precision('f32')`; also the  */
/* hyperprior bottlenecks and the input codecs of compression.py (all four transforms there).      */
/* ------------------------------------------------------------------------------------------ */
/* x: f32 NCHW [N,C,H,W] -> y: f32 NHWC [N,H,W,Cpad], channels >= C zero, Cpad % 4 == 0. */
int sc2_nchw_f32_to_nhwc_f32(const float *x, float *y, int N, int C, int H, int W, int Cpad, void *stream);
/* Output channels per weight chunk for a given Cout (32, 48 or 96): the packing unit of w_frag below. */
int sc2_conv_f32_chunk_channels(int Cout);
/* d      : as for sc2_conv2d_fwd; Cin % 4 == 0 (the padded channel count of x), square stride (stride_h == stride_w), pad_h and
 *          pad_w each >= 0 and independent; Cout_pad / k_order are ignored.  Kpad: 0, or the number of REAL input channels: Cin == 4 with Kpad == 3 says that
 *          channel 3 of x is zero and zero-weighted (the layout sc2_nchw_f32_to_nhwc_f32 and the packer produce for RGB), and
 *          the kernel skips those products (same sums: they are exact zeros).  With that, k_order == 1 says that x is the f32 NCHW image
 *          [N, 3, H, W] itself (the reference's input layout): the three channel planes are read in place, no NHWC copy.  a_op: NONE / ABS / SQUARE.  epilogue: NONE, BIAS, GDN (y = ep_x * (1 /
 *          (ep_beta[c] + acc))), IGDN (y = ep_x * (ep_beta[c] + acc)) -- the operation order of compressai GDN1.forward;
 *          FUSED_GDN / FUSED_IGDN (Cout <= 96): the conv followed by GDN1 over its own output in one launch, `ep_x` = the
 *          effective gamma as the w_frag of a 1x1 conv Cout -> Cout (same packing), ep_beta = the effective beta; bit-identical
 *          to the two launches.
 *          GDN2 / IGDN2 (compressai GDN, the squared form of the input codecs' g_a / g_s; a 1x1 launch with a_op = SQUARE, ep_x =
 *          the GDN's input, ep_beta = the effective beta): norm = acc + ep_beta[c], r = sqrtf(norm), y = ep_x * (1.0f / r) (GDN2)
 *          resp. y = ep_x * r (IGDN2) -- a correctly rounded f32 square root, a correctly rounded division and one multiply, no
 *          reciprocal-square-root approximation.  (Upstream calls torch.rsqrt, which is not bit-defined: its CPU vector path and
 *          its tail path differ on 0.57 % of random values; 1 / sqrt is reproducible and within an ulp of either.)  They need ep_x
 *          and ep_beta (SC2_ERR_INVALID_ARG otherwise), write SC2_OUT_F32_NHWC or SC2_OUT_F32_NCHW but not the symbols, and are
 *          refused with SC2_ERR_UNSUPPORTED together with output scatter.  There is no fused form of them: FUSED_* stays GDN1-only
 *          (the codecs' N is 128 or 192, above the 96-channel chunk).
 *          BIAS_RELU / BIAS_LEAKY_RELU (the activations of the hyperprior transforms h_a / h_s): on the f32 value v = acc
 *          (+ ep_beta[c]; ep_beta may be NULL: no bias), v > 0 ? v : 0 resp. v > 0 ? v : v * 0.01f -- torch's CPU forms, one f32
 *          multiply; any out_format but the symbols.
 *          Output scatter (out_H != 0), with the meaning sc2_conv2d_fwd gives the fields: OH / OW are taken as given (rows past the
 *          padding formula read implicit zeros) and output pixel (oh, ow) goes to (oh*out_stride_h + out_off_h, ow*out_stride_w +
 *          out_off_w) of y = f32 NHWC [N,out_H,out_W,Cout]; pixels outside it are dropped.  SC2_OUT_F32_NHWC only, with the
 *          epilogues NONE / BIAS / BIAS_RELU / BIAS_LEAKY_RELU: a transposed convolution is one such launch per stride-parity
 *          class (`HipConvTranspose2d.forward_nhwc_precise`).  Scatter with GDN / IGDN / GDN2 / IGDN2 / FUSED_*, with another out_format, or a
 *          stride_h != stride_w returns SC2_ERR_UNSUPPORTED.
 * x      : f32 NHWC [N,H,W,Cin]; addressed through a 32-bit buffer descriptor: N*H*W*Cin*4 (N*H*W*12 for the NCHW image) must be
 *          below 0x7FF00000 bytes (SC2_ERR_UNSUPPORTED otherwise -- about 445 images of the 96-channel 112 x 112 map; the host side
 *          runs larger batches as slices, `FPBasedResNetBottleneck._analysis_f32`)
 * w_frag : f32, [chunks][steps][NT][64 lanes][4] with cc = sc2_conv_f32_chunk_channels(Cout), NT = cc / 16, chunks =
 *          ceil(Cout / cc), steps = ceil(KH*KW*Cin / 16); entry (ch, s, nt, lane = q*16 + r, j) =
 *          W[ch*cc + nt*16 + r][k = 16 s + 4 q + j], k = (kh*KW + kw)*Cin + ci, zero beyond Cout / K.
 * ep_x   : f32 NHWC [N,OH,OW,Cout] for GDN / IGDN / GDN2 / IGDN2;  ep_beta : f32 [Cout] (beta, bias, or the medians for symbols)
 * y      : SC2_OUT_F32_NHWC [N,OH,OW,Cout] / SC2_OUT_F32_NCHW / SC2_OUT_I32_NCHW_SYM (round_half_even(acc - ep_beta[c])). */
int sc2_conv2d_f32_fwd(const sc2_conv_desc *d, const float *x, const float *w_frag, void *y, const float *ep_x,
                       const float *ep_beta, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Split-bf16 analysis transform: the same convolution / GDN1 with every f32 operand written as  */
/* a sum of n_parts bf16 numbers (hi = bf16_rne(x), lo = bf16_rne(x - hi), lo2 = bf16_rne(x - hi  */
/* - lo)) and the part products (i, j) with i + j <= n_parts - 1 accumulated in f32 on            */
/* v_mfma_f32_16x16x32_bf16: 3 products (n_parts 2) or 6 (n_parts 3) per k.  Each product is      */
/* exact in f32, so only the dropped products separate the result from an f32 convolution.        */
/* `FPBasedResNetBottleneck.set_encoder_precision('bf16x3' / 'bf16x6')`; csrc/conv_split.hip.     */
/* ------------------------------------------------------------------------------------------ */
/* Output channels per weight chunk for a given Cout (32, 48 or 96): the packing unit of w_frag below. */
int sc2_conv_split_chunk_channels(int Cout);
/* d       : as for sc2_conv2d_f32_fwd, but x is always f32 NHWC (k_order must be 0; Kpad / Cout_pad are ignored): Cin % 4 == 0,
 *           square stride, pad_h / pad_w independent.  a_op: NONE / ABS / SQUARE, applied to the f32 value before the split.
 *           epilogue: NONE, BIAS, BIAS_RELU, BIAS_LEAKY_RELU, GDN, IGDN, GDN2, IGDN2, FUSED_GDN / FUSED_IGDN (a_op NONE, Cout <= 96
 *           with ceil(Cout / 16) * 16 == the chunk width), in the operation order of sc2_conv2d_f32_fwd; the fused form is
 *           bit-identical to the two launches.  GDN2 / IGDN2: the rules of sc2_conv2d_f32_fwd word for word -- ep_x and ep_beta
 *           needed, the two f32 output formats but not the symbols, SC2_ERR_UNSUPPORTED with output scatter, no fused form
 *           (FUSED_* stays GDN1-only), sqrt and division correctly rounded.  Output scatter (out_H != 0): exactly as for sc2_conv2d_f32_fwd -- both kernels run one copy of
 *           the epilogue and of the descriptor rules (csrc/conv_precise.h).
 * n_parts : 2 or 3 (anything else: SC2_ERR_UNSUPPORTED); w_frag and gamma_frag must be packed for the same value.
 * x       : f32 NHWC [N,H,W,Cin], N*H*W*Cin*4 below 0x7FF00000 bytes (SC2_ERR_UNSUPPORTED otherwise)
 * w_frag  : bf16, [chunks][steps][n_parts][NT][64 lanes][8] with cc = sc2_conv_split_chunk_channels(Cout), NT = cc / 16, chunks =
 *           ceil(Cout / cc), steps = ceil(KH*KW*Cin / 32); entry (ch, s, part, nt, lane = q*16 + r, j) = part `part` of
 *           W[ch*cc + nt*16 + r][k = 32 s + 16 (j >> 2) + 4 q + (j & 3)], k = (kh*KW + kw)*Cin + ci, zero beyond Cout / K.
 * ep_x    : f32 NHWC [N,OH,OW,Cout] for GDN / IGDN / GDN2 / IGDN2 (NULL otherwise)
 * gamma_frag : FUSED_* only (NULL otherwise; unlike sc2_conv2d_f32_fwd, gamma does not travel in ep_x): the effective gamma as
 *           the w_frag of a 1x1 conv Cout -> Cout, same packing and n_parts
 * ep_beta : f32 [Cout] (beta, bias, or the medians for symbols)
 * y       : SC2_OUT_F32_NHWC [N,OH,OW,Cout] / SC2_OUT_F32_NCHW / SC2_OUT_I32_NCHW_SYM (round_half_even(acc - ep_beta[c])).
 * Unsupported geometry returns SC2_ERR_UNSUPPORTED. */
int sc2_conv2d_split_fwd(const sc2_conv_desc *d, int n_parts, const float *x, const void *w_frag, void *y, const float *ep_x,
                         const void *gamma_frag, const float *ep_beta, void *stream);

/* First decoder stage in ONE launch: y = GDN1_512(Conv2d(Cin -> 512, k2, s1, p1, bias=False)(x)) with the inverse
 * (multiplicative) or forward (divisive) normalisation: t = conv(x); y = t * (beta + gamma |t|) resp. t / (...).
 * Replaces decoder[0] + decoder[1] of FPBasedResNetBottleneck (sc2bench/models/layer.py:486-488); the 512-channel
 * intermediate never reaches HBM.
 *   x : bf16 NHWC [N,H,W,Cin], Cin in {8,16,24};   w_packed : bf16 [512][Kpad], Kpad = sc2_conv_weight_pitch(4*Cin)
 *   gamma_frag : effective gamma as bf16 MFMA-fragment blocks [32 channel tiles][16 k steps][64 lanes][8]: entry
 *                (jt, ks, lane = fq*16 + frow, e) = gamma[jt*16 + frow][ks*32 + fq*8 + e] (one operand fragment =
 *                1 KB contiguous);   beta : f32 [512] (effective beta)
 *   y : bf16 NHWC [N,H+1,W+1,512]
 *   t_out : NULL, or bf16 laid out like y (round 5, training): the conv output in front of the GDN, the tensor the GDN's backward
 *           needs (`_forward2train`, layer.py:529-533: decoder[0] + decoder[1] as this one launch); needs N*(H+1)*(W+1)*1024 B < 2^31 */
int sc2_conv2x2_gdn512_supported(int Cin, int Cout, int KH, int KW, int stride, int pad);
int sc2_conv2x2_gdn512_fwd(const void *x, const void *w_packed, int Kpad, const void *gamma_frag, const float *beta,
                           void *y, void *t_out, int N, int H, int W, int Cin, int inverse, void *stream);

/* First encoder stage in ONE persistent launch: y = GDN1_96(Conv2d(3 -> 96, k5, s2, p2, bias=False)(x)) on the
 * pixel-pair view of the image (replaces encoder[0] + encoder[1], sc2bench/models/layer.py:476-478).
 *   x_pairs : bf16 [N, H, W/2, 8] (two pixels x four channels, channel 3 zero: sc2_nchw_f32_to_nhwc_bf16 with c_pad 4)
 *   w_frag  : bf16 MFMA-fragment blocks [6][4][64][8] of the pair-packed weights W'[96][128], k = (kh*3 + t)*8 + dw*4 + c
 *   gamma_frag : bf16 fragment blocks [6][3][64][8] of the effective gamma;  beta : f32 [96]
 *   y : bf16 NHWC [N, OH, W/2, 96], OH = (H - 1)/2 + 1.   Any width: rows are cut into 112-pixel output segments.
 *   t_out : NULL, or bf16 laid out like y (round 5, training): the conv output in front of the GDN, the tensor the GDN's backward
 *           needs (`_forward2train`, layer.py:529-533: encoder[0] + encoder[1] as this one launch) */
int sc2_conv0_gdn96_supported(int Cin_pairs, int Cout, int W_pairs);
int sc2_conv0_gdn96_fwd(const void *x_pairs, const void *w_frag, const void *gamma_frag, const float *beta, void *y, void *t_out,
                        int N, int H, int W_pairs, int inverse, void *stream);
/* The same launch on the reference's own input: x_nchw = the f32 NCHW image batch [N, 3, H, W] that
 * `FPBasedResNetBottleneck.encoder` receives (sc2bench/models/layer.py:496-498), read where it lies -- the three colour planes
 * of a pixel pair are rounded to bf16 (round-to-nearest-even, as sc2_nchw_f32_to_nhwc_bf16 rounds) as the kernel stages them:
 * bit-identical to sc2_nchw_f32_to_nhwc_bf16(c_pad 4) + sc2_conv0_gdn96_fwd without the layout pass.  W even (an odd width
 * goes through the pair view, zero-padded by the caller); y : bf16 NHWC [N, OH, W/2, 96]. */
int sc2_conv0_gdn96_nchw_fwd(const float *x_nchw, const void *w_frag, const void *gamma_frag, const float *beta, void *y,
                             int N, int H, int W, int inverse, void *stream);

/* 1x1 convolution with a long K and the weights resident in registers (conv1 + bn1 + ReLU and the stride-2 downsample of
 * the ResNet tail's layer3 / layer4 in eval mode, sc2bench/models/backbone.py:235-254): y = act(x W^T + bias).
 * Cin = 1024: Cout % 128 == 0, Cout <= 2048;  Cin = 2048: Cout % 64 == 0, Cout <= 1024;  stride 1 or 2 (no padding).
 *   x : bf16 NHWC [N,H,W,Cin];  w_frag : bf16 fragment blocks [Cout/16][Cin/32][64][8] (BN folded);  bias : f32 [Cout];
 *   y : bf16 NHWC [N,OH,OW,Cout], OH = (H-1)/stride + 1;  relu != 0: ReLU. */
int sc2_conv1x1_kres_supported(int Cin, int Cout, int stride);
int sc2_conv1x1_kres_fwd(const void *x, const void *w_frag, const float *bias, void *y, int N, int H, int W, int Cin, int Cout,
                         int stride, int relu, void *stream);

/* The last encoder convolution of the FP bottleneck, Conv2d(48 -> Cout <= 32, k2, s1, p0, bias=False) (sc2bench/models/layer.py:482
 * `encoder[4]`; 48 -> 24 in every released configuration), as a streaming kernel without LDS (conv2x2_c48.hip): the two column
 * taps of a pixel are 96 contiguous NHWC channels, so the MFMA operand fragments are plain 16-byte loads; weights resident in
 * registers.  Results bit-identical to sc2_conv2d_fwd's.
 *   x : bf16 NHWC [N,H,W,48];   w_frag : bf16 fragment blocks [2][6][64][8] of the [32][192] matrix W[co][kh*96 + kw*48 + ci]
 *       (rows >= Cout zero; hip.pack_conv2x2_c48);   y : NCHW [N,Cout,H-1,W-1], f32 latent (symbols == 0) or int32 symbols
 *       round-half-even(acc - medians[co]) (symbols != 0: EntropyModel.quantize(..., 'symbols') fused, as SC2_OUT_I32_NCHW_SYM). */
int sc2_conv2x2_c48_supported(int H, int W, int Cin, int Cout);
int sc2_conv2x2_c48_fwd(const void *x, const void *w_frag, const float *medians, void *y, int N, int H, int W, int Cin, int Cout,
                        int symbols, void *stream);

/* 1x1 convolution + bias (+ residual) (+ ReLU) in the window-plane structure (conv1x1_win.hip): conv1 + bn1 + ReLU, conv3 + bn3 +
 * identity + ReLU and the downsample layers of the torchvision Bottleneck blocks behind the bottleneck
 * (sc2bench/models/backbone.py:235-254) where K is long and the layer is not HBM-bound.  Tiles of 208 output pixels x 128
 * channels, 64-channel slabs of the pixel operand as chunk planes in LDS, weights straight into registers.
 *   x : bf16 NHWC [N,H,W,Cin], Cin % 128 == 0;   y : bf16 NHWC [N,OH,OW,Cout], OH = (H-1)/stride + 1, Cout % 128 == 0, stride 1 | 2
 *   w_frag : bf16 [Cin/32][Cout/16][64][8] (BN folded), the k-step stream of sc2_conv3x3_win_fwd for a 1 x 1 kernel (same row
 *            permutation);   bias : f32 [Cout];   residual : bf16 [N,OH,OW,Cout] or NULL (added before the ReLU);   relu != 0: ReLU. */
int sc2_conv1x1_win_supported(int Cin, int Cout, int stride);
int sc2_conv1x1_win_fwd(const void *x, const void *w_frag, const float *bias, const void *residual, const void *mask, void *y, int N,
                        int H, int W, int Cin, int Cout, int stride, int relu, void *stream);

/* The same 1x1 convolution + bias (+ residual) (+ ReLU) on the eight-wave, 256-channel form of the window-plane structure
 * (conv1x1_w8.hip): the long-K layers that are plain compute-heavy GEMMs -- conv1 of layer3 / layer4, layer4's conv3 and the stride-2
 * downsample layers of the torchvision Bottleneck blocks behind the bottleneck (sc2bench/models/backbone.py:235-254).  Tiles of 224
 * output pixels x 256 channels, 128-channel slabs of the pixel operand as chunk planes in LDS, weights straight into registers,
 * at most one workgroup per CU, successive tiles' K loops joined.  Arguments as sc2_conv1x1_win_fwd (the SAME w_frag stream) without
 * `mask`; Cin % 128 == 0, Cout % 256 == 0, stride 1 | 2.  Results are bit-identical to sc2_conv1x1_win_fwd's. */
int sc2_conv1x1_w8_supported(int Cin, int Cout, int stride);
int sc2_conv1x1_w8_fwd(const void *x, const void *w_frag, const float *bias, const void *residual, void *y, int N, int H, int W,
                       int Cin, int Cout, int stride, int relu, void *stream);

/* 3x3 stride-1 pad-1 convolution + bias (+ ReLU) on 28 x 28 / 14 x 14 / 7 x 7 maps: conv2 + bn2 + ReLU of the torchvision
 * Bottleneck blocks of layer2 / layer3 / layer4 behind the bottleneck (sc2bench/models/backbone.py:235-254 runs them) at the
 * 224 x 224 operating point.  Tiles of 196 output pixels x 128 channels, zero-padded window planes in LDS, weights straight
 * into registers (conv3x3_win.hip).
 *   x : bf16 NHWC [N,H,W,Cin], H == W in {28, 14, 7}, Cin % 64 == 0;   y : bf16 NHWC [N,H,W,Cout], Cout % 128 == 0
 *   w_frag : bf16 [Cin/32 * 9][Cout/16][64][8] (BN folded): entry (kt = slab*9 + kh*3 + kw, tile t = 2 g + j, lane = fq*16 +
 *            frow, e) = W[32 g + 8 (frow / 4) + 4 j + frow % 4][slab*32 + fq*8 + e][kh][kw]   (the row permutation leaves
 *            every lane with eight consecutive output channels of a pixel);   bias : f32 [Cout];   relu != 0: ReLU. */
int sc2_conv3x3_win_supported(int H, int W, int Cin, int Cout);
int sc2_conv3x3_win_fwd(const void *x, const void *w_frag, const float *bias, const void *mask, void *y, int N, int H, int W, int Cin,
                        int Cout, int relu, void *stream);

/* The stride-2 form of the same kernel: conv2 + bn2 + ReLU of layer2.0 / layer3.0 / layer4.0 (3x3, stride 2, pad 1; torchvision
 * puts the stride on conv2), 56 -> 28, 28 -> 14, 14 -> 7 at the 224 x 224 operating point (sc2bench/models/backbone.py:235-254).
 * The window is stored in four parity classes so that the nine taps stay immediate offsets (conv3x3_win.hip, GeoS2).
 *   x : bf16 NHWC [N,H,W,Cin], H == W in {56, 28, 14}, Cin % 32 == 0;   y : bf16 NHWC [N,H/2,W/2,Cout], Cout % 128 == 0
 *   w_frag, bias, relu : as sc2_conv3x3_win_fwd. */
int sc2_conv3x3s2_win_supported(int H, int W, int Cin, int Cout);
int sc2_conv3x3s2_win_fwd(const void *x, const void *w_frag, const float *bias, void *y, int N, int H, int W, int Cin, int Cout,
                          int relu, void *stream);

/* The two MFMA-bound decoder convolutions of the FP / SHP / MSHP bottlenecks on the window-plane structure, with the
 * inverse GDN1 that follows the first one fused in (sc2bench/models/layer.py:489-493: Conv2d(512 -> 256, k2, p0) + GDN1(256,
 * inverse) and Conv2d(256 -> 256, k2, p1)); conv2x2_win.hip.  Results bit-identical to sc2_conv2d_fwd's.
 *   x : bf16 NHWC [N,H,W,Cin], Cin % 64 == 0, pad 0 (H, W >= 2) or 1;   y : bf16 NHWC [N,H+2pad-1,W+2pad-1,256]
 *       (W == 56 with pad 0 and W == 55 with pad 1 -- the 224 x 224 operating point -- run the static-geometry instantiation;
 *        every other width runs the same kernel over column segments of 55 output pixels: BASELINE configs 4 / 5)
 *   w_frag : bf16 [Cin/32 * 4 (+ 8 when fused)][16][64][8]: conv k-step kt = slab*4 + kh*2 + kw, then (fused) the 8 k-steps of
 *            the effective gamma [256][256] as a 1x1 layer; entry (kt, tile t = 2 g + j, lane = fq*16 + frow, e) =
 *            W[32 g + 8 (frow / 4) + 4 j + frow % 4][slab*32 + fq*8 + e][kh][kw]  (row permutation as sc2_conv3x3_win_fwd)
 *   fused != 0: y = GDN1(conv(x)) with beta f32 [256]; inverse != 0: x * (beta + gamma |x|), else x / (...).
 *   y_channels 256, y_channel0 0: y as above.  y_channels 512 (plain pad-1 convs only): y is bf16 NHWC [N,H+1,W+1,512] and this
 *   launch writes its channels [y_channel0, y_channel0 + 256), y_channel0 in {0, 256} -- the data gradient of the 512 -> 256 layer
 *   (loss.backward() of script/task/image_classification.py:79 through layer.py:489) is two such launches. */
int sc2_conv2x2_win_supported(int H, int W, int Cin, int Cout, int pad);
int sc2_conv2x2_win_fwd(const void *x, const void *w_frag, const float *beta, void *y, int N, int H, int W, int Cin, int pad,
                        int fused, int inverse, int y_channels, int y_channel0, void *stream);

/* The last decoder convolution (256 -> 256, k2, p1: 55 -> 56) with the two 1x1 layers of the caller that consume its output
 * fused behind it: conv1 + bn1 + ReLU (256 -> 128) and downsample conv + bn (256 -> 512, stride 2) of layer2.0 of the ResNet
 * tail (sc2bench/models/backbone.py:235-254 runs decoder then layer2; torchvision Bottleneck.forward).  The 411 MB
 * feature map between the bottleneck and the head is then never written (y == NULL) or written once and not read back.
 *   x : bf16 NHWC [N,55,55,Cin];   w_stream : bf16 [Cin/32*4 + 24][16][64][8] = the conv's k-steps, 8 k-steps of W1 (BN folded,
 *   rows 128..255 zero), 8 k-steps of Wds rows 0..255, 8 k-steps of Wds rows 256..511 (packing as sc2_conv2x2_win_fwd);
 *   bias1 f32 [128], bias_ds f32 [512] (folded BN);   y : bf16 NHWC [N,56,56,256] or NULL;
 *   o1 : bf16 NHWC [N,56,56,128] = relu(W1 y + bias1);   ods : bf16 NHWC [N,28,28,512] = Wds y[::2, ::2] + bias_ds.
 * Same operation order per element as the separate launches: bit-identical results. */
int sc2_conv2x2_win_tail_supported(int H, int W, int Cin);
int sc2_conv2x2_win_tail_fwd(const void *x, const void *w_stream, const float *bias1, const float *bias_ds, void *y, void *o1,
                             void *ods, int N, int H, int W, int Cin, void *stream);

/* Second encoder stage in ONE persistent launch: y = GDN1_48(Conv2d(96 -> 48, k5, s2, p2, bias=False)(x)) (replaces
 * encoder[2] + encoder[3], sc2bench/models/layer.py:479-481; inverse != 0: inverse GDN1).  W == 112 (the 224 x 224 operating
 * point) runs the static geometry, any other width the same kernel over 56-column output segments.
 *   x : bf16 NHWC [N, H, W, 96];   y : bf16 NHWC [N, (H - 1)/2 + 1, (W - 1)/2 + 1, 48]
 *   w_frag : the conv weights packed SC2_K_SLAB_MAJOR | SC2_K_B_FRAG_MAJOR ([k-step = slab*25 + tap][3][64][8] bf16)
 *   gamma_frag : bf16 fragment blocks [3][2][64][8] of the effective gamma [48][48 -> 64 zero-padded];  beta : f32 [48]
 *   t_out : NULL, or bf16 laid out like y (round 5, training): the conv output in front of the GDN, which the GDN's backward needs --
 *           `_forward2train` (layer.py:529-533) then runs encoder[2] + encoder[3] as this one launch. */
int sc2_conv2_gdn48_supported(int Cin, int Cout, int W);
int sc2_conv2_gdn48_fwd(const void *x, const void *w_frag, const void *gamma_frag, const float *beta, void *y, void *t_out, int N, int H,
                        int W, int inverse, void *stream);

/* Streaming 1x1 convolution with a short K and a wide N: y = act(x W^T + bias [+ residual]) in one persistent launch
 * (the HBM-bound 1x1 layers of the ResNet-50 tail behind the bottleneck, backbone.py:235-254: third conv of a
 * Bottleneck block with its residual add + ReLU, stride-2 downsample).
 *   x : bf16 NHWC [N,H,W,Cin], Cin in {128, 256};  w_frag : bf16 MFMA-fragment blocks [Cout/16][Cin/32][64][8], entry
 *   (jt, ks, lane = fq*16 + frow, e) = W[jt*16 + frow][ks*32 + fq*8 + e];  bias : f32 [Cout];  residual : bf16 NHWC
 *   [N,OH,OW,Cout] or NULL;  y : bf16 NHWC [N,OH,OW,Cout], OH = (H-1)/stride + 1;  Cout % 256 == 0; stride 1 or 2.
 *   (round 5: Cin also 64 and 512, Cout % 128 == 0.)  mask : NULL, or bf16 like y (sc2_conv1x1_stream_mask_supported: Cin 128 / 256,
 *   Cout % 256 == 0, stride 1, relu 0): y = mask > 0 ? x W^T + bias [+ residual] : 0 -- the layer is the data gradient of a Bottleneck
 *   block's conv1 and `mask` the previous block's output, whose ReLU gradient then needs no pass of its own (as sc2_conv1x1_win_fwd /
 *   sc2_conv3x3_win_fwd take it). */
int sc2_conv1x1_stream_supported(int Cin, int Cout, int stride);
int sc2_conv1x1_stream_mask_supported(int Cin, int Cout, int stride);
int sc2_conv1x1_stream_fwd(const void *x, const void *w_frag, const float *bias, const void *residual, const void *mask, void *y, int N,
                           int H, int W, int Cin, int Cout, int stride, int relu, void *stream);

/* Weight gradient of sc2_conv2d_fwd: dw[co][(kh*KW+kw)*Cin+ci] = sum over output pixels of gy * im2col(x).
 * Replaces the weight half of nn.Conv2d's backward (reached through loss.backward(), image_classification.py:79).
 *   x  : bf16 NHWC [N,H,W,Cin]      gy : bf16 NHWC [N,OH,OW,Cout]
 *   dw : f32 [Cout][KH*KW*Cin], overwritten (zeroed on the stream, then accumulated with f32 atomics)
 * Uses N,H,W,Cin,Cout,KH,KW,stride,pad,OH,OW and a_op (SC2_AOP_ABS: |x| operand, for GDN1's gamma) of the
 * descriptor; the other fields are ignored. */
int sc2_conv2d_wgrad(const sc2_conv_desc *d, const void *x, const void *gy, float *dw, void *stream);

/* Element-wise halves of the GDN1 backward (norm = beta + gamma|x|, y = x/norm or x*norm; all tensors bf16 NHWC
 * [M pixels][C], C % 8 == 0).  The channel-mixing halves are sc2_conv2d_fwd (gamma^T d_norm) and sc2_conv2d_wgrad.
 *   pre : d_norm, dx_direct out; d_beta f32[C] out (zeroed on the stream, then atomically accumulated)
 *   post: dx = dx_direct + sign(x) * t */
int sc2_gdn_bwd_pre(const void *gy, const void *x, const void *norm, long long M, int C, int inverse, void *d_norm,
                    void *dx_direct, float *d_beta, void *stream);
int sc2_gdn_bwd_post(const void *dx_direct, const void *x, const void *t, long long n_elements, void *dx, void *stream);
/* their grids (workgroups of 256 threads): pre min(ceil(M / (256 / (C / 8))), 1 024), two pixels per thread and iteration; post
 * min(ceil(n_elements / 8 / 256), 8 192), grid-stride; 0 for arguments the launchers refuse. */
long long sc2_gdn_bwd_pre_blocks(long long M, int C);
long long sc2_gdn_bwd_post_blocks(long long n_elements);

/* ------------------------------------------------------------------------------------------ */
/* Entropy bottleneck (factorised prior), filters fixed to (3,3,3,3) as sc2bench uses them     */
/* Replaces CompressAI EntropyBottleneck.forward called at layer.py:531 (and wrapper.py:238),  */
/* EntropyModel.quantize/dequantize at layer.py:545-547.                                       */
/* ------------------------------------------------------------------------------------------ */
#define SC2_EB_PARAM_STRIDE 64
/* Per-channel parameter block (f32[64]); "sp" = softplus(matrix), "th" = tanh(factor):
 *  [0..2]   sp(M0)[3x1]  [3..5]   b0[3]  [6..8]   th(f0)[3]
 *  [9..17]  sp(M1)[3x3]  [18..20] b1[3]  [21..23] th(f1)[3]
 *  [24..32] sp(M2)[3x3]  [33..35] b2[3]  [36..38] th(f2)[3]
 *  [39..47] sp(M3)[3x3]  [48..50] b3[3]  [51..53] th(f3)[3]
 *  [54..56] sp(M4)[1x3]  [57]     b4     [58]     median (quantiles[c,0,1])   [59..63] 0 */
enum sc2_eb_mode { SC2_EB_NOISE = 0, SC2_EB_DEQUANTIZE = 1 };

/* y        : f32 NCHW [N,C,HW]
 * noise    : f32 NCHW, same shape (mode NOISE: y_hat = y + noise; ignored otherwise; the caller
 *            draws U(-1/2,1/2) as the reference does with torch.empty_like().uniform_())
 * y_hat    : f32 NCHW out (nullable)
 * y_hat_bf16_nhwc : bf16 NHWC out, the decoder's input (nullable)
 * lik      : f32 NCHW out = max(sigmoid(L(y_hat+.5)) - sigmoid(L(y_hat-.5)), lik_bound) (nullable)
 * bits_partial : f32 [N*C*gridDim.y] partial sums of -log2(lik) (nullable; n_partial receives count)
 */
int sc2_eb_forward(const float *y, const float *noise, const float *params, int N, int C, int HW,
                   int mode, float lik_bound, float *y_hat, void *y_hat_bf16_nhwc, float *lik,
                   float *bits_partial, int bits_partial_len, void *stream);
/* number of partial sums sc2_eb_forward writes for this problem size */
int sc2_eb_bits_partial_len(int N, int C, int HW);

/* Backward of sc2_eb_forward (CompressAI EntropyBottleneck.forward under autograd, reached from the training loop
 * through layer.py:531) w.r.t. y and the effective parameter block.  Re-evaluates the forward from (y, noise).
 *   g_yhat, g_lik : upstream gradients, f32 NCHW (nullable = zero)
 *   g_y           : f32 NCHW out
 *   g_params_partial : f32 [n_partial][64] out, n_partial = sc2_eb_bits_partial_len(N, C, HW) rows ordered
 *                   (n, c, tile); the caller sums the rows of a channel.  Slot 58 is the median's gradient. */
int sc2_eb_backward(const float *y, const float *noise, const float *params, int N, int C, int HW, int mode,
                    float lik_bound, const float *g_yhat, const float *g_lik, float *g_y, float *g_params_partial,
                    int n_partial, void *stream);
/* planes (images) of one channel that a workgroup of sc2_eb_backward walks for this problem size: the largest of 8, 4, 2, 1
 * that divides N and leaves (N / it) * C >= 512 workgroups.  The workgroup's sums go to the first partial row of its first plane,
 * zeros to the other rows of its planes (rows per plane = sc2_eb_bits_partial_len(N, C, HW) / (N * C)). */
int sc2_eb_backward_planes_per_wg(int N, int C, int HW);

/* symbols = int32(round_half_even(y - median[c])) in NCHW order, one row of C*HW per image.
 * Replaces EntropyModel.quantize(x, "symbols", means) reached from layer.py:506. */
int sc2_eb_symbols(const float *y, const float *medians, int N, int C, int HW, int32_t *symbols, void *stream);
/* y_hat = float(symbols) + median[c]   (EntropyModel.dequantize reached from layer.py:520). */
int sc2_eb_dequantize(const int32_t *symbols, const float *medians, int N, int C, int HW, float *y_hat_f32_nchw,
                      void *y_hat_bf16_nhwc, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* GaussianConditional (hyperprior bottlenecks, sc2bench/models/layer.py:553-817)              */
/* Replaces CompressAI GaussianConditional.forward / quantize / dequantize / build_indexes     */
/* reached from layer.py:646-647,665,679,691-693,776,785,794,811-813.                          */
/* All tensors f32 NCHW with `chw` elements per image; `scales` / `means` may be channel       */
/* slices of a wider tensor and carry their own per-image element stride.                      */
/* ------------------------------------------------------------------------------------------ */
/* mode SC2_EB_NOISE: y_hat = y + noise (means ignored, as upstream); SC2_EB_DEQUANTIZE: y_hat = round(y - means) +
 * means.  lik = max(Phi((.5 - |v|)/s) - Phi((-.5 - |v|)/s), lik_bound), v = y_hat - means, s = max(scales,
 * scale_bound), Phi(t) = .5 erfc(-t / sqrt 2).  means, noise, y_hat, lik nullable. */
int sc2_gc_forward(const float *y, const float *scales, int64_t scales_img_stride, const float *means,
                   int64_t means_img_stride, const float *noise, int64_t n_img, int64_t chw, int mode,
                   float scale_bound, float lik_bound, float *y_hat, float *lik, void *stream);
/* Backward of sc2_gc_forward in SC2_EB_NOISE mode (GaussianConditional.forward under autograd in training, reached
 * from layer.py:679,794 through loss.backward()): g_yhat / g_lik upstream gradients (nullable = zero); g_y, g_scales,
 * g_means dense f32 [n_img][chw] outputs (each nullable).  noise nullable = zero. */
int sc2_gc_backward(const float *y, const float *scales, int64_t scales_img_stride, const float *means,
                    int64_t means_img_stride, const float *noise, int64_t n_img, int64_t chw, float scale_bound,
                    float lik_bound, const float *g_yhat, const float *g_lik, float *g_y, float *g_scales,
                    float *g_means, void *stream);
/* symbols = int32(round_half_even(y - means)); indexes = (n_table - 1) - #{t < n_table - 1 : max(scales,
 * scale_bound) <= scale_table[t]} (GaussianConditional.build_indexes).  Either output may be NULL. */
int sc2_gc_symbols_indexes(const float *y, const float *scales, int64_t scales_img_stride, const float *means,
                           int64_t means_img_stride, int64_t n_img, int64_t chw, const float *scale_table, int n_table,
                           float scale_bound, int32_t *symbols, int32_t *indexes, void *stream);
/* y_hat = float(symbols) + means (means nullable), f32 NCHW and / or bf16 NHWC [n_img, HW, C]. */
int sc2_gc_dequantize(const int32_t *symbols, const float *means, int64_t means_img_stride, int64_t n_img, int C,
                      int HW, float *y_hat_f32_nchw, void *y_hat_bf16_nhwc, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* CDF quantisation (HOST function, bit-exact integer result)                                  */
/* Replaces compressai._CXX.pmf_to_quantized_cdf reached from layer.py:431-441 (update()).     */
/* pmf: HOST f32[n]; cdf: HOST u32[n+1].                                                       */
/* ------------------------------------------------------------------------------------------ */
int sc2_pmf_to_quantized_cdf(const float *pmf, int n, int precision, uint32_t *cdf);

/* ------------------------------------------------------------------------------------------ */
/* rANS (64-bit state, 32-bit renormalisation, 16-bit precision, 4-bit bypass), one stream per */
/* image, all streams of a batch in one launch.  Bit-exact to CompressAI's                     */
/* RansEncoder.encode_with_indexes / RansDecoder.decode_with_indexes (layer.py:506,520).       */
/* ------------------------------------------------------------------------------------------ */
/* symbols : i32 [n_streams][n_sym]
 * indexes : i32 [n_streams][n_sym] CDF row per symbol, or NULL -> row = position / index_div
 *           (the entropy bottleneck's indexes[n,c,h,w] = c with index_div = H*W)
 * cdfs    : i32 [n_cdfs][cdf_stride];  cdf_sizes, offsets : i32 [n_cdfs]
 * out     : u8  [n_streams][out_stride]; stream i occupies
 *           out[i*out_stride + out_offset[i] .. + out_nbytes[i])  (streams are END-aligned in
 *           their rows because rANS emits its words back to front)
 * out_stride must be >= sc2_rans_max_bytes(n_sym); out_stride % 4 == 0.
 * status  : i32 [n_streams] 0 ok; bit 0 = row overflow (cannot happen with sc2_rans_max_bytes); bit 1 = a symbol with
 *           |symbol - offset| >= 2^30 was clamped (non-finite / diverged latent); decoders only: bit 3 = corrupt, truncated or
 *           hostile stream (an escape that announces more than the eight nibbles of a 32-bit value -- upstream's decoder
 *           loops on such a count for ever -- or words read past the end of the stream, where zeros are supplied): the
 *           decode always terminates, the symbols of a flagged stream are undefined.
 * workspace : device scratch of sc2_rans_workspace_bytes(n_streams, n_sym, n_cdfs, cdf_stride) bytes (the
 *             [position][lane] transposed intermediate of the multi-pass coder and the per-entry reciprocal
 *             table); contents undefined afterwards.
 */
int64_t sc2_rans_max_bytes(int64_t n_sym);
int64_t sc2_rans_workspace_bytes(int n_streams, int64_t n_sym, int n_cdfs, int cdf_stride);
int sc2_rans_encode_batch(const int32_t *symbols, const int32_t *indexes, int64_t index_div, int n_streams,
                          int64_t n_sym, const int32_t *cdfs, int n_cdfs, int cdf_stride,
                          const int32_t *cdf_sizes, const int32_t *offsets, uint8_t *out, int64_t out_stride,
                          int32_t *out_offset, int32_t *out_nbytes, int32_t *status, void *workspace,
                          int64_t workspace_bytes, void *stream);
/* in : u8 [n_streams][in_stride], stream i at in[i*in_stride + in_offset[i] ..+in_nbytes[i]),
 *      in_offset[i] % 4 == 0.  symbols_out : i32 [n_streams][n_sym]. */
int sc2_rans_decode_batch(const uint8_t *in, int64_t in_stride, const int32_t *in_offset, const int32_t *in_nbytes,
                          const int32_t *indexes, int64_t index_div, int n_streams, int64_t n_sym,
                          const int32_t *cdfs, int n_cdfs, int cdf_stride, const int32_t *cdf_sizes,
                          const int32_t *offsets, int32_t *symbols_out, int32_t *status, void *workspace,
                          int64_t workspace_bytes, void *stream);
/* sc2_rans_decode_batch for implicit indexes (row = position / index_div, n_sym == n_cdfs * index_div) with
 * EntropyModel.dequantize fused into its last pass (sc2bench/models/layer.py:520 `entropy_bottleneck.decompress` ->
 * dequantize(values, medians)): y_hat_bf16_nhwc[s][pix][c] = bf16(symbol[s][c * index_div + pix] + medians[c]), the layout the
 * synthesis kernels read (as sc2_eb_dequantize's y_hat_bf16_nhwc, same rounding).  symbols_out may be NULL (the int32 symbols
 * are then never written).  n_cdfs % 8 == 0, n_cdfs <= 64. */
int sc2_rans_decode_dequantize_batch(const uint8_t *in, int64_t in_stride, const int32_t *in_offset, const int32_t *in_nbytes,
                                     int64_t index_div, int n_streams, int64_t n_sym, const int32_t *cdfs, int n_cdfs,
                                     int cdf_stride, const int32_t *cdf_sizes, const int32_t *offsets, const float *medians,
                                     int32_t *symbols_out, void *y_hat_bf16_nhwc, int32_t *status, void *workspace,
                                     int64_t workspace_bytes, void *stream);

/* The same call; additionally records the caller's two hipEvent_t (may be NULL) on `stream` directly in front of and behind its
 * LAST pass (dequantise + transposition to NHWC = EntropyModel.dequantize, layer.py:520), so that a caller can time that pass
 * as part of the bottleneck forward while the serial passes count as the range coder's. */
int sc2_rans_decode_dequantize_batch_ev(const uint8_t *in, int64_t in_stride, const int32_t *in_offset, const int32_t *in_nbytes,
                                        int64_t index_div, int n_streams, int64_t n_sym, const int32_t *cdfs, int n_cdfs,
                                        int cdf_stride, const int32_t *cdf_sizes, const int32_t *offsets, const float *medians,
                                        int32_t *symbols_out, void *y_hat_bf16_nhwc, int32_t *status, void *workspace,
                                        int64_t workspace_bytes, void *stream, void *ev_dequantize_begin, void *ev_dequantize_end);

/* Which kernels a decode call of these sizes runs under the policy in force: the decision the decode entry points themselves
 * switch on (one host function, no launch, no device needed), exported so that a test knows which decoder its case reached.
 * explicit_indexes: the call passes `indexes`; fused_dq: it is sc2_rans_decode_dequantize_batch (with the sizes that call
 * accepts).  Returns the serial kernel (enum sc2_rans_dec_path), or 0 for sizes no decode call takes (n_streams <= 0,
 * n_sym < 0, n_cdfs <= 0, cdf_stride < 3, implicit indexes with index_div <= 0).  *waves (may be NULL): waves per workgroup
 * of SC2_RANS_DEC_RAGGED2 (1, 2, 4, 8), 1 for every other kernel.  *finish (may be NULL): the parallel pass behind the serial
 * kernel, enum sc2_rans_dec_finish -- for implicit indexes what a call that asks for y_hat (fused_dq) resp. symbols_out runs; a
 * fused call that also asks for symbols_out runs the transposition behind the dequantising pass; n_sym == 0 runs neither. */
enum sc2_rans_dec_path {
    SC2_RANS_DEC_LUT8 = 1,            /* one-lookup bucketed tables (policy rans_lut8), behind the table-building pre-pass */
    SC2_RANS_DEC_LUT_U8 = 2,          /* two-lookup decoder, byte-sized lookup table: rows of up to 257 entries */
    SC2_RANS_DEC_LUT_U16 = 3,         /* ... 16-bit lookup table: rows of up to 4 096 entries */
    SC2_RANS_DEC_RAGGED2 = 4,         /* explicit indexes, four lanes per stream: more than 12 288 table entries, at most 64 rows */
    SC2_RANS_DEC_RAGGED_8BIT = 5,     /* explicit indexes, one lane per stream, 256 buckets per row (policy rans_ragged2 = 0) */
    SC2_RANS_DEC_RAGGED_5BIT = 6,     /* ... 32 buckets per row: 65 - 256 rows */
    SC2_RANS_DEC_GENERIC_LDS = 7,     /* binary search on the rectangular table in LDS: at most 12 288 entries */
    SC2_RANS_DEC_GENERIC_GLOBAL = 8   /* ... on the table in global memory */
};
enum sc2_rans_dec_finish {
    SC2_RANS_FINISH_NONE = 0,         /* the serial kernel writes symbols_out itself (the generic kernels) */
    SC2_RANS_FINISH_TRANSPOSE = 1,    /* [position][lane] intermediate -> symbols_out */
    SC2_RANS_FINISH_DQ_REG = 2,       /* dequantise + NHWC transposition in registers: 8, 16, 24, 32 channels */
    SC2_RANS_FINISH_DQ_LDS = 3        /* ... through LDS: the other channel counts, or policy rans_dq_lds */
};
int sc2_rans_decode_path(int explicit_indexes, int64_t index_div, int n_streams, int64_t n_sym, int n_cdfs, int cdf_stride,
                         int fused_dq, int *waves, int *finish);

/* ------------------------------------------------------------------------------------------ */
/* Element-wise pieces of the distillation step (stage 1 of the Entropic-Student recipe:          */
/* nn.MSELoss(reduction='sum') between student and teacher feature maps, yaml:155-200; ReLU       */
/* gradients of the frozen ResNet tail, yaml:135), bf16 tensors of n elements, n % 8 == 0.         */
/* ------------------------------------------------------------------------------------------ */
/* partial : f32 [sc2_mse_partial_len(n)] block sums of (x - y)^2 (f32 accumulation, fixed order); the caller adds them. */
int sc2_mse_partial_len(long long n);
int sc2_mse_sum_bf16(const void *x, const void *y, long long n, float *partial, void *stream);
/* gx = bf16(2 * scale[0] * (x - y)); scale: DEVICE f32 scalar (the upstream gradient of the loss). */
int sc2_mse_grad_bf16(const void *x, const void *y, long long n, const float *scale, void *gx, void *stream);
/* gi = (g [+ add]) * (out > 0): gradient through a ReLU whose output was saved; `add` (nullable) = a second gradient that
 * reaches the same tensor, summed in f32 before the mask. */
int sc2_relu_bwd_bf16(const void *g, const void *out, const void *add, long long n, void *gi, void *stream);
/* ... with the feature-matching MSE term that sits on the same tensor folded in: g_in = ([g] + 2 * scale[0] * (out - t)) * (out > 0),
 * g may be NULL (no other gradient reaches the tensor).  `out` = the student's stack output the criterion compares with the teacher's
 * `t` (yaml:155-200: MSELoss(reduction='sum') per layer), scale = loss weight x upstream gradient [/ numel for 'mean'] as an f32 device
 * scalar; relu = 0: no activation behind the tensor (the bottleneck's own output: [g] + 2 scale (out - t)).  Replaces sc2_mse_grad_bf16 +
 * the add + sc2_relu_bwd_bf16 at the output of a frozen stack. */
int sc2_relu_bwd_mse_bf16(const void *g, const void *out, const void *t, const float *scale, long long n, int relu, void *gi, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* HOST range coder (same bit-exact format; every pointer is HOST memory, no HIP call is made).  */
/* For the reference's evaluation mode -- test batch size 1, ONE stream per forward               */
/* (script/task/image_classification.py:106-145 -> layer.py:506,520): a single rANS stream is a   */
/* serial chain that one CPU core steps ~30x faster than one GPU lane, so below a stream-count    */
/* threshold EntropyBottleneck / GaussianConditional .compress / .decompress call these instead   */
/* of the batched device coder.  Product code (csrc/rans_host.cpp), not the test oracle.          */
/* ------------------------------------------------------------------------------------------ */
/* Opaque prepared tables: per CDF row the cumulative frequencies and a 256-bucket index for the decoder's symbol
 * search.  cdfs : i32 [n_cdfs][cdf_stride], cdf_sizes / offsets : i32 [n_cdfs] as above.  SC2_ERR_INVALID_ARG if a row is
 * not a strictly increasing table from 0 to 65 536 with at least two entries. */
typedef struct sc2_rans_host_tables sc2_rans_host_tables;
int sc2_rans_host_tables_create(const int32_t *cdfs, int n_cdfs, int cdf_stride, const int32_t *cdf_sizes,
                                const int32_t *offsets, sc2_rans_host_tables **out);
void sc2_rans_host_tables_destroy(sc2_rans_host_tables *tables);
/* Both passes in one call: every stream is encoded into its row of `out` and that row decoded into symbols_out by the same host
 * thread (the first coder groups of a pipelined run: sc2bench_amd/pipeline.py `host_steps`); status = encode | decode bits. */
int sc2_rans_code_host(const sc2_rans_host_tables *tables, const int32_t *symbols, const int32_t *indexes, int64_t index_div,
                       int n_streams, int64_t n_sym, uint8_t *out, int64_t out_stride, int32_t *out_offset, int32_t *out_nbytes,
                       int32_t *symbols_out, int32_t *status, int n_threads);
/* floor(x / freq) as the host ENCODER forms it (a multiplication by freq's precomputed reciprocal, exact for x < 2^63: the
 * coder's state never leaves [2^31, 2^63)); exported so that a test can sweep it against the division (1 <= freq <= 65 536). */
uint64_t sc2_rans_host_rcp_div(uint64_t x, uint32_t freq);
/* Same arguments, row layout (END-aligned streams, out_offset / out_nbytes) and status bits as sc2_rans_encode_batch /
 * sc2_rans_decode_batch (additionally bit 2 = a CDF-row index outside the table); `out` / `in` 4-byte aligned;
 * streams are spread over n_threads host threads (<= 1: the calling thread). */
int sc2_rans_encode_host(const sc2_rans_host_tables *tables, const int32_t *symbols, const int32_t *indexes,
                         int64_t index_div, int n_streams, int64_t n_sym, uint8_t *out, int64_t out_stride,
                         int32_t *out_offset, int32_t *out_nbytes, int32_t *status, int n_threads);
int sc2_rans_decode_host(const sc2_rans_host_tables *tables, const uint8_t *in, int64_t in_stride,
                         const int32_t *in_offset, const int32_t *in_nbytes, const int32_t *indexes, int64_t index_div,
                         int n_streams, int64_t n_sym, int32_t *symbols_out, int32_t *status, int n_threads);

/* ------------------------------------------------------------------------------------------ */
/* Serial context-model scan of the joint autoregressive hierarchical prior (csrc/ar_context.hip).  */
/* ------------------------------------------------------------------------------------------ */
/* One workgroup per image walks the B x H x W latent in raster order over pixels [pix0, pix1); per pixel (all bf16 weights,
 * f32 activations, a fixed reduction order per output that does not depend on B):
 *   ctx = Wc . gather(y_hat_pad, the 12 causal taps of the 5x5 type-A mask) + bc          (12M -> 2M)
 *   h1  = lrelu(W1b . ctx + p1[pixel])      p1 = W1[:, :2M] . params + b1, computed before the scan (C1p wide)
 *   h2  = lrelu(W2 . h1 + b2)   gp = W3 . h2 + b3   scales = gp[:M], means = gp[M:]
 *   index = gc_symbols_indexes' table search on max(scale, scale_bound)
 *   symbol = rint(y - mean) (decode == 0: y is f32 NCHW)  or  the next symbol of the image's rANS stream (decode == 1)
 *   y_hat_pad[b][h+2][w+2][:] = symbol + mean;  y_hat_nhwc[b][h][w][:] = bf16 of it.
 * Weights are k-major bf16: wc [12M][2M] (k = tap * M + channel, taps in raster order), w1 [2M][C1p], w2 [C1p][C2p],
 * w3 [C2p][2M]; C1p, C2p multiples of 8 with zero padding.  y_hat_pad: f32 [B][H+2][W+4][M], zero outside the latent.
 * symbols / indexes: i32 [B][H*W*M], pixel-major, channel-minor (written by the encoder; the decoder writes symbols if non-NULL).
 * Decoder: stream b at buf[b*stride + io_offset[b] ..+ io_nbytes[b]) (io_offset % 4 == 0); its rANS state and read position
 * live in st_x / st_pos between calls (initialised when pix0 == 0), so a scan may be split into pixel ranges.  status[b]:
 * bit 3 = a corrupt or truncated stream (no word outside the stream is read), bit 4 = the stream did not end where the last
 * pixel ended (state != 2^31 or words left over).  All M <= 512, 2M and C1p / C2p <= 1280.  The decoder keeps the CDF rows in
 * LDS when they fit beside the step's vectors and searches them in device memory otherwise (same symbols either way).
 * sc2_ar_scan_f32: the same struct, the same step, checks and error codes, with wc / w1 / w2 / w3 read as `const float *`:
 * k-major F32 matrices of the shapes and zero padding above, each 8-byte aligned (a lane loads two adjacent outputs' weights as
 * one 8-byte value).  The products are then those of the unrounded f32 weights; the reduction order, the biases / p1, the table
 * search, rint, the decoder and the resumable state are shared code.  A stream decodes only with the weight form (and the weights)
 * that encoded it: one scale on the other side of a table boundary, or one mean that rounds y the other way, changes every
 * later pixel of the image. */
typedef struct sc2_ar_scan_args {
    int32_t B, H, W, M, C1p, C2p;
    int32_t n_table, n_cdfs, cdf_stride, pix0, pix1, decode;
    float scale_bound;
    int32_t cdf_entries;   /* decode: sum(cdf_sizes) - n_cdfs (the packed table's length) */
    int64_t stride;
    const void *wc, *bc, *w1, *p1, *w2, *b2, *w3, *b3;
    const float *scale_table;
    float *y_hat_pad;
    void *y_hat_nhwc;
    const float *y;
    int32_t *symbols, *indexes;
    const uint8_t *buf;
    const int32_t *io_offset, *io_nbytes;
    const int32_t *cdfs, *cdf_sizes, *offsets;
    uint64_t *st_x;
    int32_t *st_pos, *status;
    float *gaussian_params;   /* nullable: f32 [B][H*W][2M], each pixel's scales then means as the step computed them */
} sc2_ar_scan_args;
int sc2_ar_scan(const sc2_ar_scan_args *args, void *stream);
int sc2_ar_scan_f32(const sc2_ar_scan_args *args, void *stream);
/* Resumable rANS decoder (the scan's decoder as a kernel of its own): decodes n_sym symbols per stream with explicit per-symbol
 * indexes [n_streams][n_sym], continuing from st_x / st_pos / status unless `first` (then it starts at the stream's first word).
 * `last`: also check that the stream ends here (status bit 4).  Same stream layout and status bits as sc2_ar_scan, and bit 2 = an
 * index outside [0, n_cdfs) (row 0 is decoded in its place); bits 2 and 3 set by one call stay set in the calls that continue it. */
int sc2_rans_decode_resume(const uint8_t *buf, int64_t stride, const int32_t *io_offset, const int32_t *io_nbytes,
                           const int32_t *indexes, int n_streams, int64_t n_sym, const int32_t *cdfs, int n_cdfs,
                           int cdf_stride, const int32_t *cdf_sizes, const int32_t *offsets, int first, int last,
                           uint64_t *st_x, int32_t *st_pos, int32_t *status, int32_t *symbols_out, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* CR+BQ baseline (csrc/bq.hip): the 8-bit affine quantizer of `SimpleQuantizer` / `SimpleDequantizer`  */
/* (sc2bench/transforms/misc.py:181-231 -> torchdistill tensor_util.quantize_tensor / dequantize_tensor) */
/* and the two pooling layers of `larger_resnet_bottleneck` (sc2bench/models/layer.py:108-153).          */
/* Plain grid-size kernels, no atomics; every result below is defined to the bit.                        */
/* ------------------------------------------------------------------------------------------ */
/* x: f32, n_seg contiguous segments of n_per_seg elements (n_seg = 1: the reference's per-tensor quantization; n_seg = N: one
 * scale per image).  Per segment, in f32 and in this order, each step rounded once:
 *   scale = (max - min) / 255;  izp = 0 - min / scale;  zero_point = (int)clamp(izp, 0, 255);
 *   q = u8(rint(clamp(zero_point + x / scale, 0, 255)))          (rint: half to even; both divisions correctly rounded)
 * min / max as torch.min / torch.max (a NaN makes both NaN).  status[seg] bit 1: izp is NaN (a NaN in the segment, or an all-zero
 * segment: 0 / 0) -- the reference raises ValueError from int(nan) there; q of that segment is 0.  A non-zero constant segment is
 * no error (scale 0, IEEE infinities: codes all 255 with zero point 0, or all 0 with zero point 255).
 * Two launches: per-workgroup (min, max) pairs into partial [sc2_bq_partial_len(n_seg, n_per_seg)] f32, then every workgroup reduces
 * its segment's pairs again and quantizes its share.  q: u8 in x's order; scale f32 / zero_point i32 / status i32: [n_seg]. */
long long sc2_bq_partial_len(long long n_seg, long long n_per_seg);
int sc2_bq_quantize(const float *x, uint8_t *q, float *scale, int32_t *zero_point, int32_t *status, float *partial, long long n_seg,
                    long long n_per_seg, void *stream);
/* y = scale[seg] * ((float)q - (float)zero_point[seg]): one exact subtraction, one multiply; y f32 in q's order.  scale and
 * zero_point are DEVICE arrays [n_seg]. */
int sc2_bq_dequantize(const uint8_t *q, const float *scale, const int32_t *zero_point, float *y, long long n_seg, long long n_per_seg,
                      void *stream);
/* The same from u8 NCHW codes [N,C,H,W] to a bf16 NHWC map [N,H,W,Cpad] (Cpad % 8 == 0, channels >= C exact zeros), with an optional
 * per-channel affine (a, b: f32 [C], both or neither -- the decoder's leading eval-mode BatchNorm2d) and ReLU:
 * relu(fmaf(a_c, scale * (q - zp), b_c)) in f32, rounded to bf16 once.  per_sample: scale / zero_point are [N], else [1]. */
int sc2_bq_dequantize_nhwc(const uint8_t *q, const float *scale, const int32_t *zero_point, int per_sample, const float *a,
                           const float *b, int relu, void *y, int N, int C, int H, int W, int Cpad, void *stream);
/* nn.MaxPool2d + eval-mode nn.BatchNorm2d + ReLU on a bf16 NHWC map (layer.py:133-135): sc2_maxpool_nhwc's window walk, then
 * relu(fmaf(a_c, max, b_c)) in f32 rounded to bf16 once -- the affine AFTER the max (a_c may be negative).  a, b: f32 [C], 16-byte
 * aligned; C % 8 == 0. */
int sc2_maxpool_affine_relu_nhwc(const void *x, void *y, const float *a, const float *b, int N, int H, int W, int C, int KH, int KW,
                                 int stride_h, int stride_w, int pad_h, int pad_w, void *stream);
/* nn.AvgPool2d(kernel, stride, no padding) on a bf16 NHWC map (layer.py:149: kernel 2, stride 1): f32 sum over the window in
 * row-major order, times 1 / kernel^2, rounded to bf16 once.  x [N,H,W,C] -> y [N,OH,OW,C], C % 8 == 0. */
int sc2_avgpool2d_nhwc(const void *x, void *y, int N, int H, int W, int C, int kernel, int stride, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Detection tail (csrc/detect.hip): the two operations of torchvision's Faster R-CNN inference path behind the  */
/* feature pyramid that torch has no operator for.  tests/ref_detection.py restates both.                        */
/* ------------------------------------------------------------------------------------------ */
#define SC2_NMS_MAX_BOXES 16384   /* one call's boxes: a 32 MiB pair mask */
#define SC2_ROI_MAX_LEVELS 5
/* Greedy non-maximum suppression with groups (torchvision's `batched_nms`, the "vanilla" form: boxes of different groups never
 * suppress each other; no coordinate offsets).  boxes: f32 [n,4] (x1, y1, x2, y2), 16-byte aligned, ALREADY in processing order
 * (descending score, ties by ascending original index: the caller sorts); groups: i32 [n].
 * keep[i] = 1 iff no earlier KEPT box j of the same group has IoU(j, i) > iou_threshold (strictly: equal is kept; a box that only a
 * suppressed box overlaps is kept), else 0; *count = the number of ones.  keep: u8 [n], count: i32 [1], both DEVICE memory.
 * IoU in f32, every operation rounded once and in this order (no fused multiply-add, IEEE division):
 *   area = (x2 - x1) * (y2 - y1);  w = max(0, min(x2a, x2b) - max(x1a, x1b));  h likewise;  inter = w * h;
 *   iou = inter / (area_a + area_b - inter)                     (0 / 0 = NaN compares false: kept)
 * Two launches on `stream`: a 64 x 64-block pair mask into ws (one 64-bit word per row and column block, right of the diagonal
 * only), then ONE workgroup that walks the rows in order against a bitmap in LDS.  Nothing is copied to the host.
 * ws: sc2_nms_ws_bytes(n) bytes, 8-byte aligned (0 for n outside 1..SC2_NMS_MAX_BOXES).  n == 0 launches nothing (*count is cleared by
 * a stream-ordered fill); n > SC2_NMS_MAX_BOXES returns SC2_ERR_UNSUPPORTED: split by group (groups are independent). */
long long sc2_nms_ws_bytes(int n);
int sc2_nms(const float *boxes, const int32_t *groups, int n, float iou_threshold, uint8_t *keep, int32_t *count, void *ws, void *stream);

/* One pyramid level of sc2_roi_align: an NHWC map [N,H,W,C] (f32 or bf16, 16-byte aligned) and image pixels -> map pixels. */
typedef struct sc2_roi_level {
    const void *data;
    int32_t H, W;
    float spatial_scale;
} sc2_roi_level;
typedef struct sc2_roi_levels {
    sc2_roi_level level[SC2_ROI_MAX_LEVELS];
} sc2_roi_levels;
/* Multi-level RoIAlign with torchvision's aligned=False semantics (what `MultiScaleRoIAlign` runs inside `FasterRCNN`).
 * lv: the first n_levels descriptors (passed by value: no device copy of them); every level holds N images of C channels,
 * C % 8 == 0, all f32 or all bf16 (is_bf16).  rois: f32 [K,5] (image index, x1, y1, x2, y2 in image pixels); levels: i32 [K], the level
 * each RoI is pooled from.  out: f32 [K,C,P,P].  P in 1..14, sampling_ratio in 1..16 (the adaptive form, <= 0, is not built).
 * Per RoI and axis, in f32: start = x1 * scale, end = x2 * scale, size = max(end - start, 1), bin = size / P; sample i of bin p at
 * start + p * bin + (i + 0.5) * bin / sampling_ratio.  A sample with y < -1 or y > H (x likewise) contributes 0; otherwise y is
 * clamped to [0, H - 1] (the neighbour y_low + 1 is clamped to H - 1, then with weight 0) and read bilinearly; the output is the mean
 * of the sampling_ratio^2 samples.  A RoI whose level is outside 0..n_levels-1 or whose image index is outside 0..N-1 reads nothing:
 * its outputs are NaN.  One workgroup per RoI, one launch on `stream`. */
int sc2_roi_align(sc2_roi_levels lv, int n_levels, int N, int C, int is_bf16, const float *rois, const int32_t *levels, int K, int P,
                  int sampling_ratio, float *out, void *stream);

/* The adjoint of sc2_roi_align with respect to f32 maps: grad_out f32 [K,C,P,P] and the forward call's rois, levels, P and
 * sampling_ratio -> one f32 NHWC gradient [N,H_l,W_l,C] per level, written through lv.level[l].data (16-byte aligned; H, W and
 * spatial_scale as in the forward call).  EVERY element of every map is written: zero where no sample lands.  Sample positions and
 * bilinear weights are the forward's, in f32 by the same expressions; a RoI whose level or image index does not exist contributes
 * nothing.  RoI coordinates must be finite.
 * The caller bins the RoIs: order: i32 [K], the RoI indices sorted by bin = level * N + image and ASCENDING within a bin, RoIs without a
 * valid bin last; bin_off: i32 [n_levels * N + 1], bin b is order[bin_off[b] .. bin_off[b+1]).  Both DEVICE memory.  Every entry is
 * checked (offsets clamped to 0..K, indices outside 0..K-1 and RoIs that do not belong to the bin are skipped), so malformed bins lose
 * contributions but never address outside the arrays.
 * One launch on `stream`: a workgroup per 8 x 8 pixel tile of one (level, image) map gathers that map's RoIs in the order given.  No
 * atomics: two calls on the same inputs give the same bits.  K == 0 gives all-zero maps. */
int sc2_roi_align_backward(sc2_roi_levels lv, int n_levels, int N, int C, const float *grad_out, const float *rois, const int32_t *levels,
                           const int32_t *order, const int32_t *bin_off, int K, int P, int sampling_ratio, void *stream);

#define SC2_MATCH_CHUNK 2048      /* candidates per workgroup of sc2_box_match's first launch: one workspace row per chunk */
/* torchvision's `Matcher` over `box_iou` for several images in one call, without the [G, A] IoU matrix in memory.
 * gt: f32 [total_gt,4], cand: f32 [total_cand,4] (x1, y1, x2, y2; both 16-byte aligned); gt_off, cand_off: i32 [n_img + 1] on the DEVICE,
 * image i owns rows off[i] .. off[i+1]; gt_off_host, cand_off_host: the caller's HOST copies of the same offsets.  The host copies are
 * checked before anything is launched (first 0, never decreasing, last == the total: SC2_ERR_INVALID_ARG otherwise) and size the
 * grids; the kernels read the device copies and clamp them to the totals.
 * matches: i32 [total_cand]; best_iou: f32 [total_cand] or NULL.  IoU in f32, every operation rounded once, as sc2_nms states it
 * (areas (x2 - x1) * (y2 - y1); w, h clamped at 0; inter / (area_gt + area_cand - inter)).
 * Per candidate: best_iou = the maximum over its image's gt boxes, taken as a running maximum from -infinity that only a strictly
 * greater value replaces, in ascending gt index.  Hence (1) a tie goes to the LOWEST gt index and (2) a NaN IoU (0 / 0) never becomes
 * the maximum; a candidate all of whose IoUs are NaN keeps -infinity and index 0.  matches = -1 if best_iou < low, -2 if
 * low <= best_iou < high, else the gt index local to the image.
 * allow_low_quality: a candidate whose IoU with SOME gt box equals that gt box's maximum over all candidates of the image (same
 * rules: NaN never the maximum) gets its own pre-threshold argmax back -- torchvision's behaviour: the argmax is restored, not the
 * gt box the candidate is best for.  A per-gt maximum of exactly 0 restores every candidate with IoU 0 to it, as in torchvision.
 * An image without gt boxes: matches = -1, best_iou = 0, nothing of gt is read.
 * At most two launches on `stream`: per-gt maxima over chunks of SC2_MATCH_CHUNK candidates into ws (a max-reduction: independent of
 * order; skipped without allow_low_quality), then the per-candidate pass, which folds the chunks.  No atomics.
 * ws: sc2_box_match_ws_bytes(total_gt, the longest image's candidate count) bytes, 4-byte aligned (0 if either is <= 0). */
long long sc2_box_match_ws_bytes(int total_gt, int max_candidates);
int sc2_box_match(const float *gt, const int32_t *gt_off, const float *cand, const int32_t *cand_off, const int32_t *gt_off_host,
                  const int32_t *cand_off_host, int n_img, int total_gt, int total_cand, float low, float high, int allow_low_quality,
                  int32_t *matches, float *best_iou, void *ws, void *stream);

#define SC2_DETPOST_MAX_CLASSES 128   /* C, background included: a lane owns two classes */
#define SC2_DETPOST_MAX_DET 1024      /* D = detections_per_img */
#define SC2_DETPOST_MAX_SEG 2048      /* survivors of ONE class of one image: sorted and suppressed in LDS (the reference runs 1 000 proposals) */
#define SC2_DETPOST_MAX_CAND 20480    /* survivors of one image: at most 1 / score_thresh classes of a row pass, 19 x 1 000 at 0.05 */
#define SC2_DETPOST_OVER_CAND 1       /* status bits */
#define SC2_DETPOST_OVER_SEG 2
/* torchvision's `RoIHeads.postprocess_detections` for a batch (csrc/det_post.hip; tests/ref_det_post.py restates it).
 * logits: f32 [R,C], deltas: f32 [R,4C] (16-byte aligned), proposals: f32 [R,4] (16-byte aligned), the rows of image i being
 * offsets[i] .. offsets[i+1]; offsets: i32 [n+1] on the DEVICE and offsets_host the caller's HOST copy, checked before anything is
 * launched as sc2_box_match checks its own (first 0, never decreasing, last == R: SC2_ERR_INVALID_ARG otherwise; the kernels read the
 * device copy and clamp it to 0..R); image_sizes: i32 [n,2] (height, width) on the device.  2 <= C <= SC2_DETPOST_MAX_CLASSES,
 * 1 <= D <= SC2_DETPOST_MAX_DET, R (C-1) < 2^31 (SC2_ERR_UNSUPPORTED otherwise), n <= 65535; no threshold may be NaN.
 * Stage A, per (row r, class c >= 1), all in f32 with every operation rounded once:
 *   score = exp(l_c - max) / sum, max and sum over the row's C logits (sum: classes c and c + 64 first, then a fixed butterfly);
 *   the box is BoxCoder.decode_single in that function's order: widths = x2 - x1, ctr_x = x1 + 0.5 * widths, dx = d0 / wx,
 *   dw = d2 / ww cut at bbox_xform_clip, pred_ctr_x = dx * widths + ctr_x, half_w = 0.5 * (exp(dw) * widths), x1' = pred_ctr_x - half_w,
 *   x2' = pred_ctr_x + half_w (y likewise), then clipped to [0, width] x [0, height];
 *   the candidate survives iff score > score_thresh and x2' - x1' >= min_size and y2' - y1' >= min_size.  Comparisons with a NaN
 *   are false: a row whose scores are NaN (a NaN or +infinite logit) yields no candidate.
 * Stage B, per image: the survivors in order of descending score, equal scores by ascending flat index r_local * (C-1) + (c-1) (the
 * stable sort of `batched_nms`); greedy NMS within each class with sc2_nms's IoU and test (IoU > nms_thresh, the earlier box first);
 * the first D kept, in that order, are the image's detections.
 * boxes: f32 [n,D,4] (16-byte aligned), scores: f32 [n,D], labels: i64 [n,D], count, status: i32 [n].  EVERY element is written
 * exactly once: slots at or behind count[i] hold zeros.  An image with more than SC2_DETPOST_MAX_CAND survivors, or more than
 * SC2_DETPOST_MAX_SEG of one class, gets the matching status bit and count 0 (the caller takes another path); status 0 otherwise.
 * cand_scores f32 [R,C-1], cand_boxes f32 [R,C-1,4] (16-byte aligned): both NULL in production; a test passes both and receives the
 * whole candidate table of stage A (survivors or not), which stage B then reads in place of the workspace's copy.
 * Three launches on `stream` whatever n is (rows; (class, image) segments: bitonic sort and the greedy walk in LDS, stopping at D
 * kept; one merge per image), none when n == 0; nothing is copied to the host, no atomics on global memory: the same bits each call.
 * ws: sc2_det_postprocess_ws_bytes(R, C, n, D) bytes, 16-byte aligned (0 for dimensions outside the ranges above). */
long long sc2_det_postprocess_ws_bytes(int R, int C, int n, int D);
int sc2_det_postprocess(const float *logits, const float *deltas, const float *proposals, const int32_t *offsets, const int32_t *offsets_host,
                        const int32_t *image_sizes, int R, int C, int n, float wx, float wy, float ww, float wh, float bbox_xform_clip,
                        float score_thresh, float min_size, float nms_thresh, int D, float *boxes, float *scores, int64_t *labels,
                        int32_t *count, int32_t *status, float *cand_scores, float *cand_boxes, void *ws, void *stream);

#define SC2_RPNPOST_MAX_LEVELS 8          /* L */
#define SC2_RPNPOST_MAX_PRE_NMS 2048      /* K = pre-NMS top-n per level: one level's selection is sorted and suppressed in LDS (training runs 2 000) */
#define SC2_RPNPOST_MAX_POST_NMS 2048     /* P = post-NMS top-n per image */
#define SC2_RPNPOST_MAX_KEYS 16384        /* sum over the levels of min(K, n_l): an image's kept keys are merged in one workgroup's LDS (128 KiB) */
#define SC2_RPNPOST_MAX_ANCHORS 536870912 /* T, the anchors of one image, stays BELOW this (2^31 / 4) */
/* torchvision's `RegionProposalNetwork.filter_proposals`, with the decode of the boxes it keeps, for a batch (csrc/rpn_post.hip;
 * tests/ref_rpn_post.py restates it).  The RPN head's outputs are read in place: no permute, no concat, no decode of all anchors.
 * objectness, deltas: HOST arrays of L device pointers: level l's objectness map f32 [N, A_l, H_l, W_l] and delta map
 * f32 [N, 4 A_l, H_l, W_l] (channel 4 a + c), NCHW and contiguous; num_anchors, heights, widths: HOST arrays of A_l, H_l, W_l (>= 1).
 * Level l has n_l = A_l H_l W_l anchors, index t = (h W_l + w) A_l + a within the level (the order of
 * `concat_box_prediction_layers` and of `AnchorGenerator`); anchors: f32 [T,4] of ONE image, T = sum n_l, level l starting at
 * n_0 + .. + n_(l-1); image_sizes: i32 [N,2] (height, width) on the device.
 * Caps, checked on the host before anything is launched: 1 <= L <= SC2_RPNPOST_MAX_LEVELS, 1 <= K <= SC2_RPNPOST_MAX_PRE_NMS,
 * 1 <= P <= SC2_RPNPOST_MAX_POST_NMS, sum_l min(K, n_l) <= SC2_RPNPOST_MAX_KEYS, T < SC2_RPNPOST_MAX_ANCHORS (SC2_ERR_UNSUPPORTED
 * otherwise); N <= 65535, no threshold NaN, every pointer 16-byte aligned (SC2_ERR_INVALID_ARG otherwise).  The counts are bounded
 * by K: there is no data-dependent overflow and no status word.
 * 1. Selection, per (image, level): the k_l = min(K, n_l) anchors greatest by logit, the logits compared as floats -- -0 equals +0,
 *    every NaN ranks above every number (and equals every other NaN) -- and of equal logits the LOWER index t first.  An anchor's
 *    RANK is its place in that order.  (torch.topk leaves ties unspecified; this entry specifies them.)
 * 2. Per selected anchor, in f32 with every operation rounded once: score = 1 / (1 + exp(-logit)); the box is
 *    BoxCoder.decode_single of (anchor, the four deltas) followed by the clip to the image, as sc2_det_postprocess states it.
 * 3. It survives iff x2' - x1' >= min_size and y2' - y1' >= min_size and score >= score_thresh (all inclusive: the RPN's rule); a
 *    comparison with a NaN is false.
 * 4. Per image, the survivors in order of (score descending, level ascending, rank ascending) -- the stable sort of `batched_nms`
 *    over the levels' concatenation; greedy NMS within each level in that order with sc2_nms's IoU and test (IoU > nms_thresh, the
 *    earlier box kept).
 * 5. The kept boxes of all levels in that order, the first P: boxes f32 [N,P,4], scores f32 [N,P], count i32 [N].  EVERY element
 *    is written exactly once: slots at or behind count[i] hold zeros.
 * cand_index i32 [N,L,K], cand_scores f32 [N,L,K], cand_boxes f32 [N,L,K,4], cand_k i32 [N,L]: all NULL in production; a test passes
 * all four and receives the candidate table of steps 1 and 2 -- slot j < k_l of (image, level): the level-local index, score and
 * clipped box of rank j; slots behind k_l: index -1, zeros; cand_k: k_l -- which steps 3 to 5 then read in place of the workspace's.
 * Three launches on `stream` whatever N is ((level, image): radix select over LDS histograms, ordered pick of the ties, sort,
 * decode; (level, image): sort and greedy walk in LDS; one merge per image), none when N == 0; nothing is copied to the host, no
 * atomics on global memory: the same bits each call.
 * ws: sc2_rpn_proposals_ws_bytes(N, L, K, P) bytes, 16-byte aligned (0 for dimensions outside the ranges above). */
long long sc2_rpn_proposals_ws_bytes(int N, int L, int K, int P);
int sc2_rpn_proposals(const float *const *objectness, const float *const *deltas, const int32_t *num_anchors, const int32_t *heights,
                      const int32_t *widths, int L, const float *anchors, const int32_t *image_sizes, int N, int K, int P, float nms_thresh,
                      float score_thresh, float min_size, float wx, float wy, float ww, float wh, float bbox_xform_clip, float *boxes,
                      float *scores, int32_t *count, int32_t *cand_index, float *cand_scores, float *cand_boxes, int32_t *cand_k, void *ws,
                      void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Segmentation tail (csrc/seg.hip): low-resolution class logits -> labels of the resized map and confusion counts, */
/* one launch.  tests/ref_seg.py restates it in float64.                                                            */
/* ------------------------------------------------------------------------------------------ */
#define SC2_SEG_MAX_CLASSES 64    /* a workgroup's [C,C] int32 histogram: 16 KB of LDS at most */
/* What `interpolate(logits, (H, W), mode='bilinear', align_corners=False).argmax(1)` followed by the confusion-matrix update of
 * the reference's SegEvaluator computes, without forming the resized logits, in f32 on the unrounded input.
 * logits : [N,C,h,w], f32 or bf16 (is_bf16), addressed by four ELEMENT strides (>= 0): NCHW memory, a slice of it, or the permuted
 *          view of an NHWC map whose channel pitch is padded.  Only classes 0..C-1 decide a label.  c_readable: how many
 *          consecutive elements behind class 0 of EVERY pixel lie inside the caller's allocation (>= C; their values beyond C are
 *          never used).  With stride_c == 1, c_readable >= C rounded up to 8 (bf16) / 4 (f32), a 16-byte aligned base and the other
 *          strides multiples of 8 / 4, classes are read with 16-byte loads; any other layout takes the strided path.
 * H, W   : the output size; any size, H < h included.  All four sides at most 32768; C in 1..SC2_SEG_MAX_CLASSES
 *          (SC2_ERR_UNSUPPORTED otherwise: the caller keeps its torch-op path).
 * Per axis, for output index d, in integers: t = (2d+1)*in - out;  t <= 0: i0 = 0, lambda = 0;  otherwise i0 = t / (2 out),
 * lambda = float(t % (2 out)) / float(2 out);  i1 = min(i0 + 1, in - 1).  Per class, every operation rounded once (no fused
 * multiply-add):  (1-ly)*((1-lx)*x[y0,x0] + lx*x[y0,x1]) + ly*((1-lx)*x[y1,x0] + lx*x[y1,x1]).
 * label  = the first class holding the maximum; a NaN counts as larger than any number and the first NaN wins (torch.argmax).
 * labels : int64 [N,H,W] contiguous, or NULL (no store is issued).
 * targets: int64 [N,H,W] contiguous, mat: int64 [C,C]; given together, every pixel with 0 <= target < C ADDS 1 to
 *          mat[target][label] (any other target value -- 255, negatives, >= C -- is skipped).  mat is not cleared: it carries over
 *          from call to call.  Integer sums: the matrix does not depend on the order of arrival.  Either NULL: nothing is counted.
 * At least one of labels and the (targets, mat) pair must be given.  One launch on `stream`. */
int sc2_seg_predict(const void *logits, int is_bf16, int N, int C, int h, int w, long long stride_n, long long stride_c,
                    long long stride_h, long long stride_w, int c_readable, int H, int W, const long long *targets, long long *labels,
                    long long *mat, void *stream);

/* Segmentation training loss (csrc/seg_loss.hip): `cross_entropy(interpolate(logits, (H, W), mode='bilinear', align_corners=False),
 * targets, ignore_index=..)` and its gradient with respect to the LOW-resolution logits, without forming the resized logits or their
 * gradient.  tests/ref_seg_loss.py restates both in float64.
 * logits, strides, c_readable, H, W, the limits on sizes and classes: as for sc2_seg_predict, and at most 65535 images.  The resized
 * value v[p,c] of output pixel p and class c is sc2_seg_predict's formula (the kernels share its code: csrc/seg_common.h).
 * targets: int64 [N,H,W] contiguous.  A pixel is VALID when 0 <= target < C and target != ignore_index.  A pixel whose target equals
 * ignore_index is skipped (torch's rule); a target that is neither valid nor ignore_index is skipped too and counted as BAD (torch
 * trips a device assert there; no label may fault the device). */
#define SC2_SEG_CE_MEAN 0
#define SC2_SEG_CE_SUM 1
#define SC2_SEG_CE_NONE 2
/* Bytes of workspace a forward call needs for its per-workgroup partials (0 for sizes the kernels refuse). */
long long sc2_seg_ce_ws_bytes(int N, int H, int W);
/* Per valid pixel  loss_p = lse_p - v[p,target_p],  lse_p = m + logf(sum_c expf(v[p,c] - m)),  m = max_c v[p,c]: f32, accurate expf /
 * logf, one online pass over the classes (running maximum; the running sum is rescaled by expf(m_old - m_new) when the maximum moves).
 * pixel_loss: f32 [N,H,W] or NULL; skipped pixels get 0 (reduction='none').  lse: f32 [N,H,W] or NULL; written for every pixel,
 *             what the backward call reads.
 * sums      : three 8-byte words of device memory: float64 sum of loss_p over the valid pixels, int64 number of valid pixels, int64
 *             number of bad targets.  Nothing is read back; the caller divides on the device.
 * ws        : sc2_seg_ce_ws_bytes(N, H, W) bytes, 8-byte aligned.  Every workgroup leaves one float64 partial (and its two counts)
 *             there; a second launch of one workgroup adds them in a fixed order (consecutive runs of partials per thread, then a
 *             fixed tree).  No atomics: the sum has the same bits on every call, whatever order the workgroups ran in.
 * Two launches on `stream`, no host synchronisation. */
int sc2_seg_ce_forward(const void *logits, int is_bf16, int N, int C, int h, int w, long long stride_n, long long stride_c,
                       long long stride_h, long long stride_w, int c_readable, int H, int W, const long long *targets,
                       long long ignore_index, float *pixel_loss, float *lse, void *sums, void *ws, void *stream);
/* dx[n,c,i,j] = g * sum_p w_p(i,j) * (expf(v[p,c] - lse_p) - [c == target_p])  over the valid output pixels p whose bilinear footprint
 * holds source pixel (i,j).  w_p(i,j) is the product of the two axis weights: (1 - lambda) where i is the axis' i0, lambda where it is
 * i1, their sum where i0 == i1 at the clamped edge.
 * lse, sums : what the forward call wrote (sums[1], the number of valid pixels, is read on the device).
 * reduction : SC2_SEG_CE_MEAN: g = *grad_out / count, and every dx is 0 when count == 0 (torch: a NaN loss with a zero gradient);
 *             SC2_SEG_CE_SUM: g = *grad_out;  SC2_SEG_CE_NONE: grad_out is f32 [N,H,W], the factor of pixel p goes into its term, g = 1.
 * dx        : the logits' dtype (a bf16 gradient is rounded once from the f32 sum), addressed by its own four element strides.  EVERY
 *             element of [N,C,h,w] is written; source pixels no output pixel touches (downsampling) get 0.
 * A gather: the output rows that touch source row i are seg-axis-first(i-1) .. seg-axis-first(i+1) - 1, computable from integers because
 * i0(d) does not decrease with d, and likewise for columns; one thread owns one (source pixel, class) and adds its terms in f32,
 * row by row and left to right.  No atomics: dx has the same bits on every call.  One launch on `stream`. */
int sc2_seg_ce_backward(const void *logits, int is_bf16, int N, int C, int h, int w, long long stride_n, long long stride_c,
                        long long stride_h, long long stride_w, int c_readable, int H, int W, const long long *targets,
                        long long ignore_index, const float *lse, const void *sums, const float *grad_out, int reduction, void *dx,
                        long long dx_stride_n, long long dx_stride_c, long long dx_stride_h, long long dx_stride_w, void *stream);

/* Segmentation training input (csrc/seg_augment.hip): the PASCAL VOC augmentation chain of a whole batch -- Pillow's bilinear resize
 * of the 8-bit RGB image and its nearest resize of the 8-bit mask, horizontal flip, pad right / bottom, crop, ToTensor, Normalize, and
 * the collator's padded batch -- from the source bytes straight to the batch tensors.  Only the output window is computed: neither the
 * resized image nor the intermediate of Pillow's two passes is written to memory.  tests/ref_pil_resize.py restates the two resizes;
 * the result equals the host chain (Pillow + torch) bit for bit.
 * buf    : nbytes (1 .. 2^31-1) of device memory holding every sample's image (h*w*3 bytes, HWC, rows dense) and mask (h*w bytes).
 * desc   : int32 [n, SC2_SEG_AUGMENT_DESC_INTS] on the device, one row per sample:
 *            [0] image offset in buf   [1] mask offset in buf   [2] h  [3] w (source)   [4] nh  [5] nw (resized)   [6] flip (0 / 1)
 *            [7] top  [8] left (origin of the output window in the padded, flipped, resized image)
 *            [9] ext_h  [10] ext_w (extent of the sample inside its [oh, ow] slot)   [11..15] unused by the kernels (the wrapper keeps
 *            the padded size there to refuse a window outside the padded image before the launch)
 * Output pixel (y, x) of sample i: outside ext_h x ext_w the image is 0.0f and the target 255 (the collator's fill); else it shows
 * position (top + y, left + x) of the padded image: beyond nh x nw the image is (0 / 255 - mean) / std and the target 255 (the pad
 * area); else the resized pixel of that row and of column left + x, or nw - 1 - (left + x) when flipped, as
 * (float(p) / 255.0f - mean[c]) / std[c] with two correctly rounded f32 divisions, and the resized mask's byte as int64.
 * Image pixels: Pillow's ImagingResample with the bilinear filter -- per axis n_in -> n_out in float64, every operation rounded once:
 * scale = n_in / n_out, support = filterscale = max(scale, 1), center = (xx + 0.5) * scale, first = max(int(center - support + 0.5), 0),
 * count = min(int(center + support + 0.5), n_in) - first, weight max(0, 1 - |(x + first - center + 0.5) * (1 / filterscale)|), weights
 * divided by their left-to-right sum, k = int(0.5 + w * 2^22); a pass is clip((2^21 + sum(pixel * k)) >> 22, 0, 255); the horizontal
 * pass first, to 8 bits, the vertical pass on those.  (A pass of equal lengths, which Pillow skips, has the one coefficient 2^22.)
 * Mask pixels: Pillow's nearest resize -- source index int(xo) with xo = a * 0.5 at output 0 and xo += a per output, a = n_in / n_out.
 * mean, std : three f32 each, HOST memory (std != 0).
 * images : f32 [n,3,oh,ow];  targets : int64 [n,oh,ow];  both contiguous, every element of an accepted sample written.
 * ws     : sc2_seg_augment_workspace(n, oh, ow) bytes, 4-byte aligned.  Per sample ow column entries, then oh row entries, of
 *          SC2_SEG_AUGMENT_ENTRY_INTS int32 each: first source index, count, nine coefficients, the nearest resize's source index;
 *          entries of positions that show no resized pixel are zero.
 * status : int32 [n], written for every sample: 0, or SC2_SEG_AUGMENT_RATIO when an axis shrinks by more than 4 (filterscale > 4: more
 *          than nine taps), or SC2_SEG_AUGMENT_BAD for a row with offsets outside buf, sides outside 1 .. SC2_SEG_AUGMENT_MAX_SIDE, a
 *          negative origin or an extent beyond the slot.  Such a sample's outputs and tables are left unwritten; no address is formed
 *          from it.  The caller redoes the batch on the host.
 * Two launches on `stream` (tables, then one workgroup per 16 x 64 output tile), no atomics, no host synchronisation. */
#define SC2_SEG_AUGMENT_DESC_INTS 16
#define SC2_SEG_AUGMENT_ENTRY_INTS 12
#define SC2_SEG_AUGMENT_MAX_SIDE 16384
#define SC2_SEG_AUGMENT_MAX_BATCH 65535
#define SC2_SEG_AUGMENT_RATIO 1
#define SC2_SEG_AUGMENT_BAD 2
long long sc2_seg_augment_workspace(int n, int oh, int ow);
int sc2_seg_augment(const uint8_t *buf, long long nbytes, const int32_t *desc, int n, int oh, int ow, const float *mean,
                    const float *std, float *images, long long *targets, void *ws, int32_t *status, void *stream);

/* Classification input (csrc/cls_input.hip): the ImageNet chains of a whole batch -- RandomResizedCrop -> RandomHorizontalFlip ->
 * ToTensor -> Normalize, or Resize -> CenterCrop -> ToTensor -> Normalize -- from source bytes straight to the f32 batch.  A sample is a
 * STORED BOX of a full image, resampled with the full image's coefficients (Pillow's ImagingResample, bilinear, exactly the arithmetic
 * stated above for sc2_seg_augment), flipped, and shown through an oh x ow window.  tests/ref_cls_input.py restates it; the result
 * equals the host chain (Pillow + torch) bit for bit.
 * buf    : nbytes (1 .. 2^31-1) of device memory holding every sample's stored box (h*w*3 bytes, RGB, HWC, rows dense: pitch 3*w).
 * desc   : int32 [n, SC2_CLS_INPUT_DESC_INTS] on the device, one row per sample:
 *            [0] offset of the stored box in buf   [1] h  [2] w (the stored box)   [3] full_h  [4] full_w (the axis lengths the
 *            coefficients see)   [5] row0  [6] col0 (where the stored box sits inside the full image)   [7] nh  [8] nw (resized)
 *            [9] flip (0 / 1)   [10] top  [11] left (origin of the window in the resized, flipped image)   [12..15] unused
 *          Training: the box is the crop itself -- full = (h, w), row0 = col0 = 0, (nh, nw) = (oh, ow), top = left = 0 -- so the
 *          resample clamps at the crop's edges as `img.crop(...).resize(...)` does.  Evaluation: full is the whole image, (nh, nw)
 *          Resize's size, (top, left) CenterCrop's origin, and the box need hold only the rows and columns the window's taps read.
 * Output pixel (y, x) of sample i is resized row top + y and resized column left + x, or nw - 1 - (left + x) when flipped, as
 * (float(p) / 255.0f - mean[c]) / std[c] with two correctly rounded f32 divisions.  An axis with full == resized is the identity pass:
 * the one coefficient 2^22 on the pixel itself, which is Pillow's skipped pass byte for byte and reads no neighbour.
 * mean, std : three f32 each, HOST memory (std != 0).
 * images : f32 [n,3,oh,ow], contiguous; every element of an accepted sample is written.
 * status : int32 [n], written for every sample: 0, or
 *            SC2_CLS_INPUT_BAD    sides outside 1 .. SC2_SEG_AUGMENT_MAX_SIDE, a box outside buf or outside the full image, a window outside
 *                                 the resized image, a flip that is not 0 / 1;
 *            SC2_CLS_INPUT_RATIO  an axis shrinks by more than 4 (full > 4 * resized: more than nine taps);
 *            SC2_CLS_INPUT_TAP    a tap of the window lies outside the stored box.
 *          Such a sample's slot is left unwritten and no address is formed from it.  The caller redoes the batch on the host.
 * ONE launch on `stream`, one workgroup per 16 x 64 output tile: the tile's 64 column and 16 row entries are computed in the
 * workgroup's prologue into LDS, so there is no table in memory: sc2_cls_input_workspace is 0 for every batch the entry takes (-1 for
 * sizes it refuses: n outside 1 .. SC2_CLS_INPUT_MAX_BATCH, a side outside 1 .. SC2_SEG_AUGMENT_MAX_SIDE).  No atomics, no host
 * synchronisation. */
#define SC2_CLS_INPUT_DESC_INTS 16
#define SC2_CLS_INPUT_MAX_BATCH 65535
#define SC2_CLS_INPUT_RATIO 1
#define SC2_CLS_INPUT_BAD 2
#define SC2_CLS_INPUT_TAP 3
long long sc2_cls_input_workspace(int n, int oh, int ow);
int sc2_cls_input(const uint8_t *buf, long long nbytes, const int32_t *desc, int n, int oh, int ow, const float *mean, const float *std,
                  float *images, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* COCO box AP (csrc/coco.hip): COCOeval's `bbox` protocol with its default parameters, written from the published     */
/* protocol.  tests/ref_coco.py restates it as a sequential float64 loop; both kernels reproduce that bit for bit.    */
/* ------------------------------------------------------------------------------------------ */
#define SC2_COCO_THRS 10          /* iouThrs = linspace(.5, .95, 10) */
#define SC2_COCO_RECS 101         /* recThrs = linspace(0, 1, 101) */
#define SC2_COCO_AREAS 4          /* [0,1e10], [0,32^2], [32^2,96^2], [96^2,1e10] */
#define SC2_COCO_MAXDETS 3        /* maxDets = (1, 10, 100) */
#define SC2_COCO_TILE_DETS 100    /* the on-chip IoU tile of one (image, category) segment: 100 x 64 f64 = 50 KB of LDS */
#define SC2_COCO_TILE_GTS 64
#define SC2_COCO_SCAN_CHUNK 1024  /* detections per step of the accumulate kernel's scan (256 lanes x 4) */
/* The definition (useCats = 1; categories are the ground truth's in ascending id order, detections of any other label are dropped;
 * images are those the evaluator was given, in ascending id order, one with no prediction included):
 * Boxes: a detection (x1,y1,x2,y2) in f32 becomes (x1, y1, f32(x2-x1), f32(y2-y1)), then f64; ground truth is xywh in f64.  Detection
 *   area = w*h in f64; ground-truth area = the annotation's `area` field.
 * IoU, in f64, every operation rounded once: w = min(dx+dw, gx+gw) - max(dx, gx), h likewise; w <= 0 or h <= 0: 0; else i = w*h,
 *   u = dw*dh for a crowd ground truth, else dw*dh + gw*gh - i; iou = i / u.
 * Per (image, category) SEGMENT: detections in descending score order (ties: ascending original position), the first 100 kept.  Per
 *   area range [lo, hi]: a ground truth is IGNORED if it is a crowd or its area is < lo or > hi; ground truths are walked non-ignored
 *   first (stable).  Per threshold t and detection in order: best = min(t, 1 - 1e-10), m = none; walk the ground truths: skip one
 *   already matched at t unless it is a crowd; stop if m is non-ignored and this one is ignored; skip if iou < best; else best = iou,
 *   m = this (equal IoU moves the match to the LATER ground truth).  A match marks both; the detection inherits the ground truth's
 *   ignore flag.  An unmatched detection whose own area is < lo or > hi is ignored.  npig = the number of non-ignored ground truths.
 * Per (category, area range, maxDet): the first maxDet detections of every image, images in ascending id order, stable-sorted by
 *   descending score.  Per threshold: tp = matched and not ignored, fp = unmatched and not ignored, integer running sums;
 *   rc = tp / npig, pr = tp / (fp + tp + 2^-52); pr made non-increasing from the right; precision[t, r] = pr[first i with
 *   rc[i] >= recThrs[r]] or 0; recall[t] = rc[last], 0 with no detections.  A total npig of 0 leaves -1 everywhere.
 * Summary: the twelve statistics (AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl), each the mean of the entries
 *   > -1, or -1 with none.
 *
 * sc2_coco_match: ONE launch, one workgroup per segment.  dets: f64 [n_det,4] xywh ALREADY in processing order within each segment;
 * gts: f64 [n_gt,4] xywh, gt_area: f64 [n_gt], gt_crowd: u8 [n_gt]; det_off / gt_off: i32 [n_seg+1] ascending offsets (segment s holds
 * det_off[s] .. det_off[s+1]-1; a segment whose offsets leave 0..n_det / 0..n_gt is treated as empty); iou_thrs: f64 [10], area_rng: f64
 * [4,2] (lo, hi), both computed by the host so that both sides compare against the same bits.  Every pointer is DEVICE memory.
 * flags: i32 [n_det,4]: per detection and area range, bit t = matched at threshold t, bit 10+t = ignored at t.
 * npig : i32 [n_seg,4].
 * The IoU of the first SC2_COCO_TILE_DETS x SC2_COCO_TILE_GTS pairs of a segment is computed once, by the whole workgroup, into LDS;
 * the forty (area range, threshold) walks run on forty lanes of one wave, serial over the detections.  Neither count is bounded:
 * pairs outside the tile are recomputed where they are read (the same operations: the same bits), and a segment of more than
 * SC2_COCO_TILE_GTS ground truths keeps its matched marks (one byte per ground truth and lane) in `ws` instead of LDS.
 * ws: sc2_coco_match_ws_bytes(n_gt) bytes.  Empty segments are legal; n_seg == 0 launches nothing.  Nothing is copied to the host.
 * A detection past the hundredth of its segment is matched like any other, behind the first hundred (it cannot change them): the
 * cut is sc2_coco_accumulate's `rank < maxDet`. */
long long sc2_coco_match_ws_bytes(long long n_gt);
int sc2_coco_match(const double *dets, const double *gts, const double *gt_area, const uint8_t *gt_crowd, const int32_t *det_off,
                   const int32_t *gt_off, int n_seg, int n_det, int n_gt, const double *iou_thrs, const double *area_rng, int32_t *flags,
                   int32_t *npig, void *ws, void *stream);
/* sc2_coco_accumulate: ONE launch, one workgroup per (category, area range, maxDet), looping over the ten thresholds.
 * order: i32 [n_order], indices into flags / rank: category k's detections are order[cat_off[k] .. cat_off[k+1]-1] in that category's
 * score-sorted order (the caller's stable sorts); cat_off: i32 [K+1]; flags: i32 [n_det,4] of sc2_coco_match; rank: i32 [n_det], the
 * detection's position inside its (image, category) segment (kept where rank < maxDet); npig: i32 [K,4] category totals; rec_thrs: f64
 * [101] ascending; max_dets: i32 [3].  An index outside 0..n_det-1 is skipped, a category whose offsets leave 0..n_order is empty.
 * precision: f64 [10,101,K,4,3], recall: f64 [10,K,4,3]; every element is written.
 * A category's detections are scanned in chunks of SC2_COCO_SCAN_CHUNK with carried totals (block-wide integer scan of the packed
 * tp / fp counts).  The reverse running maximum and the 101 look-ups are one maximum per recall bin: precision[t, r] is the largest
 * pr among the entries whose rc reaches recThrs[r], which only a true positive can raise -- each true positive takes its pr to the
 * bin counting the thresholds its rc reaches (an integer maximum on the f64 bits, pr >= 0), and a suffix maximum over the 102 bins
 * ends the threshold.  K == 0 launches nothing. */
int sc2_coco_accumulate(const int32_t *order, const int32_t *cat_off, const int32_t *flags, const int32_t *rank, const int32_t *npig,
                        const double *rec_thrs, const int32_t *max_dets, int K, int n_order, int n_det, double *precision, double *recall,
                        void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Codec feature compression (csrc/jpeg.hip): a feature map through baseline JPEG, three channels per image, as the     */
/* reference's PILTensorModule(format='JPEG') computes it.  tests/ref_jpeg.py restates it as a sequential integer program. */
/* ------------------------------------------------------------------------------------------ */
#define SC2_JPEG_MAX_SIDE 64      /* H and W of the feature map: an image's planes, coefficients and bits stay in 53 KB of LDS */
#define SC2_JPEG_GREY 0
#define SC2_JPEG_RGB 1
#define SC2_JPEG_HEADER_GREY 328  /* bytes in front of the entropy-coded segment: SOI, JFIF APP0, one DQT per table, SOF0, one DHT per */
#define SC2_JPEG_HEADER_RGB 623   /* table, SOS -- the same at every size and quality */
#define SC2_JPEG_NEGATIVE_MIN 1   /* status bits of an image the kernel leaves to the caller's host path */
#define SC2_JPEG_ZERO_MAX 2
#define SC2_JPEG_NOT_FINITE 4
/* x: f32 [B,C,H,W] contiguous, H and W in 1..SC2_JPEG_MAX_SIDE (SC2_ERR_UNSUPPORTED beyond), quality in 1..100.  Every sample is cut
 * into C/3 images of three channels (RGB) followed by C%3 images of one channel (grey): n = C/3 + C%3 images per sample, image
 * `sample * n + g` everywhere below.  ONE launch on `stream`, one workgroup per image, nothing copied to the host.
 * Per image, with low = min and high = max of its channels:
 *   status: SC2_JPEG_NOT_FINITE alone (a NaN or an infinity in the group), else SC2_JPEG_NEGATIVE_MIN (low < 0: normalised values
 *   above 1 would reach an implementation-defined float-to-byte cast) | SC2_JPEG_ZERO_MAX (high <= 0: 0 / 0).  A non-zero status writes
 *   size 0 and the extrema, and nothing else: the caller runs that sample on its host path.
 *   p = u8(trunc(((v - low) / high) * 255)): three f32 operations, the division correctly rounded.
 *   RGB: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 128 * 65536 + 32767) >> 16,
 *   Cr = (32768 R - 27439 G - 5329 B + 128 * 65536 + 32767) >> 16; sampling 2x2 / 1x1 / 1x1.  Chroma: rows padded to an even count with
 *   the last row, columns with the last pixel; (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ... along a row; the last row then repeated
 *   to whole blocks.  Luma and grey planes edge-replicated to whole blocks.
 *   Level shift by 128; the slow-integer forward DCT with 13-bit constants (rows scaled by 4, columns descaled by 2 / 15, every shift
 *   rounding half up); coefficient = sign(x) * ((|x| + (8q >> 1)) / (8q)) with the Annex K tables scaled by `quality`
 *   (s = 5000 / quality below 50, else 200 - 2 quality; q = clamp((base * s + 50) / 100, 1, 255)).
 *   One scan: interleaved for RGB (MCU = four Y blocks, Cb, Cr), block after block for grey.  A Y block of an MCU beyond the block
 *   grid is a dummy: no AC, the DC of the block before it in the MCU.  DC as the difference from the previous block of its component,
 *   the Annex K Huffman tables, ZRL for runs above 15, EOB for trailing zeros, the last byte filled with 1 bits, a zero byte behind
 *   every 0xFF.
 *   Decoding from the coefficients on chip: times the table, the slow-integer inverse DCT (columns descaled by 11, rows by 18), + 128
 *   clamped to 0..255; chroma through the triangle upsampler where the chroma plane has more than two columns (vertically 3 near +
 *   far, the row beyond an edge equal to the edge row; horizontally (3 s + left + 8) >> 4 and (3 s + right + 7) >> 4, (4 s + 8) >> 4
 *   and (4 s + 7) >> 4 at the ends), repeated 2 x 2 otherwise; R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 *   G = Y + ((-22554 cb - 46802 cr + 32768) >> 16) with cb, cr minus 128, clamped.  out = (float(p) / 255) * high + low, unfused.
 * recon  : f32 [B,C,H,W].  sizes: i32 [B*n], bytes of the complete file: SC2_JPEG_HEADER_* + the entropy-coded segment + 2 (EOI).
 * extrema: f32 [B*n,2] (low, high).  status: i32 [B*n].
 * bytes  : NULL (no byte store is issued), or B*n slots of slot_bytes >= sc2_jpeg_max_bytes(RGB if C >= 3 else grey, H, W): the
 *          segment of image i at bytes + i * slot_bytes.  A block's bits are placed by a prefix sum over the blocks' bit lengths and
 *          OR-ed into LDS words; the stuffing by a prefix sum over the 0xFF counts: no bit depends on the order of arrival. */
long long sc2_jpeg_max_bytes(int mode, int H, int W);   /* every scan block at its longest code, every byte stuffed; -1: bad arguments */
int sc2_jpeg_tensor_codec(const float *x, int B, int C, int H, int W, int quality, float *recon, int32_t *sizes, float *extrema,
                          int32_t *status, uint8_t *bytes, long long slot_bytes, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Codec input compression (csrc/jpeg_image.hip): 8-bit images through baseline JPEG, as the reference's                  */
/* PILImageModule(format='JPEG') computes them.  The arithmetic, the tables and the file format are those of                */
/* sc2_jpeg_tensor_codec above from "RGB: Y = ..." to the colour conversion back; tests/ref_jpeg.py restates them.          */
/* ------------------------------------------------------------------------------------------ */
#define SC2_JPEG_IMAGE_MAX_SIDE 2048    /* H and W: 6 * 128 * 128 scan blocks of at most 1660 bits keep every bit offset inside int32 */
#define SC2_JPEG_IMAGE_CHUNK_BLOCKS 128 /* scan blocks the entropy pass codes per step */
/* x: u8, element [b,c,y,x] at x + b*sb + c*sc + y*sh + x*sw (non-negative element strides: a CHW tensor and the permuted view of an
 * HWC one are read in place).  C == 3: RGB with 2x2 / 1x1 / 1x1 sampling; C == 1: grey.  H and W in 1..SC2_JPEG_IMAGE_MAX_SIDE,
 * quality in 1..100 (SC2_ERR_UNSUPPORTED for another C, side or quality; SC2_ERR_INVALID_ARG for B < 1, a NULL or misaligned pointer,
 * a short workspace, short byte slots).  The input is 8-bit already: no extrema, no status words.  Three launches on `stream`, whose
 * boundaries are the only dependencies; no workgroup waits for another, nothing is copied to the host.
 *   workspace: sc2_jpeg_image_workspace_bytes(B, C, H, W) bytes, 4-byte aligned: i16 [B][n_scan][64], the quantised coefficients of
 *     every scan block in scan order (RGB: MCU after MCU in rows of ceil(W/16), four Y blocks, Cb, Cr; grey: block rows of ceil(W/8)),
 *     natural order inside a block.  A Y block of an MCU beyond the block grid is stored as the scan codes it: the DC of the block
 *     before it in the MCU, AC zero.  Every element is written before it is read; its content before the call does not matter.
 *   transform: one workgroup per (image, MCU row -- grey: block row --, chunk of 128 pixel columns).  The strip's pixels are
 *     edge-replicated on chip; a chroma row min(8 r + i, ceil(H/2) - 1) of MCU row r always lies inside r's own 16 pixel rows.
 *   entropy: one workgroup per image codes SC2_JPEG_IMAGE_CHUNK_BLOCKS scan blocks per step, one lane per block; the chunk's
 *     coefficients are staged in LDS in zigzag order and a lane visits only the non-zero ones of its block.  A block's DC predecessor
 *     -- the block before it OF ITS COMPONENT in scan order, also across chunks and strips -- is a stored coefficient (of the chunk
 *     on chip, or of the workspace for a chunk's first blocks), so no DC predictor is carried.
 *     The chunk carry is the count of segment bytes written so far (stuffing included) and the 0..7 bits behind the last whole byte,
 *     which open the next chunk's bit area; bits are placed by a prefix sum over the blocks' lengths and OR-ed into LDS words the kernel
 *     clears first, the stuffing by a prefix sum over the 0xFF counts of the chunk's whole bytes; the last chunk fills its last byte
 *     with 1 bits.  No bit depends on the order of arrival.
 *   decode: one workgroup per strip, from the workspace.  Strip context: the chroma blocks of the MCU row above and below and of the
 *     MCU column left and right of the strip are decoded with it, so that the triangle upsampler finds the row / column beyond the
 *     strip; the image's first and last chroma rows repeat themselves, a chroma plane of one or two columns is repeated 2 x 2.
 * recon: u8 [B,C,H,W] contiguous.  sizes: i32 [B], bytes of the complete file: SC2_JPEG_HEADER_* + the entropy-coded segment + 2.
 * bytes: NULL (no byte store is issued), or B slots of slot_bytes >= sc2_jpeg_image_max_bytes(C, H, W): image i's segment at
 *        bytes + i * slot_bytes; nothing behind the segment is written. */
long long sc2_jpeg_image_max_bytes(int C, int H, int W);            /* the formula of sc2_jpeg_max_bytes without the 64 cap; -1: bad arguments */
long long sc2_jpeg_image_workspace_bytes(int B, int C, int H, int W);   /* -1: bad arguments */
int sc2_jpeg_image_codec(const uint8_t *x, long long sb, long long sc, long long sh, long long sw, int B, int C, int H, int W, int quality,
                         uint8_t *recon, int32_t *sizes, uint8_t *bytes, long long slot_bytes, void *workspace, long long workspace_bytes,
                         void *stream);

/* ------------------------------------------------------------------------------------------ */
/* The detection transform around the image codec (csrc/rcnn_input.hip): what the reference's                               */
/* RCNNTransformWithCompression does per image in front of and behind PILImageModule(format='JPEG') -- bilinear resize and  */
/* `mul(255).byte()`, then `/ 255`, normalise and the copy into the zero-padded batch.  tests/ref_rcnn_input.py restates    */
/* both.  Streaming kernels, one launch each on `stream`; no LDS, no atomics, nothing is copied to the host.                */
/* ------------------------------------------------------------------------------------------ */
/* x: f32, element [c,y,x] at x + c*sc + y*sh + x*sw (non-negative element strides: a CHW tensor and the permuted view of an HWC one
 * are read in place), 4-byte aligned.  C in {1, 3}; H, W, oh, ow in 1..SC2_JPEG_IMAGE_MAX_SIDE (SC2_ERR_UNSUPPORTED for another C or
 * side; SC2_ERR_INVALID_ARG for a NULL or misaligned pointer, a negative stride).  oh, ow are the caller's: what
 * GeneralizedRCNNTransform.resized_size returns.
 * out: u8 [C,oh,ow] contiguous, any alignment.  Bilinear, align_corners=False, no antialiasing, as aten's upsample_bilinear2d computes
 *   it in f32 when no scale factor is handed down (F.interpolate(..., recompute_scale_factor=True)), every operation rounded once:
 *     scale = in / out;  src = max(scale * (d + 0.5) - 0.5, 0);  i0 = min(int(src), in - 1);  i1 = min(i0 + 1, in - 1);
 *     l1 = src - i0;  l0 = 1 - l1;  v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d);  byte = (uint8) trunc(v * 255.0f)
 *   One lane produces four adjacent pixels of a row (one 4-byte store where the address allows, else two 2-byte or four 1-byte ones)
 *   and reuses its column indices and weights over four rows; one workgroup per (channel, 16 rows, 256 columns).
 * status: i32 [1], 4-byte aligned, CLEARED BY THE CALLER before the launch: set to 1 (a plain store) by every lane that reads a NaN or
 *   a value outside [0, 1] -- there the host's `mul(255).byte()` wraps, which the kernel does not imitate: the bytes computed from such
 *   a value are unspecified (never a fault), the caller redoes the image on the host. */
int sc2_rcnn_resize_u8(const float *x, long long sc, long long sh, long long sw, int C, int H, int W, uint8_t *out, int oh, int ow,
                       int32_t *status, void *stream);
/* pixels: u8 [C,h,w] contiguous (sc2_jpeg_image_codec's recon), any alignment; C in {1, 3}, h and w in 1..SC2_JPEG_IMAGE_MAX_SIDE.
 * mean, std: C floats each ON THE HOST (read before the call returns).
 * out: f32 [C,Hp,Wp] contiguous, 4-byte aligned -- one image's slot of the batch tensor --, h <= Hp, w <= Wp (SC2_ERR_INVALID_ARG
 *   otherwise), Hp and Wp at most 4 * SC2_JPEG_IMAGE_MAX_SIDE (SC2_ERR_UNSUPPORTED beyond).  Inside the image
 *   fl(fl(fl(p / 255) - mean[c]) / std[c]), both divisions IEEE correctly rounded, nothing contracted: the host's
 *   `(to_tensor(u8) - mean) / std`; outside +0.0.  EVERY element of the slot is written: the caller clears nothing.  A lane loads four
 *   pixels and stores 16 bytes where the addresses allow, else element by element. */
int sc2_rcnn_normalize_pad(const uint8_t *pixels, int C, int h, int w, const float *mean, const float *std, float *out, int Hp, int Wp,
                           void *stream);

/* ------------------------------------------------------------------------------------------ */
/* The detector's input transform of a planned COCO batch (csrc/det_input.hip): what ToTensor, the loader's horizontal flip   */
/* and torchvision's GeneralizedRCNNTransform (normalise, bilinear resize, zero-padded batch) do to a list of images, from    */
/* the packed 8-bit sources in ONE launch on `stream`.  tests/ref_det_input.py restates the arithmetic.  No atomics, no       */
/* workspace, nothing is copied to the host.                                                                                  */
/* ------------------------------------------------------------------------------------------ */
#define SC2_DET_INPUT_MAX_BATCH 64      /* samples of one launch: their descriptor rows travel by value in the kernel arguments */
#define SC2_DET_INPUT_ROW_INTS 6        /* int32 words of a descriptor row: offset, h, w, oh, ow, flip */
#define SC2_DET_INPUT_TILE_H 16         /* output rows and columns of a workgroup's tile */
#define SC2_DET_INPUT_TILE_W 256
/* buf : u8 [nbytes] on the device, nbytes in 1..2^31-1 (SC2_ERR_UNSUPPORTED beyond), any alignment.
 * rows: int32 [n][SC2_DET_INPUT_ROW_INTS] ON THE HOST (read before the call returns), n in 1..SC2_DET_INPUT_MAX_BATCH
 *   (SC2_ERR_UNSUPPORTED otherwise: the caller splits).  Row i: the byte offset of the sample's interleaved [h,w,3] RGB image in buf,
 *   h, w, the resized size (oh, ow) -- the caller's: what GeneralizedRCNNTransform.resized_size returns --, flip.  EVERY row is checked
 *   on the host before anything is launched: h, w, oh, ow in 1..SC2_JPEG_IMAGE_MAX_SIDE (SC2_ERR_UNSUPPORTED otherwise);
 *   0 <= offset and offset + 3*h*w <= nbytes, oh <= Hp, ow <= Wp, flip in {0, 1} (SC2_ERR_INVALID_ARG otherwise).  On an error nothing
 *   runs and `out` is untouched.
 * mean, std: 3 floats each ON THE HOST; std[c] != 0 (SC2_ERR_INVALID_ARG).
 * out : f32 [n,3,Hp,Wp] contiguous, 4-byte aligned, Hp and Wp in 1..4 * SC2_JPEG_IMAGE_MAX_SIDE (SC2_ERR_UNSUPPORTED beyond).  EVERY
 *   element is written exactly once: the caller clears nothing.  Outside sample i's (oh, ow) +0.0.  Inside, every operation in f32
 *   and rounded once, nothing contracted:
 *     nrm[c][b] = ((float(b) / 255) - mean[c]) / std[c]      both divisions IEEE correctly rounded: the host's
 *                                                            `(to_tensor(u8) - mean) / std`, as a table of 3 x 256 values
 *     per axis, as aten's upsample_bilinear2d (align_corners=False) when no scale factor is handed down
 *     (F.interpolate(..., recompute_scale_factor=True)), the same as sc2_rcnn_resize_u8's:
 *       scale = in / out;  src = max(scale * (d + 0.5) - 0.5, 0);  i0 = min(int(src), in - 1);  i1 = min(i0 + 1, in - 1);
 *       l1 = src - i0;  l0 = 1 - l1
 *     v = ly0 * (lx0 * p + lx1 * q) + ly1 * (lx0 * s + lx1 * t)   p, q = nrm[c][.] of row j0 at columns i0, i1; s, t of row j1
 *     with flip, source column i is read at w - 1 - i (the flip comes before the resize: ToTensor -> flip -> normalise -> resize).
 *   One workgroup per (sample, SC2_DET_INPUT_TILE_H rows, SC2_DET_INPUT_TILE_W columns) produces the three channels of its tile from
 *   one set of indices and weights; the table is built per workgroup in LDS (3 KB); a lane produces four adjacent pixels of four rows
 *   and stores 16 bytes per channel and row where the address allows, else element by element. */
int sc2_det_input(const uint8_t *buf, long long nbytes, const int32_t *rows, int n, const float *mean, const float *std, float *out,
                  int Hp, int Wp, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Diagnostics (csrc/diag.hip; no product path calls these).                                    */
/* ------------------------------------------------------------------------------------------ */
/* The shader clock the chip holds while OTHER kernels run: `n_workgroups` probe waves (one per workgroup; launch >= 8 so that
 * every XCD gets one) each write n_samples triples (s_memtime, s_memrealtime, XCC id) as u64 into samples[wg][sample][3], one
 * every period_ticks ticks of the constant 100 MHz counter.  clock = delta s_memtime / delta s_memrealtime x 100 MHz between two
 * samples of one workgroup (MI355X_MICROARCH.md, DVFS item 6).  Launch it on a stream of its own BEFORE the kernels under study
 * so that it is resident while they run (tools/clock_probe.py). */
int sc2_clock_probe(unsigned long long *samples, int n_workgroups, int n_samples, unsigned period_ticks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SC2_BOTTLENECK_H */
