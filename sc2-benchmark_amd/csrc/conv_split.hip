// Split-bf16 convolution / GDN1: f32 operands written as sums of NS bf16 parts, the significant cross products accumulated in f32
// on v_mfma_f32_16x16x32_bf16 (`set_encoder_precision('bf16x3' / 'bf16x6')`, include/sc2_bottleneck.h: sc2_conv2d_split_fwd).
//
// Contract:
//   * x = x_0 + x_1 (+ x_2), x_0 = bf16_rne(x), x_1 = bf16_rne(x - x_0), x_2 = bf16_rne(x - x_0 - x_1) (the subtractions are exact
//     in f32); a_op (|x|, x^2) is applied to the f32 value before the split.  The weights arrive split the same way (hip.pack_conv_split).
//     A product of two bf16 numbers is exact in f32: the result differs from the f32 convolution by the dropped products only.
//   * part pairs (i, j) with i + j <= NS - 1 (3 products for NS = 2, 6 for NS = 3), all into the same f32 accumulator, the small
//     terms of a k-step before the large ones; for chunks of <= 48 channels in chains of four k-steps joined by v_add_f32.
//   * implicit GEMM, M = output pixels, N = output channels, K = (kh, kw, ci) with ci fastest on f32 NHWC activations with
//     Cin % 4 == 0.  A k-step is 32 consecutive k = 8 quads of 4; lane (r = l & 15, q = l >> 4) holds, as element j = 0 .. 7,
//         k(s, q, j) = 32 s + 16 (j >> 2) + 4 q + (j & 3)
//     i.e. quads 8 s + q and 8 s + 4 + q: two 16-byte loads, and -- with the weights as the first MFMA operand -- the accumulators
//     of two neighbouring 16-channel tiles ARE the second-operand fragment of the 1x1 GEMM over the channels in this k order.
//     That is what makes conv + GDN1 in one launch (SC2_EPI_FUSED_*) the same sums in the same order as two launches.
//   * a wave owns MT x 16 pixels x NT x 16 channels (one channel chunk); the four waves of a workgroup share the chunk's weight
//     stream through a two-deep LDS ring of G-step groups, one barrier per group; activations are per-wave loads through a
//     bounded buffer descriptor four steps ahead (a tap outside the image, a row past M: an out-of-range offset, zeros).
//   * epilogues and outputs: conv_precise.h, the one copy conv_f32.hip runs too.
#include <stdlib.h>

#include "conv_precise.h"
#include "gfx950_prims.h"

namespace {

struct SplitArgs : PreciseArgs {        // (n_steps = ceil(K / 32))
    const void *__restrict__ w;         // bf16 [chunks][steps][NS][NT][64 lanes][8]
    const void *__restrict__ gamma;     // fused GDN: gamma packed as a 1x1 weight (one chunk), else null
};

typedef f32x4_t sf4_t;
typedef __attribute__((ext_vector_type(4))) unsigned su4_t;

using namespace sc2prim;   // gfx950_prims.h: descriptors, buffer loads
__device__ __forceinline__ su4_t split_buf_load16(buf_rsrc_t r, uint32_t voff) {   // out of range: zeros
    return __builtin_bit_cast(su4_t, buf_load16(r, voff, 0u));
}

// eight f32 values -> NS fragments of eight bf16 each, two elements at a time: one v_cvt_pk_bf16_f32 (round to nearest even)
// makes a dword of the fragment, a shift and a mask give the two parts back as f32, two exact subtractions leave the remainders
template <int NS>
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8_t (&out)[NS]) {
    su4_t o[NS];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float r0 = v[2 * j], r1 = v[2 * j + 1];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            uint32_t pk;                   // {bf16_rne(r0), bf16_rne(r1)}
            asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(pk) : "v"(r0), "v"(r1));
            o[i][j] = pk;
            if (i + 1 < NS) {
                r0 = r0 - __builtin_bit_cast(float, pk << 16);
                r1 = r1 - __builtin_bit_cast(float, pk & 0xFFFF0000u);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) out[i] = __builtin_bit_cast(bf16x8_t, o[i]);
}

template <int NS, int NT, int MT, bool FUSED, int AOP>
__global__ __launch_bounds__(256, 2) void conv_split_kernel(const SplitArgs p) {
    extern __shared__ su4_t smem[];     // [n_steps * 8] int2 tap table, then the weight ring
    constexpr int G = NT == 6 ? 2 : 4;                   // k-steps per ring group
    constexpr int STEP_VECS = NS * NT * 64;              // 16-byte vectors of one k-step of a chunk
    constexpr int VPT = G * STEP_VECS / 256;             // vectors a thread moves per group
    constexpr int NTB = NT == 6 ? 3 : NT;                // channel tiles whose fragments are held at once
    constexpr int D = 4;                                 // k-steps of activations in flight (a multiple of G)
    static_assert(D % G == 0, "prefetch depth");
    static_assert(G * STEP_VECS % 256 == 0, "group size");
    int2 *ktab = reinterpret_cast<int2 *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int n = p.n_steps;
    // (the table runs D steps past the last whole block of steps: those entries are K padding, so the loads that the k loop issues
    //  past the end -- it issues the same loads on every path, which keeps the counted waits exact -- return zeros)
    for (int e = tid; e < ((n + D - 1) / D * D + D) * 8; e += 256) ktab[e] = precise_tap_entry(p, e, p.Cin);

    const long long m_base = ((long long)blockIdx.x * 4 + wave) * (MT * 16);
    const int chunk = blockIdx.y;
    uint32_t a_base[MT];
    int ih0[MT], iw0[MT];
    precise_rows<MT>(p, m_base, r, p.H, p.Cin, a_base, ih0, iw0);

    sf4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = sf4_t{0.f, 0.f, 0.f, 0.f};
    // Short accumulation chains (the narrow tiles, where K is long): the MFMAs of D k-steps accumulate into `acc` from zero, then
    // one v_add_f32 per element (round to nearest even) joins them to the total.  At K = 2 400 one chain of 75 x 3 (x 6) MFMAs
    // measured three times the error of an f32 fma chain.
    constexpr bool CHAIN = NT <= 3;
    sf4_t tot[CHAIN ? MT : 1][CHAIN ? NT : 1];
    if constexpr (CHAIN) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) tot[mt][nt] = sf4_t{0.f, 0.f, 0.f, 0.f};
    }

    const buf_rsrc_t rs_x = make_rsrc(p.x, p.x_bytes);
    const buf_rsrc_t rs_w = make_rsrc(p.w, p.w_bytes);
    su4_t *ring = smem + (p.ring_off >> 4);
    const uint32_t w_chunk = (uint32_t)chunk * (uint32_t)n * (uint32_t)STEP_VECS;     // in vectors
    const uint32_t w_end = w_chunk + (uint32_t)n * (uint32_t)STEP_VECS;
    su4_t wreg[VPT];
    auto fetch_group = [&](int g) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const uint32_t v = w_chunk + (uint32_t)g * (G * STEP_VECS) + (uint32_t)(i * 256 + tid);
            wreg[i] = split_buf_load16(rs_w, v < w_end ? v * 16u : 0x80000000u);
        }
    };
    auto store_group = [&](int g) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) ring[(g & 1) * (G * STEP_VECS) + i * 256 + tid] = wreg[i];
    };
    struct ASet { su4_t v[MT][2]; };
    auto load_a = [&](int s, ASet &a) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int2 t = ktab[s * 8 + h * 4 + q];
            const int kh = t.y & 0xFFFF, kw = t.y >> 16;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bool ok = ((unsigned)(ih0[mt] + kh) < (unsigned)p.H) & ((unsigned)(iw0[mt] + kw) < (unsigned)p.W);
                a.v[mt][h] = split_buf_load16(rs_x, ok ? a_base[mt] + (uint32_t)t.x : 0x80000000u);
            }
        }
    };
    // the MFMAs of one k-step: xa = the split activations, wsrc = the step's weight fragments [NS][NT][64]
    auto mma_step = [&](const bf16x8_t (&xa)[MT][NS], const su4_t *wsrc) {
#pragma unroll
        for (int nb = 0; nb < NT; nb += NTB) {
            bf16x8_t wb[NTB][NS];
#pragma unroll
            for (int t = 0; t < NTB; ++t)
#pragma unroll
                for (int j = 0; j < NS; ++j) wb[t][j] = __builtin_bit_cast(bf16x8_t, wsrc[(j * NT + nb + t) * 64 + lane]);
#pragma unroll
            for (int d = NS - 1; d >= 0; --d)            // part index sum: the small terms first
#pragma unroll
                for (int i = d; i >= 0; --i)             // (x part i, w part d - i)
#pragma unroll
                    for (int t = 0; t < NTB; ++t)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            acc[mt][nb + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[t][d - i], xa[mt][i], acc[mt][nb + t], 0, 0, 0);
        }
    };
    // one k-step: split the landed activations, re-use their registers for the load of step s + D, multiply
    auto step = [&](int s, int g, int i_in_group, ASet &cur) {
        bf16x8_t xa[MT][NS];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t u = cur.v[mt][j >> 2][j & 3];      // (a copy: bit_cast of the vector element itself reads element 0)
                const float f = __builtin_bit_cast(float, u);
                v[j] = AOP == SC2_AOP_ABS ? fabsf(f) : (AOP == SC2_AOP_SQUARE ? f * f : f);
            }
            split8<NS>(v, xa[mt]);
        }
        load_a(s + D, cur);
        if (s < n) mma_step(xa, ring + (g & 1) * (G * STEP_VECS) + i_in_group * STEP_VECS);
    };

    // activations D steps ahead in D register sets (step s lives in a[s % D]); weights one group ahead
    ASet a[D];
    fetch_group(0);
    __syncthreads();                                     // the tap table
#pragma unroll
    for (int i = 0; i < D; ++i)
        load_a(i, a[i]);
    store_group(0);
    __syncthreads();
    for (int s0 = 0; s0 < n; s0 += D) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int s = s0 + i, g = s0 / G + i / G;
            // the next group's fragments travel behind this group's MFMAs; past the end: zeros nobody reads
            if (i % G == 0) fetch_group(g + 1);
            step(s, g, i % G, a[i]);
            if (i % G == G - 1) {
                // every wave has passed the barrier that ended group g - 1, so nobody reads the other half of the ring any more
                store_group(g + 1);
                __syncthreads();
            }
        }
        if constexpr (CHAIN) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    tot[CHAIN ? mt : 0][CHAIN ? nt : 0] += acc[mt][nt];
                    acc[mt][nt] = sf4_t{0.f, 0.f, 0.f, 0.f};
                }
        }
    }
    if constexpr (CHAIN) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = tot[CHAIN ? mt : 0][CHAIN ? nt : 0];
    }

    // conv FOLLOWED BY GDN1 in the same launch: norm = gamma |acc| as a split GEMM over the channels, in the k order of the
    // separate launch (see the header).  Tiles past NT are the zero channels of the K padding.
    sf4_t nrm[FUSED ? MT : 1][FUSED ? NT : 1];
    if constexpr (FUSED) {
        const su4_t *gf = reinterpret_cast<const su4_t *>(p.gamma);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) nrm[mt][nt] = sf4_t{0.f, 0.f, 0.f, 0.f};
        constexpr int NSTEP = (NT + 1) / 2;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            bf16x8_t xa[MT][NS];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int t = 2 * s + (j >> 2);
                    v[j] = t < NT ? fabsf(acc[mt][t < NT ? t : 0][j & 3]) : 0.f;
                }
                split8<NS>(v, xa[mt]);
            }
            const su4_t *wsrc = gf + s * STEP_VECS;
#pragma unroll
            for (int nb = 0; nb < NT; nb += NTB) {
                bf16x8_t wb[NTB][NS];
#pragma unroll
                for (int t = 0; t < NTB; ++t)
#pragma unroll
                    for (int j = 0; j < NS; ++j) wb[t][j] = __builtin_bit_cast(bf16x8_t, wsrc[(j * NT + nb + t) * 64 + lane]);
#pragma unroll
                for (int d = NS - 1; d >= 0; --d)
#pragma unroll
                    for (int i = d; i >= 0; --i)
#pragma unroll
                        for (int t = 0; t < NTB; ++t)
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt)
                                nrm[mt][nb + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[t][d - i], xa[mt][i], nrm[mt][nb + t], 0, 0, 0);
            }
        }
    }

    precise_epilogue<MT, NT, FUSED>(p, acc, nrm, m_base, chunk, r, q);
}

template <int NS, int NT, int MT, bool FUSED, int AOP>
int launch_split(const SplitArgs &a, int chunks, hipStream_t s) {
    constexpr int G = NT == 6 ? 2 : 4;
    const long long tiles = (a.M + (4 * MT * 16) - 1) / (4 * MT * 16);
    SplitArgs b = a;
    b.ring_off = (unsigned)(((size_t)((a.n_steps + 3) / 4 * 4 + 4) * 8 * sizeof(int2) + 1023) / 1024 * 1024);   // (D = 4 in the kernel)
    b.w_bytes = (unsigned)((size_t)chunks * a.n_steps * NS * NT * 1024);
    const size_t lds = (size_t)b.ring_off + 2 * (size_t)G * NS * NT * 1024;
    constexpr auto kern = &conv_split_kernel<NS, NT, MT, FUSED, AOP>;
    SC2_REQUIRE(lds <= 64 * 1024 || precise_raise_lds_limit<kern>(lds), SC2_ERR_UNSUPPORTED,
                "conv2d_split: %zu bytes of LDS are not available", lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, (unsigned)chunks), dim3(256), lds, s, b);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

template <int NS, int NT>
int dispatch_aop(const SplitArgs &a, int chunks, bool fused, hipStream_t s) {
    if (fused) return launch_split<NS, NT, 2, true, SC2_AOP_NONE>(a, chunks, s);
    if (a.a_op == SC2_AOP_ABS) return launch_split<NS, NT, 2, false, SC2_AOP_ABS>(a, chunks, s);
    if (a.a_op == SC2_AOP_SQUARE) return launch_split<NS, NT, 2, false, SC2_AOP_SQUARE>(a, chunks, s);
    return launch_split<NS, NT, 2, false, SC2_AOP_NONE>(a, chunks, s);
}

template <int NS>
int dispatch_split(const SplitArgs &a, int cc, int chunks, bool fused, hipStream_t s) {
    if (cc == 32) return dispatch_aop<NS, 2>(a, chunks, fused, s);
    if (cc == 48) return dispatch_aop<NS, 3>(a, chunks, fused, s);
    return dispatch_aop<NS, 6>(a, chunks, fused, s);
}

}  // namespace

extern "C" int sc2_conv_split_chunk_channels(int Cout) { return precise_chunk_channels(Cout); }

extern "C" int sc2_conv2d_split_fwd(const sc2_conv_desc *d, int n_parts, const float *x, const void *w_frag, void *y, const float *ep_x,
                                    const void *gamma_frag, const float *ep_beta, void *stream) {
    SC2_REQUIRE(d && x && w_frag && y, SC2_ERR_INVALID_ARG, "conv2d_split: null argument");
    SC2_REQUIRE(n_parts == 2 || n_parts == 3, SC2_ERR_UNSUPPORTED, "conv2d_split: n_parts %d (2 or 3)", n_parts);
    if (const int rc = precise_check_desc("conv2d_split", d, ep_x, gamma_frag, ep_beta)) return rc;
    SC2_REQUIRE(d->k_order == 0, SC2_ERR_UNSUPPORTED, "conv2d_split: f32 NHWC input only");
    const bool fused = d->epilogue == SC2_EPI_FUSED_GDN || d->epilogue == SC2_EPI_FUSED_IGDN;
    const bool gdn = d->epilogue == SC2_EPI_GDN || d->epilogue == SC2_EPI_IGDN || d->epilogue == SC2_EPI_GDN2 || d->epilogue == SC2_EPI_IGDN2;
    SC2_REQUIRE(!fused || d->a_op == SC2_AOP_NONE, SC2_ERR_UNSUPPORTED, "conv2d_split: the fused GDN takes a_op NONE");
    const int cc = sc2_conv_split_chunk_channels(d->Cout);
    SplitArgs a;
    precise_fill_args(a, d, x, gdn ? ep_x : nullptr, ep_beta, y);
    a.w = w_frag; a.gamma = fused ? gamma_frag : nullptr;
    a.n_steps = (d->KH * d->KW * d->Cin + 31) / 32;
    const long long xb = (long long)d->N * d->H * d->W * d->Cin * 4;
    SC2_REQUIRE(xb < 0x7FF00000LL, SC2_ERR_UNSUPPORTED, "conv2d_split: input of %lld bytes exceeds 2 GB", xb);
    a.x_bytes = (unsigned)xb;
    SC2_REQUIRE(a.M < (1ll << 31) && a.M * d->Cout < (1ll << 33), SC2_ERR_UNSUPPORTED,
                "conv2d_split: tensor too large for this kernel's index arithmetic");
    SC2_REQUIRE((size_t)(a.n_steps + 8) * 64 <= 32 * 1024, SC2_ERR_UNSUPPORTED, "conv2d_split: K too long for the tap table");
    const int chunks = (d->Cout + cc - 1) / cc;
    SC2_REQUIRE((long long)chunks * a.n_steps * n_parts * (cc / 16) * 1024 < 0x7FF00000LL, SC2_ERR_UNSUPPORTED, "conv2d_split: weight stream too large");
    a.w_bytes = 0u;
    a.ring_off = 0u;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_parts == 2) return dispatch_split<2>(a, cc, chunks, fused, s);
    return dispatch_split<3>(a, cc, chunks, fused, s);
}
