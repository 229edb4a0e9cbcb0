// 1x1 convolution + bias (+ residual) (+ ReLU) for the long-K, compute-heavy 1x1 layers of the ResNet tail (gfx950): conv1 of
// layer3 / layer4, layer4's conv3 and the two stride-2 downsample layers in eval mode (torchvision Bottleneck blocks, the callers on
// the far side of the bottleneck path, sc2bench/models/backbone.py:235-254).
//     y[m, co] = act( sum_ci x[pix(m), ci] w[co, ci] + bias[co] (+ res[m, co]) ),   bf16 NHWC, m = flat output pixel.
//
// Why a third long-K 1x1 kernel.  conv1x1_kres.hip (one wave per SIMD, 32 pixels x 128 channels per unit, K-half exchange and
// epilogue serial behind the MFMAs) and conv1x1_win.hip (four waves, 208 pixels x 128 channels, ~1 000 cycles per k-step against 416
// of MFMA issue) leave these layers at 0.11 - 0.27 of the matrix pipe, while dec.conv4 -- the same GEMM as conv1 of layer3, K = 1024,
// N = 256 -- runs at 1.18 PFLOP/s on conv2x2_win.hip.  This file is conv2x2_win.hip's K loop REDUCED TO ONE TAP (that reads shorter
// than conv1x1_win.hip widened: the eight-wave frame, the chained fragment ring and the joined tiles are all there already), with
// conv1x1_win.hip's window fill, weight stream and epilogue:
//   * 512 threads = eight waves, two per SIMD (<= 256 VGPRs); a tile is 224 consecutive output pixels (14 MFMA row tiles) x 256
//     channels, wave w owns channels [32 w, 32 w + 32) of every pixel (28 accumulator tiles): each staged pixel byte feeds twice the
//     channels it does in the two older kernels;
//   * the pixel operand is staged per 128-channel slab as sixteen 16-byte-chunk planes [chunk][pixel][16 B] (64 KB), ring of two:
//     fragment reads are ONE address register + immediates (k-step KS: planes 4 KS .. 4 KS + 3, row tile i: + 256 i), no vector ALU
//     inside a slab, one barrier per slab (112 MFMAs per wave), reads seven row tiles ahead and chained across the k-steps of a slab
//     (conv2x2_win.hip, mma_step); stride 2 only changes the fill addresses;
//   * weights L2 -> registers, fragment-major, four k-steps ahead, inline-asm loads with hand-counted vmcnt waits (the rules are in the
//     header of conv2x2_win.hip); the stream is hip.pack_conv_win(w), conv1x1_win.hip's: no new layout;
//   * epilogue in registers in conv1x1_win.hip's operation order -- (acc + bias) (+ residual), ReLU, one rounding -- and one ascending-k
//     chain per output element from a zero accumulator: results are BIT-IDENTICAL to sc2_conv1x1_win_fwd's on the same operands.
//
// The choices the structure leaves open:
//   * slab width 128 channels, ring depth 2: a slab is 3.2 us of MFMA work per CU at dec.conv4's rate, so ONE slab ahead covers the
//     ~2 us of a loaded HBM round trip (conv1x1_win.hip's 64-channel slab of a 208 x 128 tile is 0.5 us and needed three ahead); four
//     k-steps per slab make the ring slot of a weight fragment its k-step, as the four taps do in conv2x2_win.hip; 2 x 64 KB of LDS.
//     The slab loop runs one slab per trip with the ring half as a runtime value (one vector add per slab), so any Cin % 128 == 0
//     works, Cin = 128 (one trip) included;
//   * tiles are claimed by a STATIC interleave: at most one workgroup per CU, workgroup slot s runs units s, s + G, s + 2 G, ...
//     (unit = pixel tile x 256-channel chunk, chunk fastest; XCD-contiguous slots so that the chunks of one pixel tile read their
//     pixels through one L2).  Units of a launch cost the same, so a counter would balance nothing a stride does not; nobody waits
//     for anybody.  The run length is whatever the share is (1 - 4 units at bs 256): the NEXT unit's first slab and first four
//     k-steps of weights are in flight during the current unit's last slab, so the K loops of successive units join without a bubble;
//   * ONE instruction stream for the first and the later units of a workgroup: the prologue issues fourteen out-of-range (dropped)
//     stores behind its fetches, so the first unit's first slab sees exactly the vector-memory history a later unit's does (the
//     previous unit's fourteen output stores) and every wait count is a compile-time constant that tools/audit_vmcnt.py --counts can
//     follow path-insensitively (conv2x2_win.hip branches between two constants there and stays outside that audit);
//   * the bias of the lane's eight channels is fetched by two asm loads at EVERY slab start (the counts stay the same on every path)
//     and waited for behind the last slab's fetches: a compiler-tracked load in the epilogue would wait vmcnt(0), i.e. for the next
//     unit's fragments.
// RELU and the residual are template parameters (four instantiations): the epilogue has no runtime branch.
//
// WHAT GUARDS THIS FILE.  Its correctness rests on two things no GPU test can promise for the next compiler: the fragment, bias and
// ring registers (bq, c_lo / c_hi) keep their physical registers from an asm load to its counted wait -- across the peeled slab, the
// slab loop and the epilogue -- with nothing copied, spilled or reused in between, and vmcnt retires loads and stores in issue order.
// tests/test_conv1x1_w8_cpu.py runs tools/audit_vmcnt.py --counts / --copies / --stores and tools/audit_inflight.py on the listing hipcc
// produces and reads the built code objects' register and scratch counts: it MUST be rerun on every ROCm update, together with the
// bit-equality tests of tests/test_gpu_conv1x1_w8.py (five launches behind another shape), as for conv2x2_win.hip.
#include <stdlib.h>

#include "gfx950_prims.h"

namespace {

using namespace sc2prim;   // gfx950_prims.h: descriptors, buffer access, the asm weight loads, counted waits (rules (i) - (iv)), LDS asm

struct W8Args {
    const uint16_t *__restrict__ x;      // bf16 NHWC [N, H, W, Cin]
    const uint16_t *__restrict__ w;      // bf16 [Cin/32][Cout/16][64][8]  (hip.pack_conv_win of the [Cout, Cin, 1, 1] weight)
    const float *__restrict__ bias;      // f32 [Cout]
    const uint16_t *__restrict__ res;    // bf16 [M, Cout] or null
    uint16_t *__restrict__ y;            // bf16 [M, Cout], M = N * OH * OW
    int N, H, W, OH, OW, stride, Cin, Cout;
    int n_chunks;                        // Cout / 256
    int n_units;                         // pixel tiles x n_chunks
    int M;
    unsigned x_bytes, w_bytes, y_bytes;
};

constexpr int MT = 14;                   // MFMA row tiles per tile
constexpr int PX = MT * 16;              // 224 output pixels per tile
constexpr int NRG = 4;                   // 64-row direct-to-LDS pieces per plane (the last one half used)
constexpr int PLANE = NRG * 1024;        // bytes per 16-byte-chunk plane
constexpr int NPLANE = 16;               // planes per slab = 128 channels
constexpr int WIN_BYTES = NPLANE * PLANE;   // 64 KB; two of them form the ring
constexpr int LDS_BYTES = 2 * WIN_BYTES;
constexpr int PF = 4;                    // weight fragments are fetched this many k-steps ahead (= k-steps per slab: ring slot = k-step of the slab)
constexpr int NFILL = 2 * NRG;           // window pieces per wave and slab start (two planes)
constexpr int NBIAS = 2;                 // bias loads per slab start
constexpr int NSTORE = MT;               // output stores per lane and unit, ALWAYS issued (masked ones out of range)
// vmcnt budget of a k-step's wait for its own two fragments (issue order, oldest first): [its two loads], the six loads of the three
// k-steps behind it and -- always inside those four k-steps -- the pieces and bias loads of ONE slab start.  The four k-steps of a
// unit's first slab were fetched across the previous unit's epilogue (the prologue's dummy stores for the first unit): + NSTORE.
constexpr int VM_STEP = 2 * (PF - 1) + NFILL + NBIAS;
// ... of a slab start's wait for this wave's window pieces: issued at the previous slab start, in front of its 2 PF fetches.  The bias
// loads of a slab start go FIRST, so this wait lands the previous slab's as well: their registers are dead from the slab start to
// the new loads, and nothing the compiler places there may be overwritten by a load still in flight.
constexpr int VM_SLAB = 2 * PF;
static_assert(3 * 4 * PLANE + (MT - 1) * 256 < 65536, "16-bit immediates");
static_assert(VM_STEP + NSTORE < 64, "6-bit vmcnt");

constexpr int NO_NEXT = -1;
// One k-step: 14 pixel fragments x 2 weight fragments, the fragment reads seven row tiles ahead through seven register quads, in the
// operand-stationary order, chained to the next k-step of the slab (PRE: the first seven fragments are in flight already; OFF_NEXT:
// read the next step's first seven while row tiles 7 .. 13 are multiplied) -- conv2x2_win.hip, mma_step, which has the notes.
template <int OFF, int NVM, bool PRE, int OFF_NEXT>
__device__ __forceinline__ void mma_step(f32x4_t (&acc)[MT][2], uint32_t a_base, u32x4_t &b0, u32x4_t &b1, u32x4_t (&av)[7]) {
    if constexpr (!PRE) {
#define SC2_W8_RD(i) av[i] = lds_read16_imm<OFF + (i) * 256>(a_base);
        SC2_W8_RD(0) SC2_W8_RD(1) SC2_W8_RD(2) SC2_W8_RD(3) SC2_W8_RD(4) SC2_W8_RD(5) SC2_W8_RD(6)
#undef SC2_W8_RD
    }
    __builtin_amdgcn_sched_barrier(0);
    wait_vm<NVM>();
    const bf16x8_t bf0 = __builtin_bit_cast(bf16x8_t, b0), bf1 = __builtin_bit_cast(bf16x8_t, b1);
#define SC2_W8_PASS_A(i, NWAIT)                                                                 \
    {                                                                                           \
        wait_lgkm<NWAIT>(av[(i) % 7]);                                                          \
        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf0, __builtin_bit_cast(bf16x8_t, av[(i) % 7]), acc[i][0], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                      \
    }
#define SC2_W8_PASS_B(i)                                                                        \
    {                                                                                           \
        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf1, __builtin_bit_cast(bf16x8_t, av[(i) % 7]), acc[i][1], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                      \
        if constexpr ((i) + 7 < 14) av[(i) % 7] = lds_read16_imm<OFF + ((i) + 7 < 14 ? (i) + 7 : 0) * 256>(a_base); \
        else if constexpr (OFF_NEXT != NO_NEXT)                                                 \
            av[(i) % 7] = lds_read16_imm<(OFF_NEXT != NO_NEXT ? OFF_NEXT : 0) + ((i) >= 7 ? (i) - 7 : 0) * 256>(a_base); \
        __builtin_amdgcn_sched_barrier(0);                                                      \
    }
    // (waits: nothing is read during a pass A, so tile i's wait leaves the 6 - i / 13 - i younger reads of its half outstanding)
    SC2_W8_PASS_A(0, 6) SC2_W8_PASS_A(1, 5) SC2_W8_PASS_A(2, 4) SC2_W8_PASS_A(3, 3) SC2_W8_PASS_A(4, 2) SC2_W8_PASS_A(5, 1) SC2_W8_PASS_A(6, 0)
    SC2_W8_PASS_B(0) SC2_W8_PASS_B(1) SC2_W8_PASS_B(2) SC2_W8_PASS_B(3) SC2_W8_PASS_B(4) SC2_W8_PASS_B(5) SC2_W8_PASS_B(6)
    SC2_W8_PASS_A(7, 6) SC2_W8_PASS_A(8, 5) SC2_W8_PASS_A(9, 4) SC2_W8_PASS_A(10, 3) SC2_W8_PASS_A(11, 2) SC2_W8_PASS_A(12, 1) SC2_W8_PASS_A(13, 0)
    SC2_W8_PASS_B(7) SC2_W8_PASS_B(8) SC2_W8_PASS_B(9) SC2_W8_PASS_B(10) SC2_W8_PASS_B(11) SC2_W8_PASS_B(12) SC2_W8_PASS_B(13)
#undef SC2_W8_PASS_A
#undef SC2_W8_PASS_B
}

template <bool RELU, bool HAS_RES>
__global__ __launch_bounds__(512, 2) void conv1x1_w8_kernel(const W8Args p) {
    constexpr uint32_t OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_ptr_t)smem;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fq = lane >> 4;
    const int Cin = p.Cin, Cout = p.Cout;
    const int NS = Cin >> 7;                 // 128-channel slabs
    const uint32_t KT = (uint32_t)NS * 4u;   // k-steps

    // slot of this workgroup: XCD x (blockIdx & 7) gets a contiguous range of slots, i.e. of (pixel tile, channel chunk) pairs with
    // the chunk fastest: the chunks of one pixel tile read their window through the same L2
    const int G = gridDim.x;
    int slot = blockIdx.x;
    {
        const int xcd = slot & 7, q = G >> 3, r = G & 7;
        const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        slot = base + (slot >> 3);
    }
    if (slot >= p.n_units) return;   // (never: the grid is at most n_units)

    const buf_rsrc_t rs_x = make_rsrc(p.x, p.x_bytes);
    const i32x4_t rs_w = rsrc_words(p.w, p.w_bytes);
    const i32x4_t rs_b = rsrc_words(p.bias, (uint32_t)Cout * 4u);
    const buf_rsrc_t rs_y = make_rsrc(p.y, p.y_bytes);
    [[maybe_unused]] const buf_rsrc_t rs_r = make_rsrc(HAS_RES ? p.res : p.y, HAS_RES ? p.y_bytes : 0u);

    // (readfirstlane: hipcc divides wave-uniform integers in the vector ALU)
    auto unit_chunk = [&](int unit) { return __builtin_amdgcn_readfirstlane(unit % p.n_chunks); };
    auto unit_m0 = [&](int unit) { return __builtin_amdgcn_readfirstlane(unit / p.n_chunks) * PX; };

    // window fill: wave w fills chunk planes 2 w and 2 w + 1 (plane c = channels [8 c, 8 c + 8) of the slab); piece j = rows
    // [64 j, 64 j + 64) = output pixels m0 + 64 j + lane.  The per-lane source offsets of the unit being filled stay in registers.
    uint32_t pw_vo[NRG];
    auto window_offsets = [&](int unit, bool live) {   // live = false: every lane out of range (zeros into a dead buffer)
        const int m0 = unit_m0(unit);
        int ln;   // (volatile: computed where it is used)
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        if (p.stride != 1) {
            const uint32_t ohw = (uint32_t)(p.OH * p.OW);
#pragma unroll
            for (int j = 0; j < NRG; ++j) {
                const int m = m0 + j * 64 + ln;
                const bool ok = live & (j * 64 + ln < PX) & (m < p.M);
                const uint32_t mc = ok ? (uint32_t)m : 0u;
                const uint32_t n = mc / ohw, rem = mc - n * ohw;
                const uint32_t oh = rem / (uint32_t)p.OW, ow = rem - oh * (uint32_t)p.OW;
                const uint32_t pix = (n * (uint32_t)p.H + oh * (uint32_t)p.stride) * (uint32_t)p.W + ow * (uint32_t)p.stride;
                pw_vo[j] = ok ? pix * (uint32_t)Cin * 2u : OOB;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NRG; ++j) {
                const int m = m0 + j * 64 + ln;
                const bool ok = live & (j * 64 + ln < PX) & (m < p.M);
                pw_vo[j] = ok ? (uint32_t)m * (uint32_t)Cin * 2u : OOB;
            }
        }
    };
    auto issue_window = [&](int cb, int par) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int j = 0; j < NRG; ++j)
                buf_load_lds16(rs_x, (lds_ptr_t)(smem + par * WIN_BYTES + (wave * 2 + c) * PLANE + j * 1024), pw_vo[j],
                               (uint32_t)cb * 256u + (uint32_t)(wave * 2 + c) * 16u);
        }
    };

    // fragment row of this lane in row tile 0 of k-step 0 of ring half 0: k-lanes fq = chunk fq of the k-step's four planes
    const uint32_t a_base0 = lds_base + (uint32_t)(fq * PLANE + frow * 16);
    // weights: k-step kt, 16-channel tile t -> 1 KB at ((kt * Cout/16) + t) * 1024; this wave's tiles are n0/16, n0/16 + 1
    const uint32_t b_vo = (uint32_t)(lane * 16);
    const uint32_t b_step = (uint32_t)(Cout >> 4) * 1024u;
    auto unit_b_so = [&](int unit) { return (uint32_t)((unit_chunk(unit) * 256 + wave * 32) >> 4) * 1024u; };
    uint32_t b_so_cur, b_so_next;
    auto fetch_b = [&](uint32_t k, u32x4_t &b0, u32x4_t &b1) {   // k in [0, 2 KT): wraps to the next unit's first k-steps
        // (readfirstlane: wave-uniform by construction, and an "s" operand of the asm must BE a scalar register whatever the
        //  divergence analysis made of the loop-carried unit index)
        const uint32_t so = (uint32_t)__builtin_amdgcn_readfirstlane((int)(k >= KT ? b_so_next + (k - KT) * b_step : b_so_cur + k * b_step));
        wload16(b0, rs_w, b_vo, so);
        wload16(b1, rs_w, b_vo, so + 1024u);
    };
    // bias of this lane's eight channels n0 + 8 fq + [0, 8) of the current unit
    const uint32_t c_vo = (uint32_t)(fq * 32);
    u32x4_t c_lo, c_hi;

    f32x4_t acc[MT][2];
    u32x4_t av[7];   // the fragment ring (mma_step): lives across the chained k-steps
    u32x4_t bq[PF][2];

    int unit = slot;
    int par = 0;     // ring half of the slab about to be multiplied
    b_so_cur = unit_b_so(unit);
    b_so_next = b_so_cur;
    window_offsets(unit, true);
    issue_window(0, 0);
#pragma unroll
    for (int s = 0; s < PF; ++s) fetch_b((uint32_t)s, bq[s][0], bq[s][1]);
    // the stand-ins for "the previous unit's output stores" (header): out of range, dropped
#pragma unroll
    for (int i = 0; i < NSTORE; ++i) buf_store16(rs_y, OOB, 0u, u32x4_t{0u, 0u, 0u, 0u});

    for (;;) {
        const bool has_next = unit + G < p.n_units;
        const int unit_next = has_next ? unit + G : unit;
        b_so_next = unit_b_so(unit_next);   // (no next unit: this unit's first k-steps again, never used)
        const uint32_t c_so = (uint32_t)((unit_chunk(unit) * 256 + wave * 32) * 4);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            acc[i][0] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            acc[i][1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }

        // k-step KS of slab cb: its fragments were fetched four k-steps ago; the fetch of k-step + 4 goes into the same registers
        // behind the step's last MFMA
#define SC2_W8_STEP(cb, KS, SLAB0)                                                                                      \
    {                                                                                                                   \
        mma_step<(KS) * 4 * PLANE, VM_STEP + ((SLAB0) ? NSTORE : 0), ((KS) > 0), ((KS) < 3 ? ((KS) + 1) * 4 * PLANE : NO_NEXT)>( \
            acc, a_cur, bq[KS][0], bq[KS][1], av);                                                                      \
        fetch_b((uint32_t)(cb) * 4u + ((KS) + PF), bq[KS][0], bq[KS][1]);                                               \
    }
#define SC2_W8_SLAB(cb, SLAB0)                                                                                          \
    {                                                                                                                   \
        /* this wave's share of the slab's window has landed: it is older than the 2 PF fetches of the previous slab          \
           and, in the first slab of a unit, than the previous unit's output stores (the prologue's stand-ins) */       \
        wait_vm<VM_SLAB + ((SLAB0) ? NSTORE : 0)>();                                                                    \
        __builtin_amdgcn_s_barrier();   /* window complete; everybody is done with the previous slab's window */        \
        /* EVERY slab start issues two bias loads and this wave's eight window pieces: the next slab's pieces, or the next \
           unit's first window, or -- behind the workgroup's last unit -- zeros into the dead ring half */              \
        cload16(c_lo, rs_b, c_vo, c_so);                                                                                \
        cload16(c_hi, rs_b, c_vo, c_so + 16u);                                                                          \
        /* (ONE copy of the eight loads behind a conditional change of their offsets: as the two arms of an if / else hipcc  \
           laid them out as two correlated branches, which the path-insensitive count audit cannot pair up) */          \
        if ((cb) + 1 >= NS) window_offsets(unit_next, has_next);                                                        \
        issue_window((cb) + 1 < NS ? (cb) + 1 : 0, par ^ 1);                                                            \
        const uint32_t a_cur = a_base0 + (uint32_t)par * (uint32_t)WIN_BYTES;                                           \
        SC2_W8_STEP(cb, 0, SLAB0) SC2_W8_STEP(cb, 1, SLAB0) SC2_W8_STEP(cb, 2, SLAB0) SC2_W8_STEP(cb, 3, SLAB0)         \
        par ^= 1;                                                                                                       \
    }
        // the first slab peeled (its waits count the stores in front of it), then one slab per trip
        SC2_W8_SLAB(0, true)
        for (int cb = 1; cb < NS; ++cb) SC2_W8_SLAB(cb, false)
#undef SC2_W8_SLAB
#undef SC2_W8_STEP

        // ---- output.  Lane (frow, fq) holds, for row tile i, channels n0 + 8 fq + [0, 4) in acc[i][0] and + [4, 8) in acc[i][1]
        // (the packing permutes the weight rows that way) of pixel m0 + 16 i + frow.  Masked lanes go out of the descriptor's
        // range: ALWAYS fourteen store instructions per unit, which the counted waits of the next unit's first slab rely on.
        // The bias loads of the last slab start have that start's window pieces and the slab's 2 PF fetches behind them.
        wait_vm_tied<NFILL + 2 * PF>(c_lo, c_hi);
        const float4 bias_lo = __builtin_bit_cast(float4, c_lo), bias_hi = __builtin_bit_cast(float4, c_hi);
        const int m0 = unit_m0(unit);
        const uint32_t y_so = ((uint32_t)m0 * (uint32_t)Cout + (uint32_t)(unit_chunk(unit) * 256 + wave * 32)) * 2u;   // unit base (bytes), scalar
        int ln_o;   // the lane index, computed HERE (volatile): the per-row-tile offsets derived from it are recomputed per unit, not held
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln_o));   // across the K loop
        const int fr = ln_o & 15, fqo = ln_o >> 4;
        auto out_off = [&](int i) -> uint32_t {
            const int ml = i * 16 + fr;
            return m0 + ml < p.M ? (uint32_t)ml * (uint32_t)Cout * 2u + (uint32_t)(fqo * 16) : OOB;
        };
        // (two batches of seven row tiles: fourteen residual quads in flight beside the next unit's fragments do not fit)
#define SC2_W8_FIN(i0)                                                                                                      \
    {                                                                                                                       \
        [[maybe_unused]] uint4 rv[7];                                                                                       \
        if constexpr (HAS_RES) {                                                                                            \
            _Pragma("unroll") for (int k = 0; k < 7; ++k) rv[k] = buf_load16(rs_r, out_off((i0) + k), y_so);                \
        }                                                                                                                   \
        _Pragma("unroll") for (int k = 0; k < 7; ++k) {                                                                     \
            const int i = (i0) + k;                                                                                         \
            float v[8] = {acc[i][0][0] + bias_lo.x, acc[i][0][1] + bias_lo.y, acc[i][0][2] + bias_lo.z, acc[i][0][3] + bias_lo.w, \
                          acc[i][1][0] + bias_hi.x, acc[i][1][1] + bias_hi.y, acc[i][1][2] + bias_hi.z, acc[i][1][3] + bias_hi.w}; \
            if constexpr (HAS_RES) {                                                                                        \
                v[0] += bf_lo(rv[k].x); v[1] += bf_hi(rv[k].x); v[2] += bf_lo(rv[k].y); v[3] += bf_hi(rv[k].y);             \
                v[4] += bf_lo(rv[k].z); v[5] += bf_hi(rv[k].z); v[6] += bf_lo(rv[k].w); v[7] += bf_hi(rv[k].w);             \
            }                                                                                                               \
            if constexpr (RELU) {                                                                                           \
                _Pragma("unroll") for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);                                      \
            }                                                                                                               \
            buf_store16(rs_y, out_off(i), y_so, u32x4_t{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])}); \
        }                                                                                                                   \
    }
        SC2_W8_FIN(0)
        SC2_W8_FIN(7)
#undef SC2_W8_FIN
        if (!has_next) break;
        unit = unit_next;
        b_so_cur = b_so_next;
    }
    // The last unit fetched "its first k-steps again" (never used): those loads may still be in flight, and the compiler regards
    // their registers as dead from here on.  The wait names them, which keeps them allocated up to it (conv1x1_win.hip).
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(bq[0][0]), "+v"(bq[0][1]), "+v"(bq[1][0]), "+v"(bq[1][1]), "+v"(bq[2][0]), "+v"(bq[2][1]), "+v"(bq[3][0]),
                   "+v"(bq[3][1])::"memory");
}

template <bool RELU, bool HAS_RES>
int launch_w8(const W8Args &a, hipStream_t s) {
    static bool attr_set_dev[SC2_MAX_DEVICES] = {};
    bool &attr_set = attr_set_dev[sc2_device_slot()];
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&conv1x1_w8_kernel<RELU, HAS_RES>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  LDS_BYTES);
        attr_set = true;
    }
    // one workgroup per CU at most (128 KB of LDS, 512 threads at the register cap): more units than CUs run as static shares
    const int cus = sc2_device_cus() > 0 ? sc2_device_cus() : 1;
    const int grid = a.n_units < cus ? a.n_units : cus;
    hipLaunchKernelGGL((conv1x1_w8_kernel<RELU, HAS_RES>), dim3((unsigned)grid), dim3(512), LDS_BYTES, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

}  // namespace

extern "C" int sc2_conv1x1_w8_supported(int Cin, int Cout, int stride) {
    return (stride == 1 || stride == 2) && Cin >= 128 && Cin % 128 == 0 && Cout >= 256 && Cout % 256 == 0 ? 1 : 0;
}

extern "C" int sc2_conv1x1_w8_fwd(const void *x, const void *w_frag, const float *bias, const void *residual, void *y, int N, int H, int W,
                                  int Cin, int Cout, int stride, int relu, void *stream) {
    SC2_REQUIRE(x && w_frag && bias && y, SC2_ERR_INVALID_ARG, "conv1x1_w8: null argument");
    SC2_REQUIRE(N > 0 && H > 0 && W > 0, SC2_ERR_INVALID_ARG, "conv1x1_w8: non-positive shape");
    SC2_REQUIRE(sc2_conv1x1_w8_supported(Cin, Cout, stride), SC2_ERR_UNSUPPORTED,
                "conv1x1_w8: needs Cin %% 128 == 0, Cout %% 256 == 0, stride 1 or 2 (got %d -> %d, stride %d)", Cin, Cout, stride);
    const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
    const long long M = (long long)N * OH * OW;
    const long long x_bytes = (long long)N * H * W * Cin * 2, w_bytes = (long long)Cin * Cout * 2, y_bytes = M * Cout * 2;
    SC2_REQUIRE(x_bytes < 0x7FF00000LL && w_bytes < 0x7FF00000LL && y_bytes < 0x7FF00000LL, SC2_ERR_UNSUPPORTED,
                "conv1x1_w8: operand of %lld bytes exceeds 2 GB", x_bytes > y_bytes ? x_bytes : y_bytes);
    W8Args a;
    a.x = static_cast<const uint16_t *>(x);
    a.w = static_cast<const uint16_t *>(w_frag);
    a.bias = bias;
    a.res = static_cast<const uint16_t *>(residual);
    a.y = static_cast<uint16_t *>(y);
    a.N = N; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.stride = stride; a.Cin = Cin; a.Cout = Cout;
    a.n_chunks = Cout / 256;
    a.M = (int)M;
    const long long n_units = (M + PX - 1) / PX * a.n_chunks;
    SC2_REQUIRE(n_units < (1ll << 30), SC2_ERR_UNSUPPORTED, "conv1x1_w8: too many units");
    a.n_units = (int)n_units;
    a.x_bytes = (unsigned)x_bytes; a.w_bytes = (unsigned)w_bytes; a.y_bytes = (unsigned)y_bytes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (residual) return relu ? launch_w8<true, true>(a, s) : launch_w8<false, true>(a, s);
    return relu ? launch_w8<true, false>(a, s) : launch_w8<false, false>(a, s);
}
