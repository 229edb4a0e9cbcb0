// Segmentation training loss: cross entropy of the bilinearly resized class logits against a target map, forward and backward,
// from the LOW-resolution logits (sc2_seg_ce_forward / sc2_seg_ce_backward).  The reference's training step forms
// `interpolate(logits, size)` for both heads, `cross_entropy` reads the two [N,C,H,W] tensors again, and the backward writes and
// reads gradients of the same size; here neither the resized logits nor their gradient exist.  include/sc2_bottleneck.h states the
// contract; tests/ref_seg_loss.py restates it in float64.  The resized value is seg_common.h's, shared with sc2_seg_predict.
// Plain kernels: every index checked against its array before use, no atomics of any kind, no workgroup waits for another.  Both
// results are reproducible bit for bit: the loss sum is a fixed tree over per-workgroup float64 partials (a second, one-workgroup
// launch), and every gradient element is one thread's f32 sum over its footprint in row-major order (a gather).
#include "seg_common.h"

namespace {

constexpr int CE_TW = 32, CE_TH = 8;         // forward: output pixels of one tile, one per lane
constexpr int CE_THREADS = CE_TW * CE_TH;
constexpr int CE_WAVES = CE_THREADS / 64;
constexpr int CE_MAX_WGS = 1024;             // forward grid cap = number of partials (the same on every device)
constexpr int BW_TX = 8, BW_TY = 4;          // backward: source pixels of one tile
constexpr int BW_PX = BW_TX + 2, BW_PY = BW_TY + 2;      // ... with the one-pixel halo its footprints read
constexpr int BW_THREADS = 256;

struct CeArgs {
    const void *logits;
    const long long *targets;
    float *pixel_loss, *lse;
    double *part_sum;              // [grid]
    long long *part_cnt, *part_bad;
    long long sN, sC, sH, sW;      // element strides of the logits
    long long n_tiles, ignore_index;
    int N, C, h, w, H, W, tiles_x, tiles_y;
};

inline long long ce_tiles(int N, int H, int W) {
    return (long long)N * ((W + CE_TW - 1) / CE_TW) * ((H + CE_TH - 1) / CE_TH);
}
inline int ce_grid(int N, int H, int W) {
    const long long t = ce_tiles(N, H, W);
    return (int)(t < CE_MAX_WGS ? t : CE_MAX_WGS);
}

// sum over the workgroup in a fixed tree: lanes of a wave by halving distances, then the waves in index order.  -> valid in thread 0
template <typename T>
__device__ __forceinline__ T ce_block_sum(T v, T *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    T total = lds[0];
    for (int i = 1; i < CE_WAVES; ++i) total += lds[i];
    __syncthreads();
    return total;
}

// One output pixel per lane over 32 x 8 tiles; a workgroup walks tiles blockIdx.x, + gridDim.x, ... and leaves ONE partial.
// Per pixel one online pass over the classes: running maximum m, running sum s of expf(v - m) (rescaled when the maximum moves),
// and the target's value picked up on the way; nothing is indexed by a runtime class.
template <bool BF16, bool VEC>
__global__ __launch_bounds__(CE_THREADS) void seg_ce_forward_kernel(const CeArgs a) {
    __shared__ double red_d[CE_WAVES];
    __shared__ long long red_i[CE_WAVES];
    const int tid = threadIdx.x;
    const int lx_in_tile = tid % CE_TW, ly_in_tile = tid / CE_TW;
    double sum = 0.0;
    long long cnt = 0, bad = 0;
    for (long long tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long per_image = (long long)a.tiles_x * a.tiles_y;
        const int n = (int)(tile / per_image);
        const int r = (int)(tile - (long long)n * per_image);
        const int ty = r / a.tiles_x, tx = r - ty * a.tiles_x;
        const int oy = ty * CE_TH + ly_in_tile, ox = tx * CE_TW + lx_in_tile;
        if (oy >= a.H || ox >= a.W) continue;      // (no barrier inside the tile loop)
        const long long at = ((long long)n * a.H + oy) * a.W + ox;
        const long long t = a.targets[at];
        const bool valid = t >= 0 && t < a.C && t != a.ignore_index;
        if (!valid && t != a.ignore_index) ++bad;
        float loss = 0.0f, lse = 0.0f;
        if (valid || a.lse) {
            int y0, y1, x0, x1;
            float ly, lx;
            seg_axis(oy, a.h, a.H, y0, y1, ly);
            seg_axis(ox, a.w, a.W, x0, x1, lx);
            const float hy = 1.0f - ly, hx = 1.0f - lx;
            const long long img = (long long)n * a.sN;
            const long long p00 = img + y0 * a.sH + x0 * a.sW, p01 = img + y0 * a.sH + x1 * a.sW;
            const long long p10 = img + y1 * a.sH + x0 * a.sW, p11 = img + y1 * a.sH + x1 * a.sW;
            float m = 0.0f, s = 1.0f, vt = 0.0f;
            const int tc = valid ? (int)t : -1;
            seg_for_each_class<BF16, VEC>(a.logits, a.C, a.sC, p00, p01, p10, p11, hy, hx, ly, lx, [&](int c, float val) {
                if (c == 0) {
                    m = val;
                } else if (val > m) {
                    s = s * expf(m - val) + 1.0f;
                    m = val;
                } else {
                    s += expf(val - m);
                }
                if (c == tc) vt = val;
            });
            lse = m + logf(s);
            if (valid) {
                loss = lse - vt;
                sum += (double)loss;
                ++cnt;
            }
        }
        if (a.pixel_loss) a.pixel_loss[at] = loss;
        if (a.lse) a.lse[at] = lse;
    }
    const double wg_sum = ce_block_sum(sum, red_d);
    const long long wg_cnt = ce_block_sum(cnt, red_i);
    const long long wg_bad = ce_block_sum(bad, red_i);
    if (tid == 0) {
        a.part_sum[blockIdx.x] = wg_sum;
        a.part_cnt[blockIdx.x] = wg_cnt;
        a.part_bad[blockIdx.x] = wg_bad;
    }
}

// One workgroup: thread t adds the partials t * per .. t * per + per - 1 in index order, then the fixed tree of ce_block_sum.
__global__ __launch_bounds__(CE_THREADS) void seg_ce_finish_kernel(const double *part_sum, const long long *part_cnt,
                                                                   const long long *part_bad, int n_part, double *sums) {
    __shared__ double red_d[CE_WAVES];
    __shared__ long long red_i[CE_WAVES];
    const int per = (n_part + CE_THREADS - 1) / CE_THREADS;
    const int lo = threadIdx.x * per;
    const int hi = min(lo + per, n_part);
    double sum = 0.0;
    long long cnt = 0, bad = 0;
    for (int i = lo; i < hi; ++i) {
        sum += part_sum[i];
        cnt += part_cnt[i];
        bad += part_bad[i];
    }
    const double total = ce_block_sum(sum, red_d);
    const long long total_cnt = ce_block_sum(cnt, red_i);
    const long long total_bad = ce_block_sum(bad, red_i);
    if (threadIdx.x == 0) {
        sums[0] = total;
        reinterpret_cast<long long *>(sums)[1] = total_cnt;
        reinterpret_cast<long long *>(sums)[2] = total_bad;
    }
}

struct CeBwArgs {
    const void *logits;
    const long long *targets;
    const float *lse, *grad_out;
    const long long *sums;         // [1]: the number of valid pixels
    void *dx;
    long long sN, sC, sH, sW;      // element strides of the logits
    long long dN, dC, dH, dW;      // ... and of dx
    long long ignore_index;
    int N, C, h, w, H, W, tiles_x, tiles_y, reduction;
};

// One workgroup per (image, 8 x 4 tile of source pixels): the tile's logits and a one-pixel halo in LDS as f32 [pixel][class].
// One thread per (source pixel, class), the class running fastest over the lanes (the lanes of a wave share a pixel's target and lse
// loads and read consecutive LDS words).  The output pixels whose footprint holds source pixel (i, j) are rows
// seg_axis_first(i-1) .. seg_axis_first(i+1) - 1 times the same range of columns: the thread walks them row by row, left to right,
// re-forms v[p,c] from the LDS tile and adds w_p(i,j) * (expf(v - lse_p) - [c == t_p]) in f32.
template <bool BF16>
__global__ __launch_bounds__(BW_THREADS) void seg_ce_backward_kernel(const CeBwArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];      // [BW_PY * BW_PX][C]
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int i_base = ty * BW_TY - 1, j_base = tx * BW_TX - 1;       // source coordinates of the LDS tile's corner
    for (int e = tid; e < BW_PY * BW_PX * a.C; e += BW_THREADS) {
        const int pix = e / a.C, c = e - pix * a.C;
        const int i = i_base + pix / BW_PX, j = j_base + pix % BW_PX;
        float v = 0.0f;
        if (i >= 0 && i < a.h && j >= 0 && j < a.w)
            v = SegVec<BF16>::load1(a.logits, (long long)n * a.sN + c * a.sC + i * a.sH + j * a.sW);
        tile[e] = v;
    }
    __syncthreads();
    const long long count = a.sums[1];
    float g = 0.0f;
    if (a.reduction == 0)
        g = count > 0 ? a.grad_out[0] / (float)count : 0.0f;
    else if (a.reduction == 1)
        g = a.grad_out[0];
    else
        g = 1.0f;
    const bool live = a.reduction != 0 || count > 0;
    for (int e = tid; e < BW_TY * BW_TX * a.C; e += BW_THREADS) {
        const int pix = e / a.C, c = e - pix * a.C;
        const int li = pix / BW_TX, lj = pix - li * BW_TX;
        const int i = ty * BW_TY + li, j = tx * BW_TX + lj;
        if (i >= a.h || j >= a.w) continue;      // (no barrier below)
        float acc = 0.0f;
        if (live) {
            const int d_lo = seg_axis_first(i - 1, a.h, a.H), d_hi = seg_axis_first(i + 1, a.h, a.H);
            const int e_lo = seg_axis_first(j - 1, a.w, a.W), e_hi = seg_axis_first(j + 1, a.w, a.W);
            SegAxisWalk wy_walk(d_lo, a.h, a.H);
            for (int d = d_lo; d < d_hi; ++d, wy_walk.step()) {
                int y0, y1;
                float ly;
                wy_walk.get(y0, y1, ly);
                const float hy = 1.0f - ly;
                const float wy = (y0 == i ? hy : 0.0f) + (y1 == i ? ly : 0.0f);
                // rows of the LDS tile: y0 and y1 lie in i-1 .. i+1 by the choice of [d_lo, d_hi)
                const float *row0 = tile + (size_t)((y0 - i_base) * BW_PX) * a.C + c;
                const float *row1 = tile + (size_t)((y1 - i_base) * BW_PX) * a.C + c;
                const long long row_at = ((long long)n * a.H + d) * a.W;
                SegAxisWalk wx_walk(e_lo, a.w, a.W);
                for (int ex = e_lo; ex < e_hi; ++ex, wx_walk.step()) {
                    const long long t = a.targets[row_at + ex];
                    if (!(t >= 0 && t < a.C && t != a.ignore_index)) continue;
                    int x0, x1;
                    float lx;
                    wx_walk.get(x0, x1, lx);
                    const float hx = 1.0f - lx;
                    const float wx = (x0 == j ? hx : 0.0f) + (x1 == j ? lx : 0.0f);
                    const int o0 = (x0 - j_base) * a.C, o1 = (x1 - j_base) * a.C;
                    const float v = seg_value(hy, hx, ly, lx, row0[o0], row0[o1], row1[o0], row1[o1]);
                    float term = expf(v - a.lse[row_at + ex]) - (c == (int)t ? 1.0f : 0.0f);
                    float wgt = wy * wx;
                    if (a.reduction == 2) wgt *= a.grad_out[row_at + ex];
                    acc += wgt * term;
                }
            }
        }
        const float out = g * acc;
        const long long at = (long long)n * a.dN + c * a.dC + i * a.dH + j * a.dW;
        if (BF16)
            static_cast<uint16_t *>(a.dx)[at] = f32_to_bf16_bits(out);
        else
            static_cast<float *>(a.dx)[at] = out;
    }
}

int ce_check_logits(const char *who, const void *logits, int is_bf16, int N, int C, int h, int w, long long stride_n, long long stride_c,
                    long long stride_h, long long stride_w, int H, int W) {
    SC2_REQUIRE(N > 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0, SC2_ERR_INVALID_ARG, "%s: bad dims N=%d C=%d %dx%d -> %dx%d", who,
                N, C, h, w, H, W);
    SC2_REQUIRE(C <= SC2_SEG_MAX_CLASSES, SC2_ERR_UNSUPPORTED, "%s: %d classes (at most %d)", who, C, SC2_SEG_MAX_CLASSES);
    SC2_REQUIRE(h <= SEG_MAX_DIM && w <= SEG_MAX_DIM && H <= SEG_MAX_DIM && W <= SEG_MAX_DIM, SC2_ERR_UNSUPPORTED,
                "%s: %dx%d -> %dx%d (at most %d per side)", who, h, w, H, W, SEG_MAX_DIM);
    SC2_REQUIRE(N <= 65535, SC2_ERR_UNSUPPORTED, "%s: %d images in one call (at most 65535)", who, N);
    SC2_REQUIRE(logits, SC2_ERR_INVALID_ARG, "%s: null logits", who);
    SC2_REQUIRE(stride_n >= 0 && stride_c >= 0 && stride_h >= 0 && stride_w >= 0, SC2_ERR_INVALID_ARG, "%s: negative stride", who);
    SC2_REQUIRE((reinterpret_cast<uintptr_t>(logits) & (is_bf16 ? 1u : 3u)) == 0, SC2_ERR_INVALID_ARG, "%s: misaligned logits", who);
    return SC2_OK;
}

}  // namespace

extern "C" long long sc2_seg_ce_ws_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || H > SEG_MAX_DIM || W > SEG_MAX_DIM || N > 65535) return 0;
    return 3ll * 8 * ce_grid(N, H, W);
}

extern "C" int sc2_seg_ce_forward(const void *logits, int is_bf16, int N, int C, int h, int w, long long stride_n, long long stride_c,
                                  long long stride_h, long long stride_w, int c_readable, int H, int W, const long long *targets,
                                  long long ignore_index, float *pixel_loss, float *lse, void *sums, void *ws, void *stream) {
    const int rc = ce_check_logits("seg_ce_forward", logits, is_bf16, N, C, h, w, stride_n, stride_c, stride_h, stride_w, H, W);
    if (rc != SC2_OK) return rc;
    SC2_REQUIRE(targets && sums && ws, SC2_ERR_INVALID_ARG, "seg_ce_forward: null targets, sums or workspace");
    SC2_REQUIRE((reinterpret_cast<uintptr_t>(targets) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(pixel_loss) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(lse) & 3u) == 0,
                SC2_ERR_INVALID_ARG, "seg_ce_forward: misaligned pointer");
    const int grid = ce_grid(N, H, W);
    CeArgs a;
    a.logits = logits;
    a.targets = targets;
    a.pixel_loss = pixel_loss;
    a.lse = lse;
    a.part_sum = static_cast<double *>(ws);
    a.part_cnt = reinterpret_cast<long long *>(a.part_sum + grid);
    a.part_bad = a.part_cnt + grid;
    a.sN = stride_n; a.sC = stride_c; a.sH = stride_h; a.sW = stride_w;
    a.ignore_index = ignore_index;
    a.N = N; a.C = C; a.h = h; a.w = w; a.H = H; a.W = W;
    a.tiles_x = (W + CE_TW - 1) / CE_TW;
    a.tiles_y = (H + CE_TH - 1) / CE_TH;
    a.n_tiles = ce_tiles(N, H, W);
    const bool vec = seg_vec_ok(logits, is_bf16, C, stride_n, stride_c, stride_h, stride_w, c_readable);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (is_bf16) {
        if (vec) hipLaunchKernelGGL((seg_ce_forward_kernel<true, true>), dim3(grid), dim3(CE_THREADS), 0, s, a);
        else hipLaunchKernelGGL((seg_ce_forward_kernel<true, false>), dim3(grid), dim3(CE_THREADS), 0, s, a);
    } else {
        if (vec) hipLaunchKernelGGL((seg_ce_forward_kernel<false, true>), dim3(grid), dim3(CE_THREADS), 0, s, a);
        else hipLaunchKernelGGL((seg_ce_forward_kernel<false, false>), dim3(grid), dim3(CE_THREADS), 0, s, a);
    }
    SC2_CHECK_LAUNCH();
    hipLaunchKernelGGL(seg_ce_finish_kernel, dim3(1), dim3(CE_THREADS), 0, s, a.part_sum, a.part_cnt, a.part_bad, grid,
                       static_cast<double *>(sums));
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}

extern "C" int sc2_seg_ce_backward(const void *logits, int is_bf16, int N, int C, int h, int w, long long stride_n, long long stride_c,
                                   long long stride_h, long long stride_w, int c_readable, int H, int W, const long long *targets,
                                   long long ignore_index, const float *lse, const void *sums, const float *grad_out, int reduction,
                                   void *dx, long long dx_stride_n, long long dx_stride_c, long long dx_stride_h, long long dx_stride_w,
                                   void *stream) {
    const int rc = ce_check_logits("seg_ce_backward", logits, is_bf16, N, C, h, w, stride_n, stride_c, stride_h, stride_w, H, W);
    if (rc != SC2_OK) return rc;
    (void)c_readable;      // the tile is staged element by element: nothing behind class C-1 is read
    SC2_REQUIRE(targets && lse && sums && grad_out && dx, SC2_ERR_INVALID_ARG, "seg_ce_backward: null pointer");
    SC2_REQUIRE(reduction >= SC2_SEG_CE_MEAN && reduction <= SC2_SEG_CE_NONE, SC2_ERR_INVALID_ARG, "seg_ce_backward: reduction %d",
                reduction);
    SC2_REQUIRE(dx_stride_n >= 0 && dx_stride_c >= 0 && dx_stride_h >= 0 && dx_stride_w >= 0, SC2_ERR_INVALID_ARG,
                "seg_ce_backward: negative dx stride");
    SC2_REQUIRE((reinterpret_cast<uintptr_t>(targets) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(lse) & 3u) == 0 && (reinterpret_cast<uintptr_t>(grad_out) & 3u) == 0 &&
                    (reinterpret_cast<uintptr_t>(dx) & (is_bf16 ? 1u : 3u)) == 0,
                SC2_ERR_INVALID_ARG, "seg_ce_backward: misaligned pointer");
    CeBwArgs a;
    a.logits = logits;
    a.targets = targets;
    a.lse = lse;
    a.grad_out = grad_out;
    a.sums = static_cast<const long long *>(sums);
    a.dx = dx;
    a.sN = stride_n; a.sC = stride_c; a.sH = stride_h; a.sW = stride_w;
    a.dN = dx_stride_n; a.dC = dx_stride_c; a.dH = dx_stride_h; a.dW = dx_stride_w;
    a.ignore_index = ignore_index;
    a.N = N; a.C = C; a.h = h; a.w = w; a.H = H; a.W = W;
    a.tiles_x = (w + BW_TX - 1) / BW_TX;
    a.tiles_y = (h + BW_TY - 1) / BW_TY;
    a.reduction = reduction;
    const long long tiles = (long long)a.tiles_x * a.tiles_y;
    SC2_REQUIRE(tiles <= 0x7FFFFFFFll, SC2_ERR_UNSUPPORTED, "seg_ce_backward: %lld source tiles per image", tiles);
    const size_t lds = (size_t)BW_PY * BW_PX * C * sizeof(float);      // 15 KB at 64 classes
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (is_bf16)
        hipLaunchKernelGGL((seg_ce_backward_kernel<true>), dim3((unsigned)tiles, (unsigned)N), dim3(BW_THREADS), lds, s, a);
    else
        hipLaunchKernelGGL((seg_ce_backward_kernel<false>), dim3((unsigned)tiles, (unsigned)N), dim3(BW_THREADS), lds, s, a);
    SC2_CHECK_LAUNCH();
    return SC2_OK;
}
