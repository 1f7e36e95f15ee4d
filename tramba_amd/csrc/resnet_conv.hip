// Convolutions of the ResNet-50 encoder (Tramba-R, 16-bit inference; encoders.set_library_convolutions).
//
// (a) tramba_conv_affine_cl: a bottleneck convolution (1x1 or 3x3, stride 1 or 2, pad = ksize / 2, no bias) with its
//     eval-mode batch norm, shortcut and ReLU in one launch (resnet_encoder.py:62-110):
//         y[t, co] = act( scale[co] * sum_k X[t, k] W[co, k] + shift[co] + residual[t, co] )
//     As an implicit GEMM: row = output pixel t = (b, oi, oj), column k = (di ksize + dj) Cin + c.  Cin % 64 == 0, so a 64-deep
//     K step lies inside one tap (di, dj): it is 64 contiguous channels of ONE input pixel, and the operand fragments of
//     mfma_f32_16x16x32 are 16-byte reads of x and of the K-major weight as they lie -- no im2col, no NCHW copy (as in
//     patch_conv.hip).  A tap outside the map contributes zero by predicate: its address is never formed.
//     Two forms, chosen on the host (ca_plan):
//       tall / shallow (layer1: M = 9216, K = 64 .. 576): a workgroup owns NW x 16 rows x 64 columns, wave w owns row block w
//         and runs the full K loop;
//       short / deep (layer3: M = 576, K = 1024 .. 2304): a workgroup owns 16 rows x 64 columns and its NW waves split K by
//         64-deep steps (wave w takes steps w, w + NW, ...); the partial tiles are added through LDS in wave order 0 .. NW-1.
//     Both pass their f32 tile through LDS so that a lane stores 8 contiguous channels; scale, shift, residual and ReLU are
//     applied in f32 and the result is rounded once.  No atomics, no hand-off between workgroups, K never split across
//     workgroups: the result is a fixed function of the inputs.
// (b) tramba_stem7_affine_relu_pool: conv1 (7x7 / 2 / pad 3, 3 -> 64) + bn1 + ReLU + max_pool2d(3, 2, 1)
//     (resnet_encoder.py:81-110).  Modelled on patch_embed_ln / stem.hip: the image is read in NCHW as it lies, the filter
//     sits in LDS tap-major, beside the image patch of the workgroup's 4 x 8 pooled pixels.  A group of 16 lanes computes the
//     3 x 5 block of convolution outputs under the pool windows of two neighbouring pooled pixels in registers (the one-pixel
//     halo included) and pools from there: the half-resolution map is never written, neither to memory nor to LDS.
// (c) tramba_conv_dgrad_cl / tramba_conv_wgrad_cl: the backward of (a)'s convolution in 16-bit training
//     (encoders.set_library_training), where (a) itself runs with NULL scale / shift and no ReLU as the raw convolution.
//     Input gradient: gx[b, p, q, c] = sum over taps (di, dj) and co of gy[b, oi, oj, co] w[co, di, dj, c] with
//     oi stride = p + pad - di (likewise oj): the implicit GEMM of (a) with rows = INPUT pixels, the reduction over (tap, co)
//     and the transposed weight copy (Cin, k, k, Cout) as the K-major operand -- the same tile arithmetic, both forms, with
//     the tap predicate "p + pad - di is a multiple of the stride and the quotient lies in the output map" in place of the
//     padding test.  No zero-inserted map; a pixel that no output reaches keeps its zero accumulator: every gx is written.
//     Weight gradient: gw[co, (di, dj, c)] = sum_t gy[t, co] x[pixel(t, di, dj), c], the reduction over tokens, the slow
//     index of both operands: the structure of patch_conv_wgrad_kernel (patch_conv_bwd.hip) -- [32 t][64 k] of x, read in
//     place with padding taps staged as zeros and never addressed, and [32 t][64 co] of gy go through LDS and all fragments are
//     transposed reads.  Grid (K / 64, Cout / 64, S): the token steps are dealt in runs to S workgroups, run z writes f32
//     slab z of the caller's workspace and the caller adds the slabs in index order.  No column matrix, no atomics.
#include "common.h"

namespace tramba {

typedef __attribute__((ext_vector_type(8))) short ca_frag8;
typedef __attribute__((ext_vector_type(4))) float ca_acc4;

template <typename T> struct CaMfma;
template <> struct CaMfma<__hip_bfloat16> {
    static __device__ __forceinline__ ca_acc4 run(ca_frag8 a, ca_frag8 b, ca_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
    }
};
template <> struct CaMfma<__half> {
    static __device__ __forceinline__ ca_acc4 run(ca_frag8 a, ca_frag8 b, ca_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) _Float16 h8;
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    }
};

constexpr int kCaRows = 16, kCaCols = 64, kCaSub = kCaCols / 16;

// the operand fragments of one 64-deep K step: two 32-deep MFMA steps, one x fragment and kCaSub weight fragments each
struct CaStep {
    ca_frag8 a[2];
    ca_frag8 b[2][kCaSub];
};

// this lane's output pixel: its image (with the lane's 8-channel offset inside a 32-deep fragment) and the map
// coordinates of tap (0, 0), which are negative where the tap lies in the padding
template <typename T> struct CaRow {
    const T *img;
    int iy0, ix0;
};

// step t covers k = 64 t .. 64 t + 63 = tap (di, dj), channels 64 rem .. 64 rem + 63 (t is wave-uniform)
template <typename T>
__device__ __forceinline__ void ca_load(CaStep &f, const CaRow<T> &r, const T *__restrict__ wcol, int t, int cs, int ks, int H,
                                        int W, int Cin, unsigned wsub, const bool (&colok)[kCaSub])
{
    const int tap = t / cs, rem = t - tap * cs;
    const int di = tap / ks, dj = tap - di * ks;
    const int iy = r.iy0 + di, ix = r.ix0 + dj;
    const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;           // a padding tap reads nothing and adds nothing
    const unsigned xoff = in ? ((unsigned)iy * W + ix) * Cin + 64u * rem : 0u;
    const ca_frag8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f.a[h] = in ? *reinterpret_cast<const ca_frag8 *>(r.img + xoff + 32 * h) : z;
#pragma unroll
        for (int j = 0; j < kCaSub; ++j)
            f.b[h][j] = colok[j] ? *reinterpret_cast<const ca_frag8 *>(wcol + (size_t)j * wsub + 64u * t + 32 * h) : z;
    }
}

// 8 columns of one output row: affine, shortcut, ReLU in f32, one rounding.  Cout % 8 == 0: a group of 8 columns is inside or
// outside as a whole.
template <typename T>
__device__ __forceinline__ void ca_finish(float (&o)[8], long row, int col, int M, int Cout, const float *__restrict__ scale,
                                          const float *__restrict__ shift, const T *__restrict__ residual, T *__restrict__ y,
                                          int relu)
{
    if (row >= M || col >= Cout) return;
    float res[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) res[v] = 0.f;
    if (residual) load_pack<T, 8>(residual + (size_t)row * Cout + col, res);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const float sc = scale ? scale[col + v] : 1.f, sh = shift ? shift[col + v] : 0.f;
        float r = fmaf(sc, o[v], sh) + res[v];
        o[v] = relu ? fmaxf(r, 0.f) : r;
    }
    store_pack<T, 8>(y + (size_t)row * Cout + col, o);
}

// grid (row tiles, column blocks of 64).  SPLITK: a row tile is 16 rows and the NW waves split K; otherwise it is NW x 16
// rows, one 16-row block per wave.
template <typename T, int NW, bool SPLITK>
__global__ __launch_bounds__(NW * 64) void conv_affine_kernel(const T *__restrict__ x, const T *__restrict__ w,
                                                             const float *__restrict__ scale,
                                                             const float *__restrict__ shift,
                                                             const T *__restrict__ residual, T *__restrict__ y, int M, int H,
                                                             int W, int Cin, int Cout, int ks, int stride, int Ho, int Wo,
                                                             int relu)
{
    __shared__ __attribute__((aligned(16))) float red[NW][kCaRows][kCaCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.y * kCaCols;
    const long m0 = (long)blockIdx.x * (SPLITK ? kCaRows : kCaRows * NW) + (SPLITK ? 0 : kCaRows * wave);
    const int cs = Cin >> 6, K = ks * ks * Cin, steps = K >> 6, pad = ks >> 1;

    // this lane's operand rows: output pixel (clamped: rows past M compute a copy of the last pixel and are never stored)
    // and weight column (columns past Cout read nothing)
    long tok = m0 + (lane & 15);
    tok = tok < M ? tok : M - 1;
    const int oj = (int)(tok % Wo);
    const long t2 = tok / Wo;
    const int oi = (int)(t2 % Ho), b = (int)(t2 / Ho);
    CaRow<T> row;
    row.img = x + (size_t)b * H * W * Cin + 8 * (lane >> 4);
    row.iy0 = oi * stride - pad;
    row.ix0 = oj * stride - pad;
    bool colok[kCaSub];
#pragma unroll
    for (int s = 0; s < kCaSub; ++s) colok[s] = n0 + 16 * s + (lane & 15) < Cout;
    const T *wcol = w + (size_t)(n0 + (lane & 15)) * K + 8 * (lane >> 4);
    const unsigned wsub = 16u * (unsigned)K;

    ca_acc4 acc[kCaSub];
#pragma unroll
    for (int s = 0; s < kCaSub; ++s) acc[s] = ca_acc4{0.f, 0.f, 0.f, 0.f};

    constexpr int kInc = SPLITK ? NW : 1;
    int t = SPLITK ? wave : 0;
    CaStep cur, nxt;
    if (t < steps) ca_load(cur, row, wcol, t, cs, ks, H, W, Cin, wsub, colok);
    nxt = cur;
    while (t < steps) {
        const int tn = t + kInc;
        if (tn < steps) ca_load(nxt, row, wcol, tn, cs, ks, H, W, Cin, wsub, colok);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < kCaSub; ++s) acc[s] = CaMfma<T>::run(cur.a[h], cur.b[h][s], acc[s]);
        cur = nxt;
        t = tn;
    }

    // tiles -> LDS (accumulator element q of lane l is row 4 (l >> 4) + q, column l & 15 of its 16 x 16 block)
#pragma unroll
    for (int s = 0; s < kCaSub; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave][4 * (lane >> 4) + q][16 * s + (lane & 15)] = acc[s][q];
    __syncthreads();

    if (SPLITK) {
        // 128 threads add the NW partials in wave order, 8 columns of one row each
        if (threadIdx.x < kCaRows * (kCaCols / 8)) {
            const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 8;
            float o[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) o[v] = red[0][r][c0 + v];
#pragma unroll 4
            for (int p = 1; p < NW; ++p)
#pragma unroll
                for (int v = 0; v < 8; ++v) o[v] += red[p][r][c0 + v];
            ca_finish<T>(o, m0 + r, n0 + c0, M, Cout, scale, shift, residual, y, relu);
        }
    } else {
        // each wave finishes its own 16 x 64 tile: two passes of 64 lanes x 8 columns
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = lane + 64 * it, r = idx >> 3, c0 = (idx & 7) * 8;
            float o[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) o[v] = red[wave][r][c0 + v];
            ca_finish<T>(o, m0 + r, n0 + c0, M, Cout, scale, shift, residual, y, relu);
        }
    }
}

// which form takes (M, K): waves per workgroup and whether they split K
struct CaPlan {
    int nw;
    bool splitk;
};
static CaPlan ca_plan(long m, int cout, int k)
{
    const int steps = k / 64;
    // short / deep: too few rows to fill the chip with row blocks, and K deep enough to give every wave two steps
    if (m < 4096 && steps >= 8) return {steps >= 32 ? 16 : steps >= 16 ? 8 : 4, true};
    // tall / shallow: 64 rows per workgroup, 32 where that alone leaves compute units idle
    const long wgs = ((m + 63) / 64) * ((cout + kCaCols - 1) / kCaCols);
    return {wgs < 256 ? 2 : 4, false};
}

template <typename T>
static void launch_conv_affine(CaPlan p, const void *x, const void *w, const float *scale, const float *shift, const void *res,
                               void *y, long m, int h, int wd, int cin, int cout, int ks, int stride, int ho, int wo, int relu,
                               hipStream_t s)
{
    const long rows = p.splitk ? kCaRows : (long)kCaRows * p.nw;
    dim3 grid((unsigned)((m + rows - 1) / rows), (unsigned)((cout + kCaCols - 1) / kCaCols));
#define TRAMBA_CA_LAUNCH(NW, SPLIT)                                                                                         \
    hipLaunchKernelGGL((conv_affine_kernel<T, NW, SPLIT>), grid, dim3(NW * 64), 0, s, (const T *)x, (const T *)w, scale, shift, \
                       (const T *)res, (T *)y, (int)m, h, wd, cin, cout, ks, stride, ho, wo, relu)
    if (p.splitk) {
        if (p.nw == 16) TRAMBA_CA_LAUNCH(16, true);
        else if (p.nw == 8) TRAMBA_CA_LAUNCH(8, true);
        else TRAMBA_CA_LAUNCH(4, true);
    } else {
        if (p.nw == 4) TRAMBA_CA_LAUNCH(4, false);
        else TRAMBA_CA_LAUNCH(2, false);
    }
#undef TRAMBA_CA_LAUNCH
}

// ---- backward of the bottleneck convolutions ----
// step t of the input gradient covers reduction indices 64 t .. 64 t + 63 = tap (di, dj), output channels 64 rem .. + 63.
// r.iy0 / r.ix0 hold p + pad / q + pad of this lane's input pixel, r.img the image of gy.
template <typename T>
__device__ __forceinline__ void cd_load(CaStep &f, const CaRow<T> &r, const T *__restrict__ wcol, int t, int cs, int ks,
                                        int stride, int Ho, int Wo, int Cout, unsigned wsub, const bool (&colok)[kCaSub])
{
    const int tap = t / cs, rem = t - tap * cs;
    const int di = tap / ks, dj = tap - di * ks;
    const int ny = r.iy0 - di, nx = r.ix0 - dj;                       // = oi stride, oj stride
    bool in = ny >= 0 && nx >= 0;
    int oy = ny, ox = nx;
    if (stride == 2) {
        in = in && ((ny | nx) & 1) == 0;                              // the tap reaches this pixel from no output otherwise
        oy = ny >> 1;
        ox = nx >> 1;
    }
    in = in && oy < Ho && ox < Wo;
    const unsigned goff = in ? ((unsigned)oy * Wo + ox) * Cout + 64u * rem : 0u;
    const ca_frag8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f.a[h] = in ? *reinterpret_cast<const ca_frag8 *>(r.img + goff + 32 * h) : z;
#pragma unroll
        for (int j = 0; j < kCaSub; ++j)
            f.b[h][j] = colok[j] ? *reinterpret_cast<const ca_frag8 *>(wcol + (size_t)j * wsub + 64u * t + 32 * h) : z;
    }
}

// grid and forms as conv_affine_kernel; M = B H W input pixels, columns = Cin, K = ks ks Cout; wt (Cin, ks, ks, Cout)
template <typename T, int NW, bool SPLITK>
__global__ __launch_bounds__(NW * 64) void conv_dgrad_kernel(const T *__restrict__ gy, const T *__restrict__ wt,
                                                            T *__restrict__ gx, int M, int H, int W, int Cin, int Cout, int ks,
                                                            int stride, int Ho, int Wo)
{
    __shared__ __attribute__((aligned(16))) float red[NW][kCaRows][kCaCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.y * kCaCols;
    const long m0 = (long)blockIdx.x * (SPLITK ? kCaRows : kCaRows * NW) + (SPLITK ? 0 : kCaRows * wave);
    const int cs = Cout >> 6, K = ks * ks * Cout, steps = K >> 6, pad = ks >> 1;

    long pix = m0 + (lane & 15);
    pix = pix < M ? pix : M - 1;
    const int q = (int)(pix % W);
    const long t2 = pix / W;
    const int p = (int)(t2 % H), b = (int)(t2 / H);
    CaRow<T> row;
    row.img = gy + (size_t)b * Ho * Wo * Cout + 8 * (lane >> 4);
    row.iy0 = p + pad;
    row.ix0 = q + pad;
    bool colok[kCaSub];
#pragma unroll
    for (int s = 0; s < kCaSub; ++s) colok[s] = n0 + 16 * s + (lane & 15) < Cin;
    const T *wcol = wt + (size_t)(n0 + (lane & 15)) * K + 8 * (lane >> 4);
    const unsigned wsub = 16u * (unsigned)K;

    ca_acc4 acc[kCaSub];
#pragma unroll
    for (int s = 0; s < kCaSub; ++s) acc[s] = ca_acc4{0.f, 0.f, 0.f, 0.f};

    constexpr int kInc = SPLITK ? NW : 1;
    int t = SPLITK ? wave : 0;
    CaStep cur, nxt;
    if (t < steps) cd_load(cur, row, wcol, t, cs, ks, stride, Ho, Wo, Cout, wsub, colok);
    nxt = cur;
    while (t < steps) {
        const int tn = t + kInc;
        if (tn < steps) cd_load(nxt, row, wcol, tn, cs, ks, stride, Ho, Wo, Cout, wsub, colok);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < kCaSub; ++s) acc[s] = CaMfma<T>::run(cur.a[h], cur.b[h][s], acc[s]);
        cur = nxt;
        t = tn;
    }

#pragma unroll
    for (int s = 0; s < kCaSub; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave][4 * (lane >> 4) + e][16 * s + (lane & 15)] = acc[s][e];
    __syncthreads();

    if (SPLITK) {
        if (threadIdx.x < kCaRows * (kCaCols / 8)) {
            const int r = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 8;
            float o[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) o[v] = red[0][r][c0 + v];
#pragma unroll 4
            for (int pp = 1; pp < NW; ++pp)
#pragma unroll
                for (int v = 0; v < 8; ++v) o[v] += red[pp][r][c0 + v];
            ca_finish<T>(o, m0 + r, n0 + c0, M, Cin, nullptr, nullptr, nullptr, gx, 0);
        }
    } else {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = lane + 64 * it, r = idx >> 3, c0 = (idx & 7) * 8;
            float o[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) o[v] = red[wave][r][c0 + v];
            ca_finish<T>(o, m0 + r, n0 + c0, M, Cin, nullptr, nullptr, nullptr, gx, 0);
        }
    }
}

template <typename T>
static void launch_conv_dgrad(CaPlan p, const void *gy, const void *wt, void *gx, long m, int h, int wd, int cin, int cout,
                              int ks, int stride, int ho, int wo, hipStream_t s)
{
    const long rows = p.splitk ? kCaRows : (long)kCaRows * p.nw;
    dim3 grid((unsigned)((m + rows - 1) / rows), (unsigned)((cin + kCaCols - 1) / kCaCols));
#define TRAMBA_CD_LAUNCH(NW, SPLIT)                                                                                         \
    hipLaunchKernelGGL((conv_dgrad_kernel<T, NW, SPLIT>), grid, dim3(NW * 64), 0, s, (const T *)gy, (const T *)wt, (T *)gx,  \
                       (int)m, h, wd, cin, cout, ks, stride, ho, wo)
    if (p.splitk) {
        if (p.nw == 16) TRAMBA_CD_LAUNCH(16, true);
        else if (p.nw == 8) TRAMBA_CD_LAUNCH(8, true);
        else TRAMBA_CD_LAUNCH(4, true);
    } else {
        if (p.nw == 4) TRAMBA_CD_LAUNCH(4, false);
        else TRAMBA_CD_LAUNCH(2, false);
    }
#undef TRAMBA_CD_LAUNCH
}

// weight gradient: staged 16-bit tiles of 32 tokens x 64 columns, rows kCwStride bytes apart (a multiple of 16)
typedef __attribute__((ext_vector_type(4))) short cw_frag4;
constexpr int kCwDepth = 32, kCwCols = 64, kCwWaves = 4, kCwStride = kCwCols * 2 + 16;
constexpr int kCwTarget = 512, kCwMaxSplit = 64;

// Elements [row0 + j][col0 + (lane & 15)], j = 0..7, of a staged tile: two transposed reads (patch_conv_bwd.hip, pb_tr_pair).
// Every address is 8-byte aligned and the callers' control flow is wave-uniform, so EXEC is all ones.
__device__ __forceinline__ ca_frag8 cw_tr_pair(const unsigned char *img, int row0, int col0, int li)
{
    typedef __attribute__((address_space(3))) cw_frag4 lds_frag4;
    const unsigned char *p = img + (row0 + (li >> 2)) * kCwStride + (col0 + 4 * (li & 3)) * 2;
    const cw_frag4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag4 *)p);
    const cw_frag4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag4 *)(p + 4 * kCwStride));
    return ca_frag8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// grid (K / 64, ceil(Cout / 64), S), 256 threads: wave w owns co 16 w .. 16 w + 15 of the block's 64; the block's 64 k lie in
// ONE tap (Cin % 64 == 0)
template <typename T>
__global__ __launch_bounds__(kCwWaves * 64) void conv_wgrad_kernel(const T *__restrict__ gy, const T *__restrict__ x,
                                                                  float *__restrict__ part, int M, int H, int W, int Cin,
                                                                  int Cout, int ks, int stride, int Ho, int Wo,
                                                                  int steps_per_split)
{
    __shared__ __attribute__((aligned(16))) unsigned char x_lds[kCwDepth * kCwStride];
    __shared__ __attribute__((aligned(16))) unsigned char g_lds[kCwDepth * kCwStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = ks * ks * Cin, pad = ks >> 1;
    const int n0 = blockIdx.x * kCwCols, c0 = blockIdx.y * kCwCols;
    const int tap = n0 / Cin, rem = n0 - tap * Cin;
    const int di = tap / ks, dj = tap - di * ks;
    const int steps_all = (M + kCwDepth - 1) / kCwDepth;
    const int s0 = blockIdx.z * steps_per_split;
    const int s1 = s0 + steps_per_split < steps_all ? s0 + steps_per_split : steps_all;
    // staging: thread = (token row of the step, 16-byte chunk) of both tiles
    const int srow = threadIdx.x >> 3, sch = 8 * (threadIdx.x & 7);
    const bool co_ok = c0 + sch < Cout;             // Cout % 8 == 0
    const ca_frag8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    ca_acc4 acc[kCwCols / 16];
#pragma unroll
    for (int s = 0; s < kCwCols / 16; ++s) acc[s] = ca_acc4{0.f, 0.f, 0.f, 0.f};

    ca_frag8 xv, gv;
    auto load = [&](int s) {
        const int t = s * kCwDepth + srow;          // tokens past M and padding taps add zeros; their address is never formed
        xv = zero;
        gv = zero;
        if (t < M) {
            const int oj = t % Wo, t2 = t / Wo, oi = t2 % Ho, b = t2 / Ho;
            const int iy = oi * stride - pad + di, ix = oj * stride - pad + dj;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W)
                xv = *reinterpret_cast<const ca_frag8 *>(x + (((size_t)b * H + iy) * W + ix) * Cin + rem + sch);
            if (co_ok) gv = *reinterpret_cast<const ca_frag8 *>(gy + (size_t)t * Cout + c0 + sch);
        }
    };
    load(s0);
    for (int s = s0; s < s1; ++s) {
        __syncthreads();
        *reinterpret_cast<ca_frag8 *>(x_lds + srow * kCwStride + sch * 2) = xv;
        *reinterpret_cast<ca_frag8 *>(g_lds + srow * kCwStride + sch * 2) = gv;
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
        const ca_frag8 bf = cw_tr_pair(g_lds, 8 * (lane >> 4), 16 * wave, lane & 15);
#pragma unroll
        for (int c = 0; c < kCwCols / 16; ++c) {
            const ca_frag8 af = cw_tr_pair(x_lds, 8 * (lane >> 4), 16 * c, lane & 15);
            acc[c] = CaMfma<T>::run(af, bf, acc[c]);
        }
    }

    // accumulator element e of lane l: k = n0 + 16 c + 4 (l >> 4) + e, co = c0 + 16 wave + (l & 15)
    float *slab = part + (size_t)blockIdx.z * ((size_t)Cout * K);
    const int co = c0 + 16 * wave + (lane & 15);
    if (co < Cout) {
#pragma unroll
        for (int c = 0; c < kCwCols / 16; ++c)
            *reinterpret_cast<float4 *>(slab + (size_t)co * K + n0 + 16 * c + 4 * (lane >> 4)) =
                make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    }
}

// steps of 32 tokens per split, and the number of splits: functions of the shape alone
static void cw_plan(long m, int k, int cout, int &steps_per_split, int &nsplit)
{
    const long steps = (m + kCwDepth - 1) / kCwDepth;
    const long base = (long)(k / kCwCols) * ((cout + kCwCols - 1) / kCwCols);
    long want = kCwTarget / (base > 0 ? base : 1);
    want = want < 1 ? 1 : (want > kCwMaxSplit ? kCwMaxSplit : want);
    want = want > steps ? steps : want;
    steps_per_split = (int)((steps + want - 1) / want);
    nsplit = (int)((steps + steps_per_split - 1) / steps_per_split);
}

// the shape checks shared by the two backward entries and the sizing entries
static bool cb_shape_ok(int batch, int hin, int win, int cin, int cout, int ksize, int stride)
{
    if (!((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2) && batch > 0 && cin > 0 && cout > 0 && hin > 0 && win > 0))
        return false;
    const int pad = ksize / 2;
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1;
    return (double)batch * hin * win * cin * 2.0 < 2147483648.0 && (double)batch * ho * wo * cout * 2.0 < 2147483648.0 &&
           (double)cout * ksize * ksize * cin * 4.0 < 2147483648.0 && (double)batch * hin * win < 2147483647.0;
}

// ---- stem: 7x7 / 2 convolution + affine + ReLU + 3x3 / 2 max pool ----
// A workgroup owns a tile of 4 x 8 pooled pixels.  16 lanes share a PAIR of pooled pixels (ph, 2 q) and (ph, 2 q + 1), 4 output
// channels each, and keep the 3 x 5 block of convolution outputs under the two pool windows in registers (60 f32
// accumulators): the windows of neighbouring pairs overlap by one row / column, so 15 outputs are computed for 8 distinct
// ones, and in exchange the half-resolution map is staged nowhere and one 16-byte filter read from LDS feeds 60 FMAs.
// The 23 x 39 image patch under the tile's 9 x 17 convolution outputs is copied to LDS once, padding as zeros, so the
// inner loop reads 16-byte pieces of LDS with no range check.
constexpr int kStTaps = 3 * 7 * 7, kStCout = 64, kStLanes = 16;
constexpr int kStTileH = 4, kStTileQ = 4;                                  // pooled rows x pooled PAIRS per workgroup
constexpr int kStPatchH = 2 * (2 * kStTileH) + 7, kStPatchW = 2 * (4 * kStTileQ) + 7, kStPatchRow = 40;   // 23 x 39, rows padded
constexpr int kStWRow = kStCout + 8;     // LDS row of one tap, padded: the tap-major fill is 8-way, not 64-way, bank-conflicted
static_assert(kStTileH * kStTileQ * kStLanes == 256 && kStPatchW <= kStPatchRow, "stem tile");

// grid (pooled tiles along W, along H, batch)
template <typename TI, typename T>
__global__ __launch_bounds__(256) void stem7_pool_kernel(const TI *__restrict__ img, const float *__restrict__ w,
                                                        const float *__restrict__ scale, const float *__restrict__ shift,
                                                        T *__restrict__ y, int H, int W, int Hc, int Wc, int Hp, int Wp)
{
    __shared__ __attribute__((aligned(16))) float wl[kStTaps][kStWRow];                     // [ci*49 + ky*7 + kx][cout]
    __shared__ __attribute__((aligned(16))) float patch[3][kStPatchH][kStPatchRow];
    const int b = blockIdx.z, ph0 = blockIdx.y * kStTileH, q0 = blockIdx.x * kStTileQ;
    // the tile's convolution rows start at 2 ph0 - 1 and its columns at 4 q0 - 1 (-1: pool padding); tap (0, 0) of the
    // first of them reads the image at (hy0, wx0)
    const int cr0 = 2 * ph0 - 1, cc0 = 4 * q0 - 1;
    const int hy0 = 2 * cr0 - 3, wx0 = 2 * cc0 - 3;
    for (int t = threadIdx.x; t < kStTaps * kStCout; t += blockDim.x) {
        const int co = t / kStTaps, tap = t % kStTaps;  // reference layout (64, 3, 7, 7)
        wl[tap][co] = w[t];
    }
    for (int t = threadIdx.x; t < 3 * kStPatchH * kStPatchRow; t += blockDim.x) {
        const int c = t % kStPatchRow, r = (t / kStPatchRow) % kStPatchH, ci = t / (kStPatchRow * kStPatchH);
        const int hy = hy0 + r, wx = wx0 + c;
        float v = 0.f;                                   // a padding tap reads nothing and adds nothing
        if (c < kStPatchW && hy >= 0 && hy < H && wx >= 0 && wx < W) v = Cvt<TI>::to_f(img[(((long)b * 3 + ci) * H + hy) * W + wx]);
        patch[ci][r][c] = v;
    }
    __syncthreads();
    const int part = threadIdx.x & (kStLanes - 1), grp = threadIdx.x / kStLanes;
    const int lph = grp / kStTileQ, lq = grp % kStTileQ;

    float acc[3][5][4];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[j][i][c] = 0.f;

    // (one filter row per trip, NOT unrolled: see stem.hip)
#pragma unroll 1
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
            // filter row ky of convolution row 2 lph + j reads patch row 2 (2 lph + j) + ky, columns 8 lq .. 8 lq + 14
            float v[3][16];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float4 *pr = reinterpret_cast<const float4 *>(&patch[ci][2 * (2 * lph + j) + ky][8 * lq]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 f = pr[q];
                    v[j][4 * q + 0] = f.x;
                    v[j][4 * q + 1] = f.y;
                    v[j][4 * q + 2] = f.z;
                    v[j][4 * q + 3] = f.w;
                }
            }
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float4 w0 = *reinterpret_cast<const float4 *>(&wl[(ci * 7 + ky) * 7 + kx][part * 4]);
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        const float x = v[j][kx + 2 * i];
                        acc[j][i][0] = fmaf(x, w0.x, acc[j][i][0]);
                        acc[j][i][1] = fmaf(x, w0.y, acc[j][i][1]);
                        acc[j][i][2] = fmaf(x, w0.z, acc[j][i][2]);
                        acc[j][i][3] = fmaf(x, w0.w, acc[j][i][3]);
                    }
            }
        }
    const int ph = ph0 + lph;
    if (ph >= Hp) return;

    float sc[4], sh[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        sc[c] = scale[part * 4 + c];
        sh[c] = shift[part * 4 + c];
    }
    // The pool's padding positions are excluded from the max.  The max starts from 0, which is the ReLU: after it every value
    // is >= 0 and the window's centre is always inside the map, so excluding the padding equals zero padding.
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int pw = 2 * (q0 + lq) + p;
        if (pw >= Wp) continue;
        float o[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int cr = cr0 + 2 * lph + j;
            if (cr < 0 || cr >= Hc) continue;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int cc = cc0 + 4 * lq + 2 * p + d;
                if (cc < 0 || cc >= Wc) continue;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = fmaxf(o[c], fmaf(sc[c], acc[j][2 * p + d][c], sh[c]));
            }
        }
        store_pack<T, 4>(y + (((size_t)b * Hp + ph) * Wp + pw) * kStCout + part * 4, o);
    }
}

}  // namespace tramba

using namespace tramba;

extern "C" int tramba_conv_affine_cl(const void *x, const void *w, const float *scale, const float *shift,
                                     const void *residual, void *y, int batch, int hin, int win, int cin, int cout, int ksize,
                                     int stride, int relu, int dtype, void *stream)
{
    TRAMBA_CHECK(x && w && y, "conv_affine_cl: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "conv_affine_cl: bf16/f16 only");
    TRAMBA_CHECK(ksize == 1 || ksize == 3, "conv_affine_cl: ksize = %d must be 1 or 3", ksize);
    TRAMBA_CHECK(stride == 1 || stride == 2, "conv_affine_cl: stride = %d must be 1 or 2", stride);
    TRAMBA_CHECK(batch > 0 && cin > 0 && cout > 0 && hin > 0 && win > 0, "conv_affine_cl: empty shape");
    TRAMBA_CHECK(cin % 64 == 0, "conv_affine_cl: Cin=%d must be a multiple of 64", cin);
    TRAMBA_CHECK(cout % 8 == 0, "conv_affine_cl: Cout=%d must be a multiple of 8", cout);
    TRAMBA_CHECK((double)batch * hin * win * cin * 2.0 < 2147483648.0, "conv_affine_cl: input map beyond 32-bit byte offsets");
    const int pad = ksize / 2;
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1;
    const long m = (long)batch * ho * wo;
    const int k = ksize * ksize * cin;
    TRAMBA_CHECK(m < 2147483647L && (cout + kCaCols - 1) / kCaCols <= 65535 && (double)cout * k * 2.0 < 2147483648.0,
                 "conv_affine_cl: too many output pixels or weights");
    TRAMBA_CHECK(aligned16(x) && aligned16(w) && aligned16(y) && aligned16(residual),
                 "conv_affine_cl: tensors must be 16-byte aligned");
    const CaPlan plan = ca_plan(m, cout, k);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16)
        launch_conv_affine<__hip_bfloat16>(plan, x, w, scale, shift, residual, y, m, hin, win, cin, cout, ksize, stride, ho, wo,
                                           relu != 0, s);
    else
        launch_conv_affine<__half>(plan, x, w, scale, shift, residual, y, m, hin, win, cin, cout, ksize, stride, ho, wo,
                                   relu != 0, s);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

#define TRAMBA_CB_SHAPE_CHECKS(NAME)                                                                                     \
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, NAME ": bf16/f16 only");                                   \
    TRAMBA_CHECK(ksize == 1 || ksize == 3, NAME ": ksize = %d must be 1 or 3", ksize);                                   \
    TRAMBA_CHECK(stride == 1 || stride == 2, NAME ": stride = %d must be 1 or 2", stride);                               \
    TRAMBA_CHECK(batch > 0 && cin > 0 && cout > 0 && hin > 0 && win > 0, NAME ": empty shape");                          \
    TRAMBA_CHECK(cin % 8 == 0 && cout % 8 == 0, NAME ": Cin=%d and Cout=%d must be multiples of 8", cin, cout);          \
    TRAMBA_CHECK(cb_shape_ok(batch, hin, win, cin, cout, ksize, stride), NAME ": map, gradient or weight beyond 32-bit byte offsets")

extern "C" int tramba_conv_dgrad_cl(const void *gy, const void *wt, void *gx, int batch, int hin, int win, int cin, int cout,
                                    int ksize, int stride, int dtype, void *stream)
{
    TRAMBA_CHECK(gy && wt && gx, "conv_dgrad_cl: null tensor");
    TRAMBA_CB_SHAPE_CHECKS("conv_dgrad_cl");
    const bool gemm = ksize == 1 && stride == 1;       // gx = gy wt^T, a plain (M, Cout) x (Cout, Cin) product
    TRAMBA_CHECK(gemm || cout % 64 == 0, "conv_dgrad_cl: Cout=%d must be a multiple of 64 (except 1x1 / stride 1)", cout);
    TRAMBA_CHECK((cin + kCaCols - 1) / kCaCols <= 65535, "conv_dgrad_cl: too many channels");
    TRAMBA_CHECK(aligned16(gy) && aligned16(wt) && aligned16(gx), "conv_dgrad_cl: tensors must be 16-byte aligned");
    const long m = (long)batch * hin * win;
    if (gemm) return tramba_linear_cl(gy, wt, nullptr, nullptr, gx, m, cin, cout, TRAMBA_ACT_NONE, dtype, dtype, stream);
    const int pad = ksize / 2;
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1;
    const CaPlan plan = ca_plan(m, cin, ksize * ksize * cout);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16)
        launch_conv_dgrad<__hip_bfloat16>(plan, gy, wt, gx, m, hin, win, cin, cout, ksize, stride, ho, wo, s);
    else
        launch_conv_dgrad<__half>(plan, gy, wt, gx, m, hin, win, cin, cout, ksize, stride, ho, wo, s);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_conv_wgrad_split(int batch, int hin, int win, int cin, int cout, int ksize, int stride)
{
    if (!cb_shape_ok(batch, hin, win, cin, cout, ksize, stride) || cin % 64 != 0 || cout % 8 != 0) return 0;
    const int pad = ksize / 2;
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1;
    int sps, nsplit;
    cw_plan((long)batch * ho * wo, ksize * ksize * cin, cout, sps, nsplit);
    return nsplit;
}

extern "C" size_t tramba_conv_wgrad_work(int batch, int hin, int win, int cin, int cout, int ksize, int stride)
{
    const int nsplit = tramba_conv_wgrad_split(batch, hin, win, cin, cout, ksize, stride);
    return (size_t)nsplit * ((size_t)cout * ksize * ksize * cin) * sizeof(float);
}

extern "C" int tramba_conv_wgrad_cl(const void *gy, const void *x, float *work, size_t work_bytes, int batch, int hin, int win,
                                    int cin, int cout, int ksize, int stride, int dtype, void *stream)
{
    TRAMBA_CHECK(gy && x, "conv_wgrad_cl: null tensor");
    TRAMBA_CB_SHAPE_CHECKS("conv_wgrad_cl");
    TRAMBA_CHECK(cin % 64 == 0, "conv_wgrad_cl: Cin=%d must be a multiple of 64", cin);
    TRAMBA_CHECK((cout + kCwCols - 1) / kCwCols <= 65535, "conv_wgrad_cl: too many channels");
    TRAMBA_CHECK(aligned16(gy) && aligned16(x) && aligned16(work), "conv_wgrad_cl: tensors must be 16-byte aligned");
    const size_t need = tramba_conv_wgrad_work(batch, hin, win, cin, cout, ksize, stride);
    TRAMBA_CHECK(work && work_bytes >= need, "conv_wgrad_cl: workspace of %zu bytes needed, %zu given", need,
                 work ? work_bytes : (size_t)0);
    const int pad = ksize / 2;
    const int ho = (hin + 2 * pad - ksize) / stride + 1, wo = (win + 2 * pad - ksize) / stride + 1;
    const long m = (long)batch * ho * wo;
    const int k = ksize * ksize * cin;
    int sps, nsplit;
    cw_plan(m, k, cout, sps, nsplit);
    dim3 grid((unsigned)(k / kCwCols), (unsigned)((cout + kCwCols - 1) / kCwCols), (unsigned)nsplit);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16)
        hipLaunchKernelGGL((conv_wgrad_kernel<__hip_bfloat16>), grid, dim3(kCwWaves * 64), 0, s, (const __hip_bfloat16 *)gy,
                           (const __hip_bfloat16 *)x, work, (int)m, hin, win, cin, cout, ksize, stride, ho, wo, sps);
    else
        hipLaunchKernelGGL((conv_wgrad_kernel<__half>), grid, dim3(kCwWaves * 64), 0, s, (const __half *)gy, (const __half *)x,
                           work, (int)m, hin, win, cin, cout, ksize, stride, ho, wo, sps);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_stem7_affine_relu_pool(const void *img, const float *w, const float *scale, const float *shift, void *y,
                                             int batch, int h, int wd, int img_dtype, int dtype, void *stream)
{
    TRAMBA_CHECK(img && w && scale && shift && y, "stem7_affine_relu_pool: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "stem7_affine_relu_pool: bf16/f16 output only");
    TRAMBA_CHECK(img_dtype == TRAMBA_F32 || img_dtype == dtype,
                 "stem7_affine_relu_pool: image must be f32 or the activation dtype");
    TRAMBA_CHECK(batch > 0 && h > 0 && wd > 0, "stem7_affine_relu_pool: empty shape");
    const int hc = (h - 1) / 2 + 1, wc = (wd - 1) / 2 + 1;
    const int hp = (hc - 1) / 2 + 1, wp = (wc - 1) / 2 + 1;
    TRAMBA_CHECK(batch <= 65535 && (hp + kStTileH - 1) / kStTileH <= 65535 && (double)batch * 3.0 * h * wd < 9.0e18,
                 "stem7_affine_relu_pool: too many pixels");
    TRAMBA_CHECK(aligned16(y), "stem7_affine_relu_pool: output must be 16-byte aligned");
    dim3 grid((unsigned)((wp + 2 * kStTileQ - 1) / (2 * kStTileQ)), (unsigned)((hp + kStTileH - 1) / kStTileH), (unsigned)batch);
    dim3 block(256);
    hipStream_t s = (hipStream_t)stream;
#define TRAMBA_ST_LAUNCH(TI, T)                                                                                             \
    hipLaunchKernelGGL((stem7_pool_kernel<TI, T>), grid, block, 0, s, (const TI *)img, w, scale, shift, (T *)y, h, wd, hc, wc, \
                       hp, wp)
    if (dtype == TRAMBA_BF16) {
        if (img_dtype == TRAMBA_F32) TRAMBA_ST_LAUNCH(float, __hip_bfloat16);
        else TRAMBA_ST_LAUNCH(__hip_bfloat16, __hip_bfloat16);
    } else {
        if (img_dtype == TRAMBA_F32) TRAMBA_ST_LAUNCH(float, __half);
        else TRAMBA_ST_LAUNCH(__half, __half);
    }
#undef TRAMBA_ST_LAUNCH
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
