// Backward of tramba_patch_conv_cl, the kernel = stride = r convolution on a channels-last map -- PVT's spatial-reduction
// `sr` (pvtv2_encoder.py:76-78,103-106) in 16-bit training (encoders.set_library_training).
//
// With row = output token t = (b, i, j) and column k = (di r + dj) Cin + c the forward is y = X W^T + bias, where row t of
// X is the r kernel rows of the token's patch: r runs of r Cin contiguous elements of x.  X is never built.
//
// (a) tramba_patch_conv_dgrad_cl: gX = gy W, (M, Cout) x (Cout, K), written through the patch addressing into x's layout.
//     The reduction index co is the SLOW index of the K-major weight, so the weight is the transposed operand: a wave
//     stages a [32 co][64 k] tile of W as it lies (16-byte loads of rows, 16-byte LDS stores) and takes its MFMA B
//     fragments out of it with ds_read_b64_tr_b16.  The A fragments are 16-byte reads of gy rows.  A workgroup owns 16
//     tokens x 256 columns: 4 waves, 64 columns each, every wave walks Cout in 32-deep steps with the next step's global
//     loads in flight over the MFMAs.  The f32 tile goes through LDS once, so that a lane stores 8 consecutive channels
//     (16 bytes) of one token: 64 columns never cross a kernel row (r Cin % 64 == 0).
//     A second launch writes zeros to the rows >= r Ho and columns >= r Wo of a map whose side is no multiple of r (it is
//     skipped when there are none), so every element of gx is written exactly once.
// (b) tramba_patch_conv_wgrad_cl: gW^T = X^T gy, reduction over tokens, which is the slow index of BOTH operands: a
//     workgroup stages [32 t][64 k] of X (read in place through the patch addressing) and [32 t][64 co] of gy, and all
//     fragments are transposed reads.  Accumulators hold k along rows, so a lane stores 4 consecutive k of one co as one
//     16-byte f32 store into the K-major gradient.  Grid (K / 64, Cout / 64, S): the token steps are dealt to S workgroups
//     in runs; split z writes the f32 slab z of the caller's workspace, [Cout K floats of gW | Cout floats of gb], and the
//     caller adds the slabs in index order (tramba_slab_sum).  S is a function of the shape alone.  gb = column sums of gy:
//     the workgroups of k block 0 add the staged rows in token order.
//
// Ragged token tiles are padded, not masked: a row past M recomputes the last token (dgrad) or is staged as zeros
// (wgrad), every lane runs every transposed read, and nothing of such a row is stored.  No atomics: the summation order
// is fixed by the shape.  No allocation, no synchronisation: capturable.
#include "common.h"

namespace tramba {

typedef __attribute__((ext_vector_type(8))) short pb_frag8;
typedef __attribute__((ext_vector_type(4))) short pb_frag4;
typedef __attribute__((ext_vector_type(4))) float pb_acc4;

template <typename T> struct PbMfma;
template <> struct PbMfma<__hip_bfloat16> {
    static __device__ __forceinline__ pb_acc4 run(pb_frag8 a, pb_frag8 b, pb_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
    }
};
template <> struct PbMfma<__half> {
    static __device__ __forceinline__ pb_acc4 run(pb_frag8 a, pb_frag8 b, pb_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) _Float16 h8;
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    }
};

constexpr int kPbRows = 16;                 // dgrad: tokens per workgroup
constexpr int kPbCols = 64;                 // columns (k, or co) per tile
constexpr int kPbDepth = 32;                // reduction depth per step = one MFMA
constexpr int kPbWaves = 4;
constexpr int kPbStride = kPbCols * 2 + 16; // bytes per row of a staged 16-bit tile (a multiple of 16)
constexpr int kPbOutLd = kPbCols + 4;       // floats per row of the dgrad output tile
constexpr int kPbWgradTarget = 512;         // workgroups the token split of the weight gradient aims at
constexpr int kPbWgradMaxSplit = 16;

// Elements [row0 + j][col0 + (lane & 15)], j = 0..7, of a 16-bit LDS tile with kPbStride bytes per row: two transposed
// reads.  Lane 4 q + p of a 16-lane group supplies the address of row q, columns 4 p .. 4 p + 3, of the group's 4 x 16
// block and receives the block's column (lane & 15).  Every address is 8-byte aligned (the stride is a multiple of 16,
// col0 of 16) and the callers' control flow is wave-uniform, so EXEC is all ones.
__device__ __forceinline__ pb_frag8 pb_tr_pair(const unsigned char *img, int row0, int col0, int li)
{
    typedef __attribute__((address_space(3))) pb_frag4 lds_frag4;
    const unsigned char *p = img + (row0 + (li >> 2)) * kPbStride + (col0 + 4 * (li & 3)) * 2;
    const pb_frag4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag4 *)p);
    const pb_frag4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_frag4 *)(p + 4 * kPbStride));
    return pb_frag8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// first element of token t's patch in x
__device__ __forceinline__ size_t pb_patch(int t, int H, int W, int Cin, int r, int Ho, int Wo)
{
    const int j = t % Wo, t2 = t / Wo, i = t2 % Ho, b = t2 / Ho;
    return (((size_t)b * H + (size_t)i * r) * W + (size_t)j * r) * Cin;
}

// ------------------------------------------------------------------------------------------------ input gradient
// grid (ceil(K / 256), token tiles of 16), 256 threads.
template <typename T>
__global__ __launch_bounds__(kPbWaves * 64) void patch_conv_dgrad_kernel(const T *__restrict__ gy, const T *__restrict__ w,
                                                                        T *__restrict__ gx, int M, int H, int W, int Cin,
                                                                        int Cout, int r, int Ho, int Wo)
{
    __shared__ __attribute__((aligned(16))) unsigned char w_lds[kPbWaves][kPbDepth * kPbStride];
    __shared__ __attribute__((aligned(16))) float o_lds[kPbWaves][kPbRows][kPbOutLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rc = r * Cin, K = r * rc;
    const int m0 = blockIdx.y * kPbRows;
    // this wave's 64 columns; a wave past K recomputes the last block and stores nothing
    int n0 = (blockIdx.x * kPbWaves + wave) * kPbCols;
    const bool wave_ok = n0 < K;
    n0 = wave_ok ? n0 : K - kPbCols;

    int tok = m0 + (lane & 15);
    tok = tok < M ? tok : M - 1;
    const T *grow = gy + (size_t)tok * Cout + 8 * (lane >> 4);
    // staging: 8 lanes move one 128-byte row of the tile, 8 rows per pass
    const int srow = lane >> 3, scol = 8 * (lane & 7);
    const T *wsrc = w + (size_t)srow * K + n0 + scol;
    unsigned char *wdst = w_lds[wave] + srow * kPbStride + scol * 2;
    const pb_frag8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    pb_acc4 acc[kPbCols / 16];
#pragma unroll
    for (int s = 0; s < kPbCols / 16; ++s) acc[s] = pb_acc4{0.f, 0.f, 0.f, 0.f};

    const int steps = (Cout + kPbDepth - 1) / kPbDepth;
    pb_frag8 a, wv[kPbDepth / 8];
    auto load = [&](int co0) {
        // Cout % 8 == 0: a group of 8 reduction indices lies inside or outside as a whole, and outside both operands are zero
        a = co0 + 8 * (lane >> 4) < Cout ? *reinterpret_cast<const pb_frag8 *>(grow + co0) : zero;
#pragma unroll
        for (int p = 0; p < kPbDepth / 8; ++p) {
            const int co = co0 + 8 * p + srow;
            wv[p] = co < Cout ? *reinterpret_cast<const pb_frag8 *>(wsrc + (size_t)(co0 + 8 * p) * K) : zero;
        }
    };
    load(0);
    for (int s = 0; s < steps; ++s) {
        __syncthreads();                      // the previous step's transposed reads are done
#pragma unroll
        for (int p = 0; p < kPbDepth / 8; ++p) *reinterpret_cast<pb_frag8 *>(wdst + 8 * p * kPbStride) = wv[p];
        const pb_frag8 acur = a;
        __syncthreads();
        if (s + 1 < steps) load((s + 1) * kPbDepth);
#pragma unroll
        for (int c = 0; c < kPbCols / 16; ++c) {
            const pb_frag8 b = pb_tr_pair(w_lds[wave], 8 * (lane >> 4), 16 * c, lane & 15);
            acc[c] = PbMfma<T>::run(acur, b, acc[c]);
        }
    }

    // accumulator element q of lane l is token row 4 (l >> 4) + q, column l & 15 of its 16 x 16 block
#pragma unroll
    for (int c = 0; c < kPbCols / 16; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) o_lds[wave][4 * (lane >> 4) + q][16 * c + (lane & 15)] = acc[c][q];
    __syncthreads();
    // 64 columns of one token lie in one kernel row di: rem .. rem + 63 of its r Cin contiguous elements
    const int di = n0 / rc, rem = n0 % rc;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int u = lane + 64 * it, row = u >> 3, c8 = 8 * (u & 7);
        const int t = m0 + row;
        if (wave_ok && t < M) {
            float o[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) o[v] = o_lds[wave][row][c8 + v];
            store_pack<T, 8>(gx + pb_patch(t, H, W, Cin, r, Ho, Wo) + (size_t)di * W * Cin + rem + c8, o);
        }
    }
}

// zeros for the pixels no patch covers: rows >= r Ho (whole width), then columns >= r Wo of the rows above
template <typename T>
__global__ __launch_bounds__(256) void patch_conv_dgrad_tail_kernel(T *__restrict__ gx, long units, int H, int W, int Cin, int rHo,
                                                                   int rWo)
{
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const int c8n = Cin / 8;
    const long tailpix = (long)H * W - (long)rHo * rWo, nbottom = (long)(H - rHo) * W;
    const int c8 = (int)(u % c8n);
    const long p = u / c8n, b = p / tailpix;
    long q = p % tailpix;
    long y, x;
    if (q < nbottom) {
        y = rHo + q / W;
        x = q % W;
    } else {
        q -= nbottom;
        y = q / (W - rWo);
        x = rWo + q % (W - rWo);
    }
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    store_pack<T, 8>(gx + ((b * H + y) * W + x) * Cin + 8 * c8, z);
}

// ------------------------------------------------------------------------------------------------ weight gradient
// grid (K / 64, ceil(Cout / 64), S), 256 threads: wave w owns co 16 w .. 16 w + 15 of the block's 64.
template <typename T>
__global__ __launch_bounds__(kPbWaves * 64) void patch_conv_wgrad_kernel(const T *__restrict__ gy, const T *__restrict__ x,
                                                                        float *__restrict__ part, int M, int H, int W, int Cin,
                                                                        int Cout, int r, int Ho, int Wo, int steps_per_split,
                                                                        int want_bias)
{
    __shared__ __attribute__((aligned(16))) unsigned char x_lds[kPbDepth * kPbStride];
    __shared__ __attribute__((aligned(16))) unsigned char g_lds[kPbDepth * kPbStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rc = r * Cin, K = r * rc;
    const int n0 = blockIdx.x * kPbCols, c0 = blockIdx.y * kPbCols;
    const int di = n0 / rc, rem = n0 % rc;          // the block's 64 k lie in kernel row di of every token
    const int steps_all = (M + kPbDepth - 1) / kPbDepth;
    const int s0 = blockIdx.z * steps_per_split;
    const int s1 = s0 + steps_per_split < steps_all ? s0 + steps_per_split : steps_all;
    // staging: thread = (token row of the step, 16-byte chunk) of both tiles
    const int srow = threadIdx.x >> 3, sch = 8 * (threadIdx.x & 7);
    const bool co_ok = c0 + sch < Cout;             // Cout % 8 == 0
    const size_t xrow = (size_t)di * W * Cin + rem + sch;
    const pb_frag8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool bias_wave = blockIdx.x == 0 && wave == 0;       // owns the gb part of the slab (zeros without want_bias)

    pb_acc4 acc[kPbCols / 16];
#pragma unroll
    for (int s = 0; s < kPbCols / 16; ++s) acc[s] = pb_acc4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;

    pb_frag8 xv, gv;
    auto load = [&](int s) {
        const int t = s * kPbDepth + srow;          // tokens past M add zeros
        xv = t < M ? *reinterpret_cast<const pb_frag8 *>(x + pb_patch(t, H, W, Cin, r, Ho, Wo) + xrow) : zero;
        gv = t < M && co_ok ? *reinterpret_cast<const pb_frag8 *>(gy + (size_t)t * Cout + c0 + sch) : zero;
    };
    load(s0);
    for (int s = s0; s < s1; ++s) {
        __syncthreads();
        *reinterpret_cast<pb_frag8 *>(x_lds + srow * kPbStride + sch * 2) = xv;
        *reinterpret_cast<pb_frag8 *>(g_lds + srow * kPbStride + sch * 2) = gv;
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
        const pb_frag8 b = pb_tr_pair(g_lds, 8 * (lane >> 4), 16 * wave, lane & 15);
#pragma unroll
        for (int c = 0; c < kPbCols / 16; ++c) {
            const pb_frag8 a = pb_tr_pair(x_lds, 8 * (lane >> 4), 16 * c, lane & 15);
            acc[c] = PbMfma<T>::run(a, b, acc[c]);
        }
        if (bias_wave && want_bias) {               // wave-uniform: column lane of the staged gy rows, in token order
#pragma unroll 8
            for (int t = 0; t < kPbDepth; ++t)
                bsum += Cvt<T>::to_f(*reinterpret_cast<const T *>(g_lds + t * kPbStride + lane * 2));
        }
    }

    // accumulator element q of lane l: k = n0 + 16 c + 4 (l >> 4) + q, co = c0 + 16 wave + (l & 15)
    float *slab = part + (size_t)blockIdx.z * ((size_t)Cout * K + Cout);
    const int co = c0 + 16 * wave + (lane & 15);
    if (co < Cout) {
#pragma unroll
        for (int c = 0; c < kPbCols / 16; ++c)
            *reinterpret_cast<float4 *>(slab + (size_t)co * K + n0 + 16 * c + 4 * (lane >> 4)) =
                make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
    }
    if (bias_wave && c0 + lane < Cout) slab[(size_t)Cout * K + c0 + lane] = bsum;
}

// steps of 32 tokens per split, and the number of splits: functions of the shape alone
static void pb_wgrad_plan(long m, int k, int cout, int &steps_per_split, int &nsplit)
{
    const long steps = (m + kPbDepth - 1) / kPbDepth;
    const long base = (long)(k / kPbCols) * ((cout + kPbCols - 1) / kPbCols);
    long want = kPbWgradTarget / (base > 0 ? base : 1);
    want = want < 1 ? 1 : (want > kPbWgradMaxSplit ? kPbWgradMaxSplit : want);
    want = want > steps ? steps : want;
    steps_per_split = (int)((steps + want - 1) / want);
    nsplit = (int)((steps + steps_per_split - 1) / steps_per_split);
}

static bool pb_layer_ok(int batch, int hin, int win, int cin, int cout, int r)
{
    return r >= 2 && r <= 8 && batch > 0 && cin > 0 && cout > 0 && hin >= r && win >= r && cin % 64 == 0 && cout % 8 == 0;
}

// map, gy and the f32 weight gradient below 2^31 bytes
static bool pb_bytes_ok(int batch, int hin, int win, int cin, int cout, int r)
{
    const long m = (long)batch * (hin / r) * (win / r);
    return (double)batch * hin * win * cin * 2.0 < 2147483648.0 && (double)cout * r * r * cin * 4.0 < 2147483648.0 &&
           (double)m * cout * 2.0 < 2147483648.0;
}

// token tiles of 16 are grid.y of the input gradient
static bool pb_grid_ok(int batch, int hin, int win, int r)
{
    const long m = (long)batch * (hin / r) * (win / r);
    return (m + kPbRows - 1) / kPbRows <= 65535;
}

static bool pb_shape_ok(int batch, int hin, int win, int cin, int cout, int r)
{
    return pb_layer_ok(batch, hin, win, cin, cout, r) && pb_bytes_ok(batch, hin, win, cin, cout, r) &&
           pb_grid_ok(batch, hin, win, r);
}

}  // namespace tramba

using namespace tramba;

#define TRAMBA_PB_SHAPE_CHECKS(NAME)                                                                                     \
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, NAME ": dtype must be bf16 or f16");                       \
    TRAMBA_CHECK(r >= 2 && r <= 8, NAME ": kernel = stride = %d must be in 2..8", r);                                    \
    TRAMBA_CHECK(batch > 0 && cin > 0 && cout > 0 && hin >= r && win >= r, NAME ": empty shape");                        \
    TRAMBA_CHECK(cin % 64 == 0, NAME ": Cin=%d must be a multiple of 64", cin);                                          \
    TRAMBA_CHECK(cout % 8 == 0, NAME ": Cout=%d must be a multiple of 8", cout);                                         \
    TRAMBA_CHECK(pb_bytes_ok(batch, hin, win, cin, cout, r), NAME ": map, gradient or weight beyond 32-bit byte offsets");  \
    TRAMBA_CHECK(pb_grid_ok(batch, hin, win, r), NAME ": too many output tokens (more than 65535 tiles of 16)")

extern "C" int tramba_patch_conv_dgrad_cl(const void *gy, const void *w, void *gx, int batch, int hin, int win, int cin,
                                          int cout, int r, int dtype, void *stream)
{
    TRAMBA_CHECK(gy && w && gx, "patch_conv_dgrad_cl: null tensor");
    TRAMBA_PB_SHAPE_CHECKS("patch_conv_dgrad_cl");
    TRAMBA_CHECK(aligned16(gy) && aligned16(w) && aligned16(gx), "patch_conv_dgrad_cl: tensors must be 16-byte aligned");
    const int ho = hin / r, wo = win / r, k = r * r * cin;
    const long m = (long)batch * ho * wo;
    dim3 grid((unsigned)((k + kPbWaves * kPbCols - 1) / (kPbWaves * kPbCols)), (unsigned)((m + kPbRows - 1) / kPbRows));
    const long units = (long)batch * ((long)hin * win - (long)(r * ho) * (r * wo)) * (cin / 8);
    hipStream_t s = (hipStream_t)stream;
#define TRAMBA_PB_LAUNCH(T)                                                                                              \
    do {                                                                                                                 \
        hipLaunchKernelGGL((patch_conv_dgrad_kernel<T>), grid, dim3(kPbWaves * 64), 0, s, (const T *)gy, (const T *)w,    \
                           (T *)gx, (int)m, hin, win, cin, cout, r, ho, wo);                                             \
        if (units > 0)                                                                                                   \
            hipLaunchKernelGGL((patch_conv_dgrad_tail_kernel<T>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, \
                               (T *)gx, units, hin, win, cin, r * ho, r * wo);                                           \
    } while (0)
    if (dtype == TRAMBA_BF16) TRAMBA_PB_LAUNCH(__hip_bfloat16);
    else TRAMBA_PB_LAUNCH(__half);
#undef TRAMBA_PB_LAUNCH
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_patch_conv_wgrad_split(int batch, int hin, int win, int cin, int cout, int r)
{
    if (!pb_shape_ok(batch, hin, win, cin, cout, r)) return 0;
    int sps, nsplit;
    pb_wgrad_plan((long)batch * (hin / r) * (win / r), r * r * cin, cout, sps, nsplit);
    return nsplit;
}

extern "C" size_t tramba_patch_conv_wgrad_work(int batch, int hin, int win, int cin, int cout, int r)
{
    const int nsplit = tramba_patch_conv_wgrad_split(batch, hin, win, cin, cout, r);
    return (size_t)nsplit * ((size_t)cout * r * r * cin + cout) * sizeof(float);
}

extern "C" int tramba_patch_conv_wgrad_cl(const void *gy, const void *x, float *work, size_t work_bytes, int batch, int hin,
                                          int win, int cin, int cout, int r, int want_bias, int dtype, void *stream)
{
    TRAMBA_CHECK(gy && x, "patch_conv_wgrad_cl: null tensor");
    TRAMBA_PB_SHAPE_CHECKS("patch_conv_wgrad_cl");
    TRAMBA_CHECK(aligned16(gy) && aligned16(x) && aligned16(work), "patch_conv_wgrad_cl: tensors must be 16-byte aligned");
    const size_t need = tramba_patch_conv_wgrad_work(batch, hin, win, cin, cout, r);
    TRAMBA_CHECK(work && work_bytes >= need, "patch_conv_wgrad_cl: workspace of %zu bytes needed, %zu given", need,
                 work ? work_bytes : (size_t)0);
    const int ho = hin / r, wo = win / r, k = r * r * cin;
    const long m = (long)batch * ho * wo;
    int sps, nsplit;
    pb_wgrad_plan(m, k, cout, sps, nsplit);
    dim3 grid((unsigned)(k / kPbCols), (unsigned)((cout + kPbCols - 1) / kPbCols), (unsigned)nsplit);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16)
        hipLaunchKernelGGL((patch_conv_wgrad_kernel<__hip_bfloat16>), grid, dim3(kPbWaves * 64), 0, s,
                           (const __hip_bfloat16 *)gy, (const __hip_bfloat16 *)x, work, (int)m, hin, win, cin, cout, r, ho, wo,
                           sps, want_bias);
    else
        hipLaunchKernelGGL((patch_conv_wgrad_kernel<__half>), grid, dim3(kPbWaves * 64), 0, s, (const __half *)gy,
                           (const __half *)x, work, (int)m, hin, win, cin, cout, r, ho, wo, sps, want_bias);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
