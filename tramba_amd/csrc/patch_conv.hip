// Dense convolutions of the Swin-B / PVTv2-b4 encoders (16-bit inference; encoders.set_library_convolutions).
//
// (a) tramba_patch_conv_cl: kernel = stride = r convolution on a channels-last map -- PVT's spatial-reduction `sr`
//     (pvtv2_encoder.py:76-78,103-106).  As a GEMM: row = output token (b, i, j), column k = (di r + dj) Cin + c, and one
//     kernel row `di` of one token is r Cin contiguous elements of x, so the operand fragments of mfma_f32_16x16x32 are
//     16-byte reads of x and of the K-major weight as they lie: no im2col, no NCHW copy, no LDS staging.
//     The workload is small-M deep-K (144 tokens per image, K = 1280 .. 4096): a workgroup owns 16 tokens x 64 columns and
//     its waves split K between them by 64-deep steps (wave w takes steps w, w + NW, ...).  Each wave accumulates in f32;
//     the partial tiles are added through LDS in wave order 0 .. NW-1, the bias is added last and the sum is rounded
//     once.  No atomics and no hand-off between workgroups: the result is a fixed function of the inputs.
// (b) tramba_patch_embed_ln: the first-layer patch embedding fused with its LayerNorm -- PVT patch_embed1 (7x7 / 4 / pad 3,
//     3 -> 64, pvtv2_encoder.py:159-199) and Swin patch_embed (4x4 / 4, 3 -> 128, swin_encoder.py:413-450).  Modelled on
//     stem.hip: the image is read in NCHW as it lies, the filter sits in LDS tap-major, Cout / 16 lanes share one output
//     pixel and the LayerNorm reduction is lane shuffles across them.  Convolution, bias and LayerNorm in f32, one
//     rounding at the store.
#include "common.h"

namespace tramba {

typedef __attribute__((ext_vector_type(8))) short pc_frag8;
typedef __attribute__((ext_vector_type(4))) float pc_acc4;

template <typename T> struct PcMfma;
template <> struct PcMfma<__hip_bfloat16> {
    static __device__ __forceinline__ pc_acc4 run(pc_frag8 a, pc_frag8 b, pc_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) __bf16 bf8;
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
    }
};
template <> struct PcMfma<__half> {
    static __device__ __forceinline__ pc_acc4 run(pc_frag8 a, pc_frag8 b, pc_acc4 c)
    {
        typedef __attribute__((ext_vector_type(8))) _Float16 h8;
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
    }
};

constexpr int kPcRows = 16, kPcCols = 64, kPcSub = kPcCols / 16;

// the operand fragments of one 64-deep K step: two 32-deep MFMA steps, one x fragment and kPcSub weight fragments each
struct PcStep {
    pc_frag8 a[2];
    pc_frag8 b[2][kPcSub];
};

template <typename T>
__device__ __forceinline__ void pc_load(PcStep &f, const T *__restrict__ xrow, const T *__restrict__ wcol, unsigned xoff,
                                        unsigned woff, unsigned wsub, const bool (&colok)[kPcSub])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f.a[h] = *reinterpret_cast<const pc_frag8 *>(xrow + xoff + 32 * h);
#pragma unroll
        for (int j = 0; j < kPcSub; ++j) {
            pc_frag8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            f.b[h][j] = colok[j] ? *reinterpret_cast<const pc_frag8 *>(wcol + (size_t)j * wsub + woff + 32 * h) : z;
        }
    }
}

// grid (column blocks of 64, token tiles of 16); NW waves per workgroup.
template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) void patch_conv_kernel(const T *__restrict__ x, const T *__restrict__ w,
                                                            const float *__restrict__ bias, T *__restrict__ y, int M,
                                                            int H, int W, int Cin, int Cout, int r, int Ho, int Wo)
{
    __shared__ __attribute__((aligned(16))) float red[NW][kPcRows][kPcCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * kPcCols, m0 = blockIdx.y * kPcRows;
    const int rc = r * Cin;                   // one kernel row of one token: contiguous in x
    const int K = r * rc;
    const int steps = K >> 6, row_steps = rc >> 6;

    // this lane's operand rows: token (clamped: rows past M compute a copy of the last token and are never stored) and
    // weight column (columns past Cout read nothing)
    int tok = m0 + (lane & 15);
    tok = tok < M ? tok : M - 1;
    const int j = tok % Wo, t2 = tok / Wo, i = t2 % Ho, b = t2 / Ho;
    const T *xrow = x + (((size_t)b * H + (size_t)i * r) * W + (size_t)j * r) * Cin + 8 * (lane >> 4);
    bool colok[kPcSub];
#pragma unroll
    for (int s = 0; s < kPcSub; ++s) colok[s] = n0 + 16 * s + (lane & 15) < Cout;
    const T *wcol = w + (size_t)(n0 + (lane & 15)) * K + 8 * (lane >> 4);
    const unsigned wsub = 16u * (unsigned)K, xrowstride = (unsigned)W * Cin;

    pc_acc4 acc[kPcSub];
#pragma unroll
    for (int s = 0; s < kPcSub; ++s) acc[s] = pc_acc4{0.f, 0.f, 0.f, 0.f};

    // step t covers k = 64 t .. 64 t + 63 = kernel row di, elements 64 rem .. of that row (wave-uniform scalars)
    int t = wave, di = wave / row_steps, rem = wave % row_steps;
    PcStep cur, nxt;
    if (t < steps) pc_load(cur, xrow, wcol, di * xrowstride + 64u * rem, 64u * t, wsub, colok);
    nxt = cur;
    while (t < steps) {
        const int tn = t + NW;
        rem += NW;
        while (rem >= row_steps) {
            rem -= row_steps;
            ++di;
        }
        if (tn < steps) pc_load(nxt, xrow, wcol, di * xrowstride + 64u * rem, 64u * tn, wsub, colok);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < kPcSub; ++s) acc[s] = PcMfma<T>::run(cur.a[h], cur.b[h][s], acc[s]);
        cur = nxt;
        t = tn;
    }

    // partial tiles -> LDS (accumulator element q of lane l is row 4 (l >> 4) + q, column l & 15 of its 16 x 16 block)
#pragma unroll
    for (int s = 0; s < kPcSub; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave][4 * (lane >> 4) + q][16 * s + (lane & 15)] = acc[s][q];
    __syncthreads();

    // 128 threads add the NW partials in wave order, 8 columns of one row each; bias last; one rounding
    if (threadIdx.x < kPcRows * (kPcCols / 8)) {
        const int row = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * 8;
        float o[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) o[v] = red[0][row][c0 + v];
#pragma unroll 4
        for (int p = 1; p < NW; ++p)
#pragma unroll
            for (int v = 0; v < 8; ++v) o[v] += red[p][row][c0 + v];
        if (m0 + row < M && n0 + c0 < Cout) {       // Cout % 8 == 0: a group of 8 columns is inside or outside as a whole
            if (bias)
#pragma unroll
                for (int v = 0; v < 8; ++v) o[v] += bias[n0 + c0 + v];
            store_pack<T, 8>(y + (size_t)(m0 + row) * Cout + n0 + c0, o);
        }
    }
}

// First-layer patch embedding + LayerNorm.  COUT / 16 lanes share one output pixel, 16 output channels each.
template <typename TI, typename T, int KS, int STRIDE, int PAD, int COUT>
__global__ __launch_bounds__(256) void patch_embed_ln_kernel(const TI *__restrict__ img, const float *__restrict__ w,
                                                            const float *__restrict__ bias,
                                                            const float *__restrict__ ln_w,
                                                            const float *__restrict__ ln_b, T *__restrict__ y, int B,
                                                            int H, int W, int Ho, int Wo, float eps)
{
    constexpr int TAPS = 3 * KS * KS, LPP = COUT / 16, PPB = 256 / LPP;
    __shared__ __attribute__((aligned(16))) float wl[TAPS][COUT];  // [ci*KS*KS + ky*KS + kx][cout]
    for (int t = threadIdx.x; t < TAPS * COUT; t += blockDim.x) {
        const int co = t / TAPS, tap = t % TAPS;  // reference layout (Cout, 3, KS, KS)
        wl[tap][co] = w[t];
    }
    __syncthreads();
    const long pix = (long)blockIdx.x * PPB + threadIdx.x / LPP;
    const int part = threadIdx.x % LPP;
    const long npix = (long)B * Ho * Wo;
    const bool ok = pix < npix;
    const long pp = ok ? pix : npix - 1;
    const int wo = (int)(pp % Wo);
    const long t2 = pp / Wo;
    const int ho = (int)(t2 % Ho), b = (int)(t2 / Ho);

    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    // (one filter row per trip, NOT unrolled: see stem.hip)
#pragma unroll 1
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky) {
            const int hy = STRIDE * ho + ky - PAD;
            if (hy < 0 || hy >= H) continue;       // a padding tap reads nothing and adds nothing
            const TI *irow = img + (((long)b * 3 + ci) * H + hy) * W;
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                const int wx = STRIDE * wo + kx - PAD;
                float v = 0.f;
                if (wx >= 0 && wx < W) v = Cvt<TI>::to_f(irow[wx]);
                const float4 *wp = reinterpret_cast<const float4 *>(&wl[(ci * KS + ky) * KS + kx][part * 16]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 ww = wp[q];
                    acc[4 * q + 0] = fmaf(v, ww.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = fmaf(v, ww.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(v, ww.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(v, ww.w, acc[4 * q + 3]);
                }
            }
        }
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] += bias[part * 16 + j];
    // LayerNorm over the COUT channels of the pixel = LPP lanes x 16
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += acc[j];
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) s += __shfl_xor(s, o, LPP);
    const float mean = s * (1.f / COUT);
    float q2 = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float d = acc[j] - mean;
        q2 = fmaf(d, d, q2);
    }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) q2 += __shfl_xor(q2, o, LPP);
    const float rstd = rsqrtf(q2 * (1.f / COUT) + eps);
    if (!ok) return;
    T *yo = y + pix * COUT + part * 16;
#pragma unroll
    for (int h8 = 0; h8 < 2; ++h8) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = part * 16 + h8 * 8 + j;
            o[j] = (acc[h8 * 8 + j] - mean) * rstd * ln_w[c] + ln_b[c];
        }
        store_pack<T, 8>(yo + h8 * 8, o);
    }
}

template <typename TI, typename T>
static void launch_patch_embed(int k, const void *img, const float *w, const float *bias, const float *ln_w,
                               const float *ln_b, void *y, int batch, int h, int wd, int ho, int wo, float eps,
                               hipStream_t s)
{
    const long npix = (long)batch * ho * wo;
    if (k == 7) {
        dim3 grid((unsigned)((npix + 63) / 64)), block(256);
        hipLaunchKernelGGL((patch_embed_ln_kernel<TI, T, 7, 4, 3, 64>), grid, block, 0, s, (const TI *)img, w, bias, ln_w,
                           ln_b, (T *)y, batch, h, wd, ho, wo, eps);
    } else {
        dim3 grid((unsigned)((npix + 31) / 32)), block(256);
        hipLaunchKernelGGL((patch_embed_ln_kernel<TI, T, 4, 4, 0, 128>), grid, block, 0, s, (const TI *)img, w, bias, ln_w,
                           ln_b, (T *)y, batch, h, wd, ho, wo, eps);
    }
}

}  // namespace tramba

using namespace tramba;

extern "C" int tramba_patch_conv_cl(const void *x, const void *w, const float *bias, void *y, int batch, int hin, int win,
                                    int cin, int cout, int r, int dtype, void *stream)
{
    TRAMBA_CHECK(x && w && y, "patch_conv_cl: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "patch_conv_cl: bf16/f16 only");
    TRAMBA_CHECK(r >= 2 && r <= 8, "patch_conv_cl: kernel = stride = %d must be in 2..8", r);
    TRAMBA_CHECK(batch > 0 && cin > 0 && cout > 0 && hin >= r && win >= r, "patch_conv_cl: empty shape");
    TRAMBA_CHECK(cin % 64 == 0, "patch_conv_cl: Cin=%d must be a multiple of 64", cin);
    TRAMBA_CHECK(cout % 8 == 0, "patch_conv_cl: Cout=%d must be a multiple of 8", cout);
    TRAMBA_CHECK((double)batch * hin * win * cin * 2.0 < 2147483648.0, "patch_conv_cl: input map beyond 32-bit byte offsets");
    const int ho = hin / r, wo = win / r;
    const long m = (long)batch * ho * wo;
    const int k = r * r * cin;
    TRAMBA_CHECK((m + kPcRows - 1) / kPcRows <= 65535 && (double)cout * k * 2.0 < 2147483648.0,
                 "patch_conv_cl: too many output tokens or weights");
    TRAMBA_CHECK(aligned16(x) && aligned16(w) && aligned16(y), "patch_conv_cl: tensors must be 16-byte aligned");
    dim3 grid((unsigned)((cout + kPcCols - 1) / kPcCols), (unsigned)((m + kPcRows - 1) / kPcRows));
    hipStream_t s = (hipStream_t)stream;
    // 16 waves where K is deep enough to give each of them two 64-deep steps, 8 otherwise
#define TRAMBA_PC_LAUNCH(T)                                                                                              \
    do {                                                                                                                 \
        if (k >= 2048)                                                                                                   \
            hipLaunchKernelGGL((patch_conv_kernel<T, 16>), grid, dim3(1024), 0, s, (const T *)x, (const T *)w, bias,      \
                               (T *)y, (int)m, hin, win, cin, cout, r, ho, wo);                                          \
        else                                                                                                             \
            hipLaunchKernelGGL((patch_conv_kernel<T, 8>), grid, dim3(512), 0, s, (const T *)x, (const T *)w, bias,        \
                               (T *)y, (int)m, hin, win, cin, cout, r, ho, wo);                                          \
    } while (0)
    if (dtype == TRAMBA_BF16) TRAMBA_PC_LAUNCH(__hip_bfloat16);
    else TRAMBA_PC_LAUNCH(__half);
#undef TRAMBA_PC_LAUNCH
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_patch_embed_ln(const void *img, const float *w, const float *bias, const float *ln_w,
                                     const float *ln_b, void *y, int batch, int h, int wd, int k, int stride, int pad,
                                     int cout, float eps, int img_dtype, int dtype, void *stream)
{
    TRAMBA_CHECK(img && w && bias && ln_w && ln_b && y, "patch_embed_ln: null tensor");
    TRAMBA_CHECK(dtype == TRAMBA_BF16 || dtype == TRAMBA_F16, "patch_embed_ln: bf16/f16 output only");
    TRAMBA_CHECK(img_dtype == TRAMBA_F32 || img_dtype == dtype, "patch_embed_ln: image must be f32 or the activation dtype");
    TRAMBA_CHECK((k == 7 && stride == 4 && pad == 3 && cout == 64) || (k == 4 && stride == 4 && pad == 0 && cout == 128),
                 "patch_embed_ln: (k, stride, pad, Cout) = (%d, %d, %d, %d) is neither PVT's (7, 4, 3, 64) nor Swin's "
                 "(4, 4, 0, 128)", k, stride, pad, cout);
    TRAMBA_CHECK(batch > 0 && h + 2 * pad >= k && wd + 2 * pad >= k, "patch_embed_ln: empty shape");
    const int ho = (h + 2 * pad - k) / stride + 1, wo = (wd + 2 * pad - k) / stride + 1;
    TRAMBA_CHECK((double)batch * ho * wo / 32.0 < 2147483647.0 && (double)batch * 3.0 * h * wd < 9.0e18,
                 "patch_embed_ln: too many pixels");
    TRAMBA_CHECK(aligned16(y), "patch_embed_ln: output must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16) {
        using T = __hip_bfloat16;
        if (img_dtype == TRAMBA_F32) launch_patch_embed<float, T>(k, img, w, bias, ln_w, ln_b, y, batch, h, wd, ho, wo, eps, s);
        else launch_patch_embed<T, T>(k, img, w, bias, ln_w, ln_b, y, batch, h, wd, ho, wo, eps, s);
    } else {
        using T = __half;
        if (img_dtype == TRAMBA_F32) launch_patch_embed<float, T>(k, img, w, bias, ln_w, ln_b, y, batch, h, wd, ho, wo, eps, s);
        else launch_patch_embed<T, T>(k, img, w, bias, ln_w, ln_b, y, batch, h, wd, ho, wo, eps, s);
    }
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
