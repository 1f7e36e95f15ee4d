// Training-mode batch norm and the stem's max pool of the ResNet-50 encoder on channels-last maps (Tramba-R, 16-bit training;
// resnet_encoder.py:62-110, where nn.BatchNorm2d runs on batch statistics under model.train()).
//
// A map is (M = B H W, C) in bf16 / fp16 with C % 8 == 0; all arithmetic is f32.  One geometry serves every batch-norm kernel:
// a workgroup of 256 threads is 32 rows x 8 lanes, a lane owns 8 contiguous channels (one 16-byte access), so a workgroup
// covers 64 channels = one 128-byte line per row, and grid.y walks the channels in blocks of 64.
//
// (a) tramba_bn_stats_cl: per-channel batch mean and biased variance, TWO passes: sum of x, then sum of (x - mean)^2 -- never
//     E[x^2] - E[x]^2, whose cancellation costs mean^2 / var digits.  The rows are dealt in P contiguous runs to P workgroups per
//     channel block; a run is added row block by row block in registers, its 32 row lanes through LDS in lane order, and the P
//     partials in index order: a fixed function of the input, no atomics.  The second pass re-derives the mean from the first
//     pass's partials in its prologue (P <= 64 floats per channel), so the statistics are 3 launches: sums, squares, finish.
//     The finish writes mean and rstd = 1 / sqrt(var + eps) and, when given, updates the running buffers in place on the
//     device (momentum m: running = (1 - m) running + m new, the variance unbiased by M / (M - 1)).
//     Bytes: 2 M C read twice (the second time from L2 / MALL for the workload's maps of at most 19 MB) + 8 P C of partials.
// (b) tramba_bn_act_cl: y = act(gamma (x - mean) rstd + beta + residual), one launch, 2 M C read (4 with a residual), 2 M C
//     written, one rounding.
// (c) tramba_bn_act_bwd_cl: with dy' = dy masked by y > 0 (ReLU) and xh = (x - mean) rstd:
//       launch 1: partial channel sums of dy' and dy' xh per row run (as in (a));
//       launch 2: the partials in index order -> dbeta, dgamma (also kept in the workspace: a frozen affine still needs them);
//       launch 3: dx = gamma rstd (dy' - dbeta / M - xh dgamma / M), and dres = dy' when asked.
//     Bytes: launch 1 reads dy, x (and y): 4 .. 6 M C; launch 3 reads them again and writes dx (and dres): 6 .. 10 M C.
// (d) tramba_maxpool3s2_cl / _bwd_cl: max_pool2d(3, 2, 1).  Forward: a lane owns 8 channels of one output pixel and takes the
//     first maximum of its window in row-major order (a later tap replaces the maximum only when strictly greater, or NaN: the
//     framework's rule); padding taps are never formed.  Backward in gather form: a lane owns 8 channels of one INPUT pixel,
//     visits the at most 2 x 2 windows that cover it, recomputes each window's arg-max from the saved input by the forward's
//     loop and adds gy where the arg-max is this pixel (f32, one rounding).  Nothing is scattered; every gx element is written.
#include "common.h"

namespace tramba {

constexpr int kBnLanes = 8, kBnRows = 32, kBnThreads = kBnLanes * kBnRows, kBnCols = 8 * kBnLanes;
constexpr int kBnMaxParts = 64;      // row runs per channel block (statistics, backward sums)
constexpr int kBnIter = 4;           // row blocks per workgroup of the element-wise kernels
static_assert(kBnThreads == 256 && kBnCols == 64, "batch-norm geometry");

// the row runs of an (M, C) map: P runs of `rows` rows (a multiple of the row block; trailing runs may be empty)
struct BnSplit {
    int parts;
    long rows;
    int cpad;                        // C rounded up to the channel block: the row length of the partial tables
};
static BnSplit bn_split(long m, int c)
{
    long p = m / (4 * kBnRows);
    p = p < 1 ? 1 : p > kBnMaxParts ? kBnMaxParts : p;
    long rows = (m + p - 1) / p;
    rows = (rows + kBnRows - 1) / kBnRows * kBnRows;
    return {(int)p, rows, (c + kBnCols - 1) / kBnCols * kBnCols};
}

// sum of the P partials of one channel, in index order: 8 independent loads in flight, then added in that order (one load
// per addition would pay the L2 latency P times; the order of the additions, and so the bits, are those of the plain loop)
__device__ __forceinline__ float bn_sum_parts(const float *__restrict__ part, int parts, int cpad, int c)
{
    float s = 0.f;
    int p = 0;
    for (; p + 8 <= parts; p += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[(size_t)(p + j) * cpad + c];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; p < parts; ++p) s += part[(size_t)p * cpad + c];
    return s;
}

// the 32 row lanes of a workgroup through LDS, added in lane order by the first 64 threads (one channel each)
__device__ __forceinline__ float bn_block_sum(float (*red)[kBnCols], const float (&acc)[8], int r, int g)
{
    __syncthreads();                 // (red may still be read from a previous use)
    float4 *dst = reinterpret_cast<float4 *>(&red[r][8 * g]);
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < kBnCols)
        for (int rr = 0; rr < kBnRows; ++rr) s += red[rr][threadIdx.x];
    return s;
}

// grid (P, channel blocks).  VAR = false: out[p][c] = sum over run p of x; VAR = true: of (x - mean)^2 with the mean from `sums`
template <typename T, bool VAR>
__global__ __launch_bounds__(kBnThreads) void bn_colsum_kernel(const T *__restrict__ x, const float *__restrict__ sums,
                                                               float *__restrict__ out, long M, int C, int cpad, long rows,
                                                               int parts)
{
    __shared__ __attribute__((aligned(16))) float red[kBnRows][kBnCols];
    __shared__ float mean_s[kBnCols];
    const int g = threadIdx.x & (kBnLanes - 1), r = threadIdx.x / kBnLanes;
    const int cb = blockIdx.y * kBnCols, c0 = cb + 8 * g;
    float mu[8], acc[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) mu[v] = acc[v] = 0.f;
    if (VAR) {
        if (threadIdx.x < kBnCols) mean_s[threadIdx.x] = bn_sum_parts(sums, parts, cpad, cb + threadIdx.x) / (float)M;
        __syncthreads();
#pragma unroll
        for (int v = 0; v < 8; ++v) mu[v] = mean_s[8 * g + v];
    }
    const long r0 = (long)blockIdx.x * rows, r1 = r0 + rows < M ? r0 + rows : M;
    if (c0 < C) {
#pragma unroll 4
        for (long row = r0 + r; row < r1; row += kBnRows) {
            float v[8];
            load_pack<T, 8>(x + (size_t)row * C + c0, v);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float d = v[k] - mu[k];
                acc[k] += VAR ? d * d : d;
            }
        }
    }
    const float s = bn_block_sum(red, acc, r, g);
    if (threadIdx.x < kBnCols) out[(size_t)blockIdx.x * cpad + cb + threadIdx.x] = s;
}

// one thread per channel: the partials in index order -> mean, rstd, running buffers
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const float *__restrict__ sums, const float *__restrict__ sqs,
                                                              float *__restrict__ mean, float *__restrict__ rstd,
                                                              float *__restrict__ running_mean,
                                                              float *__restrict__ running_var, long M, int C, int cpad,
                                                              int parts, float eps, float momentum, float unbias)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float mu = bn_sum_parts(sums, parts, cpad, c) / (float)M;        // (the expression of bn_colsum_kernel<VAR>)
    const float var = bn_sum_parts(sqs, parts, cpad, c) / (float)M;
    mean[c] = mu;
    rstd[c] = 1.f / sqrtf(var + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (var * unbias);
}

// per-lane channel constants of the element-wise kernels
struct BnChan {
    float mu[8], rs[8];
};
__device__ __forceinline__ void bn_load_chan(BnChan &ch, const float *__restrict__ mean, const float *__restrict__ rstd, int c0)
{
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        ch.mu[v] = mean[c0 + v];
        ch.rs[v] = rstd[c0 + v];
    }
}

// grid (row blocks of 32 x kBnIter, channel blocks)
template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn_act_kernel(const T *__restrict__ x, const float *__restrict__ mean,
                                                            const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const T *__restrict__ residual,
                                                            T *__restrict__ y, long M, int C, int relu)
{
    const int g = threadIdx.x & (kBnLanes - 1), r = threadIdx.x / kBnLanes;
    const int c0 = blockIdx.y * kBnCols + 8 * g;
    if (c0 >= C) return;
    BnChan ch;
    bn_load_chan(ch, mean, rstd, c0);
    float a[8], b[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        a[v] = (gamma ? gamma[c0 + v] : 1.f) * ch.rs[v];
        b[v] = beta ? beta[c0 + v] : 0.f;
    }
    const long base = (long)blockIdx.x * (kBnRows * kBnIter) + r;
#pragma unroll
    for (int it = 0; it < kBnIter; ++it) {
        const long row = base + (long)it * kBnRows;
        if (row >= M) break;
        const size_t off = (size_t)row * C + c0;
        float v[8], res[8];
        load_pack<T, 8>(x + off, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) res[k] = 0.f;
        if (residual) load_pack<T, 8>(residual + off, res);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float o = fmaf(v[k] - ch.mu[k], a[k], b[k]) + res[k];
            v[k] = relu ? fmaxf(o, 0.f) : o;
        }
        store_pack<T, 8>(y + off, v);
    }
}

// dy' and xh of 8 channels of one row
template <typename T>
__device__ __forceinline__ void bn_bwd_load(const T *__restrict__ dy, const T *__restrict__ x, const T *__restrict__ y, size_t off,
                                            const BnChan &ch, int relu, float (&d)[8], float (&xh)[8])
{
    float xv[8];
    load_pack<T, 8>(dy + off, d);
    load_pack<T, 8>(x + off, xv);
    if (relu) {
        float yv[8];
        load_pack<T, 8>(y + off, yv);
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = yv[k] > 0.f ? d[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) xh[k] = (xv[k] - ch.mu[k]) * ch.rs[k];
}

// grid (P, channel blocks): pa[p][c] = sum over run p of dy', pb[p][c] = of dy' xh
template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_sums_kernel(const T *__restrict__ dy, const T *__restrict__ x,
                                                                 const T *__restrict__ y, const float *__restrict__ mean,
                                                                 const float *__restrict__ rstd, float *__restrict__ pa,
                                                                 float *__restrict__ pb, long M, int C, int cpad, long rows,
                                                                 int relu)
{
    __shared__ __attribute__((aligned(16))) float red[kBnRows][kBnCols];
    const int g = threadIdx.x & (kBnLanes - 1), r = threadIdx.x / kBnLanes;
    const int cb = blockIdx.y * kBnCols, c0 = cb + 8 * g;
    float a1[8], a2[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) a1[v] = a2[v] = 0.f;
    const long r0 = (long)blockIdx.x * rows, r1 = r0 + rows < M ? r0 + rows : M;
    if (c0 < C) {
        BnChan ch;
        bn_load_chan(ch, mean, rstd, c0);
#pragma unroll 2
        for (long row = r0 + r; row < r1; row += kBnRows) {
            float d[8], xh[8];
            bn_bwd_load<T>(dy, x, y, (size_t)row * C + c0, ch, relu, d, xh);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a1[k] += d[k];
                a2[k] = fmaf(d[k], xh[k], a2[k]);
            }
        }
    }
    const float s1 = bn_block_sum(red, a1, r, g);
    const float s2 = bn_block_sum(red, a2, r, g);
    if (threadIdx.x < kBnCols) {
        pa[(size_t)blockIdx.x * cpad + cb + threadIdx.x] = s1;
        pb[(size_t)blockIdx.x * cpad + cb + threadIdx.x] = s2;
    }
}

// one thread per channel: sums[0][c] = dbeta, sums[1][c] = dgamma (partials in index order)
__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const float *__restrict__ pa, const float *__restrict__ pb,
                                                            float *__restrict__ sums, float *__restrict__ dgamma,
                                                            float *__restrict__ dbeta, int C, int cpad, int parts)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float s1 = bn_sum_parts(pa, parts, cpad, c), s2 = bn_sum_parts(pb, parts, cpad, c);
    sums[c] = s1;
    sums[cpad + c] = s2;
    if (dbeta) dbeta[c] = s1;
    if (dgamma) dgamma[c] = s2;
}

// grid (row blocks of 32 x kBnIter, channel blocks)
template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_dx_kernel(const T *__restrict__ dy, const T *__restrict__ x,
                                                               const T *__restrict__ y, const float *__restrict__ mean,
                                                               const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                               const float *__restrict__ sums, T *__restrict__ dx,
                                                               T *__restrict__ dres, long M, int C, int cpad, int relu)
{
    const int g = threadIdx.x & (kBnLanes - 1), r = threadIdx.x / kBnLanes;
    const int c0 = blockIdx.y * kBnCols + 8 * g;
    if (c0 >= C) return;
    BnChan ch;
    bn_load_chan(ch, mean, rstd, c0);
    float k0[8], m1[8], m2[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        k0[v] = (gamma ? gamma[c0 + v] : 1.f) * ch.rs[v];
        m1[v] = sums[c0 + v] / (float)M;
        m2[v] = sums[cpad + c0 + v] / (float)M;
    }
    const long base = (long)blockIdx.x * (kBnRows * kBnIter) + r;
#pragma unroll
    for (int it = 0; it < kBnIter; ++it) {
        const long row = base + (long)it * kBnRows;
        if (row >= M) break;
        const size_t off = (size_t)row * C + c0;
        float d[8], xh[8], o[8];
        bn_bwd_load<T>(dy, x, y, off, ch, relu, d, xh);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = k0[k] * (d[k] - m1[k] - xh[k] * m2[k]);
        store_pack<T, 8>(dx + off, o);
        if (dres) store_pack<T, 8>(dres + off, d);
    }
}

// ---- max_pool2d(3, 2, 1) ----
// the window of output pixel (oi, oj): the first maximum in row-major order and its tap index 3 di + dj
template <typename T>
__device__ __forceinline__ void pool_window(const T *__restrict__ img, int oi, int oj, int H, int W, int C, float (&best)[8],
                                            int (&arg)[8])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        best[k] = -INFINITY;
        arg[k] = -1;
    }
#pragma unroll
    for (int di = 0; di < 3; ++di) {
        const int iy = 2 * oi - 1 + di;
        if (iy < 0 || iy >= H) continue;                            // padding never wins: it is never looked at
#pragma unroll
        for (int dj = 0; dj < 3; ++dj) {
            const int ix = 2 * oj - 1 + dj;
            if (ix < 0 || ix >= W) continue;
            float v[8];
            load_pack<T, 8>(img + ((size_t)iy * W + ix) * C, v);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (v[k] > best[k] || v[k] != v[k]) {
                    best[k] = v[k];
                    arg[k] = 3 * di + dj;
                }
        }
    }
}

// one thread per (output pixel, 8 channels)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T *__restrict__ x, T *__restrict__ y, long total, int H, int W,
                                                          int C, int Ho, int Wo)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cg = C >> 3, g = (int)(idx % cg);
    long pix = idx / cg;
    const int oj = (int)(pix % Wo);
    pix /= Wo;
    const int oi = (int)(pix % Ho), b = (int)(pix / Ho);
    float best[8];
    int arg[8];
    pool_window<T>(x + (size_t)b * H * W * C + 8 * g, oi, oj, H, W, C, best, arg);
    store_pack<T, 8>(y + (((size_t)b * Ho + oi) * Wo + oj) * C + 8 * g, best);
}

// one thread per (input pixel, 8 channels)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T *__restrict__ gy, const T *__restrict__ x, T *__restrict__ gx,
                                                          long total, int H, int W, int C, int Ho, int Wo)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int cg = C >> 3, g = (int)(idx % cg);
    long pix = idx / cg;
    const int j = (int)(pix % W);
    pix /= W;
    const int i = (int)(pix % H), b = (int)(pix / H);
    const T *img = x + (size_t)b * H * W * C + 8 * g;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    // windows 2 o - 1 .. 2 o + 1 cover pixel p for o = p / 2 and, for odd p, o = p / 2 + 1
    for (int a = 0; a <= (i & 1); ++a) {
        const int oi = (i >> 1) + a;
        if (oi >= Ho) continue;
        for (int c = 0; c <= (j & 1); ++c) {
            const int oj = (j >> 1) + c;
            if (oj >= Wo) continue;
            float best[8], d[8];
            int arg[8];
            pool_window<T>(img, oi, oj, H, W, C, best, arg);
            const int mine = 3 * (i - (2 * oi - 1)) + (j - (2 * oj - 1));
            load_pack<T, 8>(gy + (((size_t)b * Ho + oi) * Wo + oj) * C + 8 * g, d);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += arg[k] == mine ? d[k] : 0.f;
        }
    }
    store_pack<T, 8>(gx + (((size_t)b * H + i) * W + j) * C + 8 * g, acc);
}

static bool bn_shape_ok(const char *what, long m, int c, int dtype)
{
    if (dtype != TRAMBA_BF16 && dtype != TRAMBA_F16) {
        set_error("%s: bf16/f16 only", what);
        return false;
    }
    if (m <= 0 || c <= 0) {
        set_error("%s: empty shape", what);
        return false;
    }
    if (c % 8 != 0) {
        set_error("%s: C=%d must be a multiple of 8", what, c);
        return false;
    }
    if (m >= 2147483647L || (c + kBnCols - 1) / kBnCols > 65535) {
        set_error("%s: too many rows or channels", what);
        return false;
    }
    return true;
}

}  // namespace tramba

using namespace tramba;

extern "C" int tramba_bn_parts(int64_t m, int c)
{
    if (m <= 0 || c <= 0) return 0;
    return bn_split((long)m, c).parts;
}

extern "C" size_t tramba_bn_work(int64_t m, int c)
{
    if (m <= 0 || c <= 0) return 0;
    const BnSplit sp = bn_split((long)m, c);
    return ((size_t)2 * sp.parts + 2) * sp.cpad * sizeof(float);
}

extern "C" int tramba_bn_stats_cl(const void *x, float *mean, float *rstd, float *running_mean, float *running_var, void *work,
                                  size_t work_bytes, int64_t m, int c, float eps, float momentum, int dtype, void *stream)
{
    TRAMBA_CHECK(x && mean && rstd && work, "bn_stats_cl: null tensor");
    if (!bn_shape_ok("bn_stats_cl", (long)m, c, dtype)) return TRAMBA_ERR_ARG;
    TRAMBA_CHECK(m >= 2, "bn_stats_cl: expected more than 1 value per channel when training (M = 1)");
    TRAMBA_CHECK(eps >= 0.f && momentum >= 0.f && momentum <= 1.f, "bn_stats_cl: eps / momentum out of range");
    TRAMBA_CHECK(work_bytes >= tramba_bn_work(m, c), "bn_stats_cl: workspace of %zu bytes, need %zu", work_bytes,
                 tramba_bn_work(m, c));
    TRAMBA_CHECK(aligned16(x) && aligned16(work), "bn_stats_cl: tensors must be 16-byte aligned");
    const BnSplit sp = bn_split((long)m, c);
    float *sums = (float *)work, *sqs = sums + (size_t)sp.parts * sp.cpad;
    dim3 grid((unsigned)sp.parts, (unsigned)(sp.cpad / kBnCols));
    hipStream_t s = (hipStream_t)stream;
    const float unbias = (float)((double)m / (double)(m - 1));
#define TRAMBA_BN_STATS(T)                                                                                                   \
    do {                                                                                                                     \
        hipLaunchKernelGGL((bn_colsum_kernel<T, false>), grid, dim3(kBnThreads), 0, s, (const T *)x, (const float *)nullptr,  \
                           sums, (long)m, c, sp.cpad, sp.rows, sp.parts);                                                    \
        hipLaunchKernelGGL((bn_colsum_kernel<T, true>), grid, dim3(kBnThreads), 0, s, (const T *)x, (const float *)sums, sqs, \
                           (long)m, c, sp.cpad, sp.rows, sp.parts);                                                          \
    } while (0)
    if (dtype == TRAMBA_BF16) TRAMBA_BN_STATS(__hip_bfloat16);
    else TRAMBA_BN_STATS(__half);
#undef TRAMBA_BN_STATS
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, s, (const float *)sums,
                       (const float *)sqs, mean, rstd, running_mean, running_var, (long)m, c, sp.cpad, sp.parts, eps, momentum,
                       unbias);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_bn_act_cl(const void *x, const float *mean, const float *rstd, const float *gamma, const float *beta,
                                const void *residual, void *y, int64_t m, int c, int relu, int dtype, void *stream)
{
    TRAMBA_CHECK(x && mean && rstd && y, "bn_act_cl: null tensor");
    if (!bn_shape_ok("bn_act_cl", (long)m, c, dtype)) return TRAMBA_ERR_ARG;
    TRAMBA_CHECK(aligned16(x) && aligned16(y) && aligned16(residual), "bn_act_cl: tensors must be 16-byte aligned");
    const int rows = kBnRows * kBnIter;
    dim3 grid((unsigned)((m + rows - 1) / rows), (unsigned)((c + kBnCols - 1) / kBnCols));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16)
        hipLaunchKernelGGL((bn_act_kernel<__hip_bfloat16>), grid, dim3(kBnThreads), 0, s, (const __hip_bfloat16 *)x, mean, rstd,
                           gamma, beta, (const __hip_bfloat16 *)residual, (__hip_bfloat16 *)y, (long)m, c, relu != 0);
    else
        hipLaunchKernelGGL((bn_act_kernel<__half>), grid, dim3(kBnThreads), 0, s, (const __half *)x, mean, rstd, gamma, beta,
                           (const __half *)residual, (__half *)y, (long)m, c, relu != 0);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_bn_act_bwd_cl(const void *dy, const void *x, const void *y, const float *mean, const float *rstd,
                                    const float *gamma, void *dx, void *dres, float *dgamma, float *dbeta, void *work,
                                    size_t work_bytes, int64_t m, int c, int relu, int dtype, void *stream)
{
    TRAMBA_CHECK(dy && x && mean && rstd && dx && work, "bn_act_bwd_cl: null tensor");
    TRAMBA_CHECK(!relu || y, "bn_act_bwd_cl: null tensor (the ReLU mask needs y)");
    if (!bn_shape_ok("bn_act_bwd_cl", (long)m, c, dtype)) return TRAMBA_ERR_ARG;
    TRAMBA_CHECK(work_bytes >= tramba_bn_work(m, c), "bn_act_bwd_cl: workspace of %zu bytes, need %zu", work_bytes,
                 tramba_bn_work(m, c));
    TRAMBA_CHECK(aligned16(dy) && aligned16(x) && aligned16(y) && aligned16(dx) && aligned16(dres) && aligned16(work),
                 "bn_act_bwd_cl: tensors must be 16-byte aligned");
    const BnSplit sp = bn_split((long)m, c);
    float *pa = (float *)work, *pb = pa + (size_t)sp.parts * sp.cpad, *sums = pb + (size_t)sp.parts * sp.cpad;
    const int rows = kBnRows * kBnIter;
    dim3 gsum((unsigned)sp.parts, (unsigned)(sp.cpad / kBnCols));
    dim3 gdx((unsigned)((m + rows - 1) / rows), (unsigned)(sp.cpad / kBnCols));
    hipStream_t s = (hipStream_t)stream;
    const int r = relu != 0;
#define TRAMBA_BN_BWD(T)                                                                                                     \
    do {                                                                                                                     \
        hipLaunchKernelGGL((bn_bwd_sums_kernel<T>), gsum, dim3(kBnThreads), 0, s, (const T *)dy, (const T *)x, (const T *)y,  \
                           mean, rstd, pa, pb, (long)m, c, sp.cpad, sp.rows, r);                                             \
        hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, s, (const float *)pa,       \
                           (const float *)pb, sums, dgamma, dbeta, c, sp.cpad, sp.parts);                                    \
        hipLaunchKernelGGL((bn_bwd_dx_kernel<T>), gdx, dim3(kBnThreads), 0, s, (const T *)dy, (const T *)x, (const T *)y,     \
                           mean, rstd, gamma, (const float *)sums, (T *)dx, (T *)dres, (long)m, c, sp.cpad, r);              \
    } while (0)
    if (dtype == TRAMBA_BF16) TRAMBA_BN_BWD(__hip_bfloat16);
    else TRAMBA_BN_BWD(__half);
#undef TRAMBA_BN_BWD
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

static bool pool_shape_ok(const char *what, int batch, int h, int w, int c, int dtype)
{
    if (dtype != TRAMBA_BF16 && dtype != TRAMBA_F16) {
        set_error("%s: bf16/f16 only", what);
        return false;
    }
    if (batch <= 0 || h <= 0 || w <= 0 || c <= 0) {
        set_error("%s: empty shape", what);
        return false;
    }
    if (c % 8 != 0) {
        set_error("%s: C=%d must be a multiple of 8", what, c);
        return false;
    }
    if ((double)batch * h * w * (c / 8) >= 2147483647.0 * 256.0) {
        set_error("%s: too many pixels", what);
        return false;
    }
    return true;
}

extern "C" int tramba_maxpool3s2_cl(const void *x, void *y, int batch, int h, int w, int c, int dtype, void *stream)
{
    TRAMBA_CHECK(x && y, "maxpool3s2_cl: null tensor");
    if (!pool_shape_ok("maxpool3s2_cl", batch, h, w, c, dtype)) return TRAMBA_ERR_ARG;
    TRAMBA_CHECK(aligned16(x) && aligned16(y), "maxpool3s2_cl: tensors must be 16-byte aligned");
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const long total = (long)batch * ho * wo * (c / 8);
    dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16)
        hipLaunchKernelGGL((maxpool_fwd_kernel<__hip_bfloat16>), grid, dim3(256), 0, s, (const __hip_bfloat16 *)x,
                           (__hip_bfloat16 *)y, total, h, w, c, ho, wo);
    else
        hipLaunchKernelGGL((maxpool_fwd_kernel<__half>), grid, dim3(256), 0, s, (const __half *)x, (__half *)y, total, h, w, c,
                           ho, wo);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}

extern "C" int tramba_maxpool3s2_bwd_cl(const void *gy, const void *x, void *gx, int batch, int h, int w, int c, int dtype,
                                        void *stream)
{
    TRAMBA_CHECK(gy && x && gx, "maxpool3s2_bwd_cl: null tensor");
    if (!pool_shape_ok("maxpool3s2_bwd_cl", batch, h, w, c, dtype)) return TRAMBA_ERR_ARG;
    TRAMBA_CHECK(aligned16(gy) && aligned16(x) && aligned16(gx), "maxpool3s2_bwd_cl: tensors must be 16-byte aligned");
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const long total = (long)batch * h * w * (c / 8);
    dim3 grid((unsigned)((total + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == TRAMBA_BF16)
        hipLaunchKernelGGL((maxpool_bwd_kernel<__hip_bfloat16>), grid, dim3(256), 0, s, (const __hip_bfloat16 *)gy,
                           (const __hip_bfloat16 *)x, (__hip_bfloat16 *)gx, total, h, w, c, ho, wo);
    else
        hipLaunchKernelGGL((maxpool_bwd_kernel<__half>), grid, dim3(256), 0, s, (const __half *)gy, (const __half *)x,
                           (__half *)gx, total, h, w, c, ho, wo);
    TRAMBA_LAUNCH_CHECK();
    return TRAMBA_OK;
}
